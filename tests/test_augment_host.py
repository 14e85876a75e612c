"""CPU-side checks of the SSL crops (vtp_amd/augment.py, csrc/augment.hip): the reference the GPU tests compare against
(tests/augment_ref.py) against F.interpolate, closed forms and itself in fp64; the random parameters MultiCrop.draw produces; the
table's layout; the generator state; the argument checks of the class and of the entry points; what the class does without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as A

F32, F64 = torch.float32, torch.float64


# ---- the reference helper ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box,S", [((0, 0, 40, 56), 16), ((3, 5, 30, 41), 48), ((7, 9, 5, 5), 16), ((39, 53, 1, 3), 16),
                                   ((38, 54, 2, 2), 96), ((0, 0, 40, 56), 96), ((0, 0, 16, 128), 16)])
def test_resize_is_interpolate_bicubic_antialias_of_the_crop(box, S):
    """the oracle of the resized crop: crop first, then F.interpolate(bicubic, antialias) -- taps outside the crop are dropped"""
    u8 = A.smooth(1, 40, 56, 1)[0] if box[3] <= 56 else A.smooth(1, 16, 128, 1)[0]
    x = A.to_unit(u8, F64)
    y0, x0, h, w = box
    want = F.interpolate(x[None, :, y0:y0 + h, x0:x0 + w], (S, S), mode="bicubic", antialias=True, align_corners=False)[0].clamp(0, 1)
    got = A.resized_crop(x, box, S)
    assert got.shape == (3, S, S) and float((got - want).abs().max()) < 1e-13
    m = A.resize_matrix(w, S, F64)
    assert m.shape == (S, w) and float((m.sum(1) - 1).abs().max()) < 1e-14
    assert int((m != 0).sum(1).max()) <= 2 * 2 * max(math.ceil(w / S), 1) + 1


@pytest.mark.parametrize("dtype", [F32, F64])
def test_identity_and_flip_are_bit_equal_to_the_plain_normalise(dtype):
    u8 = A.noise(2, 16, 16, 3)
    for b in range(2):
        plain = A.normalise(A.to_unit(u8[b], dtype))
        out, pre = A.crop(u8[b], A.row((0, 0, 16, 16)), 16, dtype)
        assert torch.equal(out, plain) and torch.equal(pre, A.to_unit(u8[b], dtype))
        out, _ = A.crop(u8[b], A.row((0, 0, 16, 16), flip=True), 16, dtype)
        assert torch.equal(out, plain.flip(-1))
    # the same expression the u8 -> image kernel of the tokenizer evaluates: (u8 / 255 - mean) / std with the fp32 constants
    m, s = torch.tensor(A.MEAN).view(3, 1, 1), torch.tensor(A.STD).view(3, 1, 1)
    assert torch.equal(A.crop(u8[0], A.row((0, 0, 16, 16)), 16, F32)[0], (u8[0].permute(2, 0, 1).float() / 255.0 - m) / s)


def test_colour_operations_closed_forms():
    x = torch.tensor([[[0.2, 0.9]], [[0.4, 0.1]], [[0.6, 0.5]]], dtype=F64)  # [3, 1, 2]
    g = A.gray(x)
    assert g.shape == (1, 1, 2) and abs(float(g[0, 0, 0]) - (0.2989 * 0.2 + 0.587 * 0.4 + 0.114 * 0.6)) < 1e-15
    assert torch.equal(A.blend(x, torch.zeros_like(x), 1.0), x) and float(A.blend(x, torch.zeros_like(x), 1.5).max()) == 1.0
    assert float((A.hue(x, 0.0) - x).abs().max()) < 1e-15 and float((A.hue(A.hue(x, 0.3), -0.3) - x).abs().max()) < 1e-15
    flat = torch.full((3, 4, 4), 0.37, dtype=F64)
    assert torch.equal(A.hue(flat, 0.25), flat)  # a gray pixel has no hue to turn
    hsv = A.rgb2hsv(torch.tensor([1.0, 0.0, 0.0], dtype=F64).view(3, 1, 1))
    assert hsv.flatten().tolist() == [0.0, 1.0, 1.0]
    assert A.hue(torch.tensor([1.0, 0.0, 0.0], dtype=F64).view(3, 1, 1), 1 / 3).flatten().tolist() == pytest.approx([0, 1, 0], abs=1e-12)
    # blur: weights sum to one (a constant stays constant), reflect padding (a ramp's border rises)
    assert float((A.blur(torch.full((3, 16, 16), 0.37, dtype=F64), 2.0) - 0.37).abs().max()) < 1e-15
    ramp = torch.arange(16, dtype=F64).expand(3, 16, 16) / 16
    b = A.blur(ramp, 2.0)
    assert float(b[0, 0, 0]) > 0 and abs(float(b[0, 8, 8]) - 0.5) < 1e-12
    assert float((A.blur(ramp, 0.1) - ramp).abs().max()) < 1e-15  # exp(-50) beside the centre tap
    out, pre = A.crop(A.noise(1, 16, 16, 2)[0], A.row((0, 0, 16, 16), solarize=True), 16, F64)
    want = torch.where(pre >= 128 / 255, 1 - pre, pre)
    assert torch.equal(out, A.normalise(want)) and 0.3 < float((pre >= 128 / 255).double().mean()) < 0.7


def _host_crops():
    """144 crops at S = 16 and 32 from the 40 x 56 source: smooth, noise and near-gray images, all 24 orders, three sigmas"""
    src = A.mixed()
    rows = []
    for i, order in enumerate(A.ORDERS):
        box = [(0, 0, 40, 56), (3, 5, 30, 41), (10, 20, 12, 9)][i % 3]
        rows.append(A.row(box, i % 2 == 1, order=order, factors=A.FACTORS, gray=i % 5 == 0, sigma=(0.1, 0.7, 2.0)[i % 3], solarize=i % 4 == 0))
    return src, A._views(3, rows)


def test_fp32_against_fp64_and_the_solarize_band():
    src, table = _host_crops()
    worst, band, total = 0.0, 0, 0
    for S in (16, 32):
        ref, pre, dev = A.deviation(src, S, table)
        keep = A.keep_mask(table, pre)
        sol = torch.tensor([(int(r[4]) & A.SOLARIZE) != 0 for r in table])
        band += int((~keep).sum())
        total += int(sol.sum()) * 3 * S * S
        worst = max(worst, dev)
        assert torch.isfinite(ref).all() and ref.shape == (72, 3, S, S)
    print(f"AUGMENT host: 144 crops, fp32 against fp64 {worst:.2e}; solarize band {band} of {total} pixels = {100.0 * band / total:.3f} %")
    assert worst < 5e-5      # a handful of fp32 ulps of 2.64 through nine stages; the GPU bars take 4 x the per-case value
    assert band < 0.01 * total


def test_fp32_against_fp64_on_the_gpu_cases():
    """the `dev` of every case tests/test_augment_gpu.py runs: small, so that max(4 dev, 2e-6) is a tight bar"""
    for name, (u8, S, table) in A.cases().items():
        if S > 96:
            continue  # the 256 x 256 case is evaluated by the GPU test alone
        ref, pre, dev = A.deviation(u8, S, table)
        print(f"AUGMENT host: {name:18s} crops={len(table):3d} dev32={dev:.2e}")
        assert torch.isfinite(ref).all() and dev < 5e-5, (name, dev)
        assert float((~A.keep_mask(table, pre)).double().mean()) <= 0.01


def test_constant_image_stays_constant():
    u8, S, table = A.cases()["constant_48"]
    out, _ = A.batch(u8, table, S, F32)
    spread = float((out.flatten(2).max(2).values - out.flatten(2).min(2).values).max())
    print(f"AUGMENT host: constant image, spread over a crop {spread:.2e}")
    assert spread < 2e-6


# ---- the random parameters -----------------------------------------------------------------------------------------------------
def test_table_layout_and_round_trip():
    from vtp_amd.augment import ROW, decode_row, encode_row
    assert ROW == 16
    kw = dict(box=(3, 5, 30, 41), flip=True, order=(2, 1, 3, 0), factors=(1.3, 0.7, 1.15, -0.08), gray=True, sigma=1.1, solarize=True)
    r = encode_row(**kw)
    assert r.dtype == np.float32 and r.shape == (16,)
    assert r.tobytes() == A.row(**kw).tobytes()                       # the layout the helper (and the header) write down
    assert r[:9].tolist() == [3, 5, 30, 41, 15, 2, 1, 3, 0] and r[14] == 0 and r[15] == 0
    assert encode_row(**decode_row(r)).tobytes() == r.tobytes()       # encode / decode, bit for bit
    for kw in (dict(box=(0, 0, 1, 1)), dict(box=(1, 2, 3, 4), order=(3,), factors=(1, 1, 1, 0.05)), dict(box=(0, 0, 9, 9), order=(1, 0), sigma=0.3)):
        r = encode_row(**kw)
        assert r.tobytes() == A.row(**kw).tobytes() and encode_row(**decode_row(r)).tobytes() == r.tobytes()
    assert decode_row(encode_row((0, 0, 4, 4)))["order"] is None and decode_row(encode_row((0, 0, 4, 4), order=()))["order"] == []
    for bad in ((0, 0), (4,), (0, 1, 2, 3, 0)):
        with pytest.raises(ValueError, match="order"):
            encode_row((0, 0, 4, 4), order=bad)


def test_draw_boxes_follow_the_policy():
    from vtp_amd.augment import MultiCrop, decode_row
    aug = MultiCrop.dino_default(global_size=32, local_size=16, seed=1)
    Hs, Ws, B = 40, 56, 200
    tg, tl = aug.draw(B, Hs, Ws)
    assert tg.shape == (2 * B, 16) and tl.shape == (8 * B, 16) and tg.dtype == np.float32
    for t, (lo, hi) in ((tg, (0.32, 1.0)), (tl, (0.05, 0.32))):
        for r in t:
            y0, x0, h, w = decode_row(r)["box"]
            assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= Hs and x0 + w <= Ws
            # area and aspect within the ranges, up to the rounding of h and w to whole pixels
            assert lo * Hs * Ws - (h + w) <= h * w <= hi * Hs * Ws + (h + w), (h, w)
            assert (w - 0.5) / (h + 0.5) <= 4 / 3 and (w + 0.5) / (h - 0.5 if h > 1 else 0.5) >= 3 / 4, (h, w)
    assert len({tuple(r[:4]) for r in tl}) > 100  # they do vary


def test_draw_reaches_the_fallback():
    from vtp_amd.augment import MultiCrop, ViewPolicy, decode_row
    # 1.5 to 2 times the image's area with a near-square box never fits: the centre crop, the ratio clamped into the policy's
    for (Hs, Ws), want in (((40, 48), (0, 0, 40, 48)), ((40, 56), (0, 1, 40, 53)), ((20, 80), (0, 26, 20, 27)), ((80, 20), (26, 0, 27, 20))):
        aug = MultiCrop([ViewPolicy(size=16, views=1, scale=(1.5, 2.0))], seed=2)
        (t,) = aug.draw(5, Hs, Ws)
        assert [decode_row(r)["box"] for r in t] == [want] * 5, (Hs, Ws)


def test_draw_is_deterministic_under_seed_and_rank():
    from vtp_amd.augment import MultiCrop
    mk = lambda seed, rank: MultiCrop.dino_default(32, 16, seed=seed, rank=rank).draw(4, 40, 56)
    a, b = mk(3, 0), mk(3, 0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for other in (mk(3, 1), mk(4, 0)):
        assert all(x.tobytes() != y.tobytes() for x, y in zip(a, other))


def test_flag_frequencies():
    from vtp_amd.augment import FLIP, GRAY, JITTER, SOLARIZE, MultiCrop
    B = 20000
    aug = MultiCrop.dino_default(32, 16, n_local=1, seed=5)
    tg, tl = aug.draw(B, 40, 56)

    def close(hits, n, p, what):
        sd = math.sqrt(n * p * (1 - p))
        assert abs(hits - n * p) <= 5 * sd, (what, hits, n * p, sd)

    for name, t, blur_p, sol_p in (("global0", tg[:B], 1.0, 0.0), ("global1", tg[B:], 0.1, 0.2), ("local", tl, 0.5, 0.0)):
        flags = t[:, 4].astype(np.int64)
        close(int((flags & FLIP != 0).sum()), B, 0.5, name + " flip")
        close(int((flags & JITTER != 0).sum()), B, 0.8, name + " jitter")
        close(int((flags & GRAY != 0).sum()), B, 0.2, name + " gray")
        blurred, solarized = int((t[:, 13] > 0).sum()), int((flags & SOLARIZE != 0).sum())
        if blur_p == 1.0:
            assert blurred == B and solarized == 0  # view 0 always blurs and never solarizes
        else:
            close(blurred, B, blur_p, name + " blur")
        if sol_p == 0.0:
            assert solarized == 0
        else:
            close(solarized, B, sol_p, name + " solarize")
        s = t[:, 13][t[:, 13] > 0]
        assert 0.1 <= s.min() and s.max() <= 2.0
        j = t[flags & JITTER != 0]
        assert all(sorted(r) == [0, 1, 2, 3] for r in j[:200, 5:9].tolist())
        assert len({tuple(r) for r in j[:2000, 5:9].tolist()}) == 24                # every order turns up
        assert 0.6 <= j[:, 9].min() and j[:, 9].max() <= 1.4 and 0.6 <= j[:, 10].min() and j[:, 10].max() <= 1.4
        assert 0.8 <= j[:, 11].min() and j[:, 11].max() <= 1.2 and -0.1 <= j[:, 12].min() and j[:, 12].max() <= 0.1
        assert (t[flags & JITTER == 0][:, 5:9] == -1).all()


def test_plain_policy_is_crop_flip_normalise():
    from vtp_amd.augment import FLIP, MultiCrop
    (t,) = MultiCrop.plain(32, scale=(0.5, 1.0), seed=9).draw(500, 40, 56)
    flags = t[:, 4].astype(np.int64)
    assert set(flags.tolist()) == {0, FLIP} and (t[:, 13] == 0).all() and (t[:, 5:9] == -1).all()
    assert (t[:, 2] * t[:, 3] >= 0.5 * 40 * 56 - 100).all()


def test_state_dict_continues_the_stream():
    from vtp_amd.augment import MultiCrop
    a = MultiCrop.dino_default(32, 16, seed=7, rank=2)
    a.draw(3, 40, 56)
    sd = a.state_dict()
    want = a.draw(3, 40, 56)
    b = MultiCrop.dino_default(32, 16, seed=0, rank=0)
    b.load_state_dict(sd)
    got = b.draw(3, 40, 56)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(want, got)) and (b.seed, b.rank) == (7, 2)
    fresh = MultiCrop.dino_default(32, 16, seed=7, rank=2).draw(3, 40, 56)
    assert any(x.tobytes() != y.tobytes() for x, y in zip(want, fresh))  # the second batch is not the first


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_validation_errors_are_raised_before_any_launch():
    from vtp_amd.augment import MultiCrop, ViewPolicy, encode_row
    aug = MultiCrop.plain(16, seed=0)
    u8 = torch.zeros(2, 40, 56, 3, dtype=torch.uint8)
    ok = [np.stack([encode_row((0, 0, 40, 56))] * 2)]
    with pytest.raises(ValueError, match="uint8"):
        aug.apply(u8.float(), ok)
    with pytest.raises(ValueError, match=r"\[B, Hs, Ws, 3\]"):
        aug.apply(u8[0], ok)
    with pytest.raises(ValueError, match=r"\[B, Hs, Ws, 3\]"):
        aug.apply(torch.zeros(2, 3, 40, 56, dtype=torch.uint8), ok)
    with pytest.raises(ValueError, match="Ws % 4"):
        aug(torch.zeros(2, 40, 54, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="at least 5"):
        MultiCrop([ViewPolicy(size=4, views=1, scale=(0.5, 1.0))])
    for box in ((0, 0, 41, 56), (1, 0, 40, 56), (0, 4, 40, 56), (-1, 0, 10, 10), (0, 0, 0, 10)):
        with pytest.raises(ValueError, match="outside"):
            aug.apply(u8, [np.stack([encode_row(box)] * 2)])
    with pytest.raises(ValueError, match="8 times"):
        aug.apply(torch.zeros(1, 132, 56, 3, dtype=torch.uint8), [np.stack([encode_row((0, 0, 129, 56))])])
    with pytest.raises(ValueError, match="float32 array"):
        aug.apply(u8, [ok[0][:1]])
    with pytest.raises(ValueError, match="tables"):
        aug.apply(u8, ok + ok)
    with pytest.raises(ValueError, match="per-view"):
        MultiCrop([ViewPolicy(size=16, views=2, scale=(0.5, 1.0), p_blur=(1.0, 0.1, 0.5))])


def test_no_cpu_path_and_export(monkeypatch, tmp_path):
    import vtp_amd
    from vtp_amd import _lib
    from vtp_amd.augment import MultiCrop
    assert vtp_amd.MultiCrop is MultiCrop
    aug = MultiCrop.plain(16)
    u8 = torch.zeros(2, 40, 56, 3, dtype=torch.uint8)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            aug(u8)
    from vtp_amd import ops
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no fallback"):
        ops.augment_scratch_size(2, 16)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    from vtp_amd import ops
    p = ctypes.c_void_p(64)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    err = lambda: lib.vtp_last_error()
    tiles = lambda S: ((S + 31) // 32) ** 2
    even = lambda n: (n + 1) // 2 * 2
    assert lib.vtp_augment_scratch_floats(6, 16) == 2 * even(6 * tiles(16)) + 6 * 3 * 16 * 16
    assert lib.vtp_augment_scratch_floats(3, 48) == 2 * even(3 * 4) + 3 * 3 * 48 * 48
    assert lib.vtp_augment_scratch_floats(64, 256) == 2 * 64 * 64 + 64 * 3 * 256 * 256
    assert ops.augment_scratch_size(256, 96) == 2 * 256 * 9 + 256 * 3 * 96 * 96
    assert lib.vtp_augment_scratch_floats(1, 4) == -1 and b"S >= 5" in err()
    assert lib.vtp_augment_scratch_floats(0, 16) == -1 and b"N >= 1" in err()
    with pytest.raises(ValueError, match="S >= 5"):
        ops.augment_scratch_size(2, 3)
    need = lib.vtp_augment_scratch_floats(6, 16)
    # src_u8 B Hs Ws table N S mean3 std3 out scratch scratch_len stream
    ok = [p, 3, 40, 56, p, 6, 16, f3, f3, p, p, need, None]
    for i in (0, 4, 7, 8, 9, 10):
        a = list(ok)
        a[i] = None
        assert lib.vtp_augment_crops(*a) == -1 and b"null" in err(), i
    for i, v, msg in ((3, 54, b"Ws % 4"), (6, 4, b"S >= 5"), (5, 0, b"N >= 1"), (5, 7, b"views * B"), (1, 0, b">= 1"), (2, 0, b">= 1"),
                      (11, need - 1, b"scratch too small")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_augment_crops(*a) == -1 and msg in err(), (i, err())
    for i, v in ((0, 66), (4, 72), (9, 68), (10, 72)):
        a = list(ok)
        a[i] = ctypes.c_void_p(v)
        assert lib.vtp_augment_crops(*a) == -1 and b"aligned" in err(), i
    a = list(ok)
    a[8] = (ctypes.c_float * 3)(0.5, 0.0, 0.5)
    assert lib.vtp_augment_crops(*a) == -1 and b"std3" in err()
