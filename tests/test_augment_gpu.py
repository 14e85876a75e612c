"""GPU: the SSL-crop kernels (csrc/augment.hip: vtp_augment_crops) and vtp_amd.MultiCrop against the restated chain
(tests/augment_ref.py, fp64 on the CPU).

Exact: a full-image box at S = Hs = Ws, flip off and on, is torch.equal to ops.u8_to_images; every output element is written (the
output is pre-filled with NaN); two runs are bit-identical.

Within tolerance, per case (augment_ref.cases(): each stage alone and the whole chain, S = 5 ... 256 with sizes that are no
multiple of 4 or of the tile, boxes at every corner, up- and down-sampling, ratio 8 on one and on both axes):
max |ours - ref64| <= max(4 dev, 2e-6) in normalised units, dev = the deviation of the helper's own fp32 evaluation from its fp64
one on that case, computed here on the CPU.  The factor 4 is the project's margin (tests/test_recon_eval_gpu.py): it allows
another summation order, such as the separable blur; 2e-6 is 8 ulp of the largest output, 2.64, for cases where the fp32
reference happens to be exact.  In a solarized crop the pixels whose fp64 value before solarize lies within 1e-4 of 128/255 may
fall on either side and are left out: at most 1 % of a case's pixels (asserted).

Measured on one MI355X (profiles/augment.log):
    case               crops  err       dev32     bar       err/bar  left out
    boxes_16             24   1.32e-06  1.92e-06  7.66e-06  0.172    0
    chain_16              6   1.87e-06  2.10e-06  8.39e-06  0.223    0.022 %
    boxes_48             24   1.42e-05  1.44e-05  5.77e-05  0.245    0
    chain_48              6   5.30e-06  5.56e-06  2.23e-05  0.238    0.002 %
    boxes_96             24   1.78e-05  1.74e-05  6.96e-05  0.256    0
    chain_96              6   9.80e-06  1.06e-05  4.24e-05  0.231    0.008 %
    each_op_16           18   2.40e-06  3.35e-06  1.34e-05  0.179    0
    orders_16            72   2.86e-06  3.77e-06  1.51e-05  0.189    0
    gray_16               6   1.01e-06  1.18e-06  4.73e-06  0.212    0
    blur_16               9   1.09e-06  1.86e-06  7.43e-06  0.146    0
    solarize_16           6   1.40e-06  2.09e-06  8.36e-06  0.167    0.022 %
    hue_near_gray_48      6   2.59e-06  2.60e-06  1.04e-05  0.249    0
    constant_48           2   1.46e-06  1.82e-06  7.27e-06  0.201    0
    ratio8_16             2   8.84e-07  1.82e-06  7.28e-06  0.121    0
    odd_10                9   1.76e-06  1.90e-06  7.60e-06  0.232    0
    min_5                 6   5.98e-07  1.87e-06  7.48e-06  0.080    0
    ratio8_33             2   9.91e-07  2.24e-06  8.95e-06  0.111    0
    global_256            2   2.44e-06  2.18e-06  8.71e-06  0.280    0.013 %
    end to end S = 32     8   4.28e-06  4.34e-06  1.74e-05  0.246    0.016 %
    end to end S = 16    32   5.11e-06  5.35e-06  2.14e-05  0.239    0
The boxes_48 / boxes_96 figures are the fp32 tap positions of the up-sampled boxes (a centre near 56 carries 4e-6 of rounding, a
noise image turns that into 1e-5 of a pixel): the fp32 reference has the same error, the kernel forms the taps the same way.
A constant source stays constant to 8.3e-7 through the full chain."""
import numpy as np
import pytest
import torch

import augment_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
NAMES = list(A.cases())


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _launch(u8, S, table):
    """the two launches through vtp_amd.ops; output and scratch pre-filled with NaN; the result on the CPU"""
    from vtp_amd import ops
    N = len(table)
    out = torch.full((N, 3, S, S), float("nan"), device=DEV)
    scratch = torch.full((ops.augment_scratch_size(N, S),), float("nan"), device=DEV)
    ops.augment_crops(u8.to(DEV), torch.from_numpy(np.ascontiguousarray(table)).to(DEV), out, A.MEAN, A.STD, scratch)
    torch.cuda.synchronize()
    return out.cpu()


def _bar_and_error(ours, ref, pre, table, dev):
    keep = A.keep_mask(table, pre)
    left_out = float((~keep).double().mean())
    err = float(((ours.double() - ref).abs() * keep).max())
    return err, max(4 * dev, 2e-6), left_out


@pytest.fixture(scope="module")
def runs():
    """every case once: the kernels' output, the reference in fp64 and the deviation of the fp32 formulation"""
    _need_gpu()
    out = {}
    for name, (u8, S, table) in A.cases().items():
        ref, pre, dev = A.deviation(u8, S, table)
        out[name] = {"ours": _launch(u8, S, table), "ref": ref, "pre": pre, "dev": dev, "table": table}
    return out


def test_full_box_is_the_plain_normalise_bit_for_bit():
    _need_gpu()
    from vtp_amd import ops
    u8 = A.noise(3, 16, 16, 4)
    table = A._views(3, [A.row((0, 0, 16, 16)), A.row((0, 0, 16, 16), flip=True)])
    ours = _launch(u8, 16, table)
    assert torch.isfinite(ours).all()
    for v, flip in enumerate((False, True)):
        want = torch.empty(3, 3, 16, 16, device=DEV)
        ops.u8_to_images(u8.to(DEV), want, A.MEAN, A.STD, flip)
        assert torch.equal(ours[3 * v:3 * v + 3], want.cpu()), flip
    assert torch.equal(ours[:3], A.batch(u8, table[:3], 16, F32)[0])  # and to the helper's fp32 evaluation


@pytest.mark.parametrize("name", NAMES)
def test_case_against_the_reference(runs, name):
    r = runs[name]
    assert torch.isfinite(r["ours"]).all(), "an output element was not written"
    err, bar, left_out = _bar_and_error(r["ours"], r["ref"], r["pre"], r["table"], r["dev"])
    print(f"AUGMENT {name:18s} crops={len(r['table']):3d} err={err:.2e} dev32={r['dev']:.2e} bar={bar:.2e} err/bar={err / bar:.3f} "
          f"left out {100 * left_out:.3f} %")
    assert left_out <= 0.01
    assert err <= bar, (name, err, bar)


def test_constant_source_stays_constant(runs):
    ours = runs["constant_48"]["ours"]
    spread = float((ours.flatten(2).max(2).values - ours.flatten(2).min(2).values).max())
    print(f"AUGMENT constant source: spread over a crop {spread:.2e}")
    assert spread <= 2e-6  # 8 ulp of the largest output


@pytest.mark.parametrize("name", ["chain_96", "global_256"])
def test_results_repeat_bit_for_bit(runs, name):
    u8, S, table = A.cases()[name]
    assert torch.equal(_launch(u8, S, table), runs[name]["ours"])


def test_multicrop_end_to_end():
    _need_gpu()
    from vtp_amd import MultiCrop
    from vtp_amd.data import collate_ssl_batch
    B, Hs, Ws = 4, 40, 56
    aug = MultiCrop.dino_default(global_size=32, local_size=16, seed=3)
    # four solid colours (distinct gray levels too): a crop's colour names the image it was cut from -- the view-major layout
    colours = torch.tensor([[200, 30, 30], [30, 200, 30], [30, 30, 200], [120, 120, 120]], dtype=torch.uint8)
    solid = colours.view(B, 1, 1, 3).expand(B, Hs, Ws, 3).contiguous()
    tables = aug.draw(B, Hs, Ws)
    outs = aug.apply(solid, tables)
    assert [tuple(o.shape) for o in outs] == [(2 * B, 3, 32, 32), (8 * B, 3, 16, 16)] and all(o.is_cuda for o in outs)
    for o, t, S in zip(outs, tables, (32, 16)):
        o = o.cpu().double()
        for n in range(len(t)):
            d = [float((o[n] - A.crop(solid[b], t[n], S, F64)[0]).abs().max()) for b in range(B)]
            assert d[n % B] < 1e-4 and min(v for b, v in enumerate(d) if b != n % B) > 1e-2, (n, d)
    # a noise batch against the helper driven by the same tables; device input, no host synchronisation once warm
    u8 = A.mixed(Hs, Ws, seed=31)
    u8 = torch.cat((u8, A.noise(1, Hs, Ws, 32)))
    tables = aug.draw(B, Hs, Ws)
    aug.apply(u8, tables)  # warm-up: the workspaces exist
    ud = u8.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        g, l = aug.apply(ud, tables)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for o, t, S in zip((g, l), tables, (32, 16)):
        ref, pre, dev = A.deviation(u8, S, t)
        err, bar, left_out = _bar_and_error(o.cpu(), ref, pre, t, dev)
        print(f"AUGMENT end to end S={S}: err={err:.2e} dev32={dev:.2e} err/bar={err / bar:.3f} left out {100 * left_out:.3f} %")
        assert left_out <= 0.01 and err <= bar, (S, err, bar)
    g2, l2 = aug(u8)  # __call__ draws its own tables: the next batch of the stream
    assert g2.shape == g.shape and l2.shape == l.shape and not torch.equal(g2, g)
    ssl = collate_ssl_batch(g.chunk(2), l.chunk(8), patch_size=16)
    assert ssl["n_global_crops"] == 2 and torch.equal(ssl["global_crops"], g) and torch.equal(ssl["local_crops"], l)
    assert ssl["masks"].shape == (2 * B, 4)


def test_shapes_that_are_refused():
    _need_gpu()
    from vtp_amd import MultiCrop
    from vtp_amd.augment import encode_row
    aug = MultiCrop.plain(16)
    u8 = torch.zeros(2, 40, 56, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="outside"):
        aug.apply(u8, [np.stack([encode_row((0, 0, 41, 56))] * 2)])
    with pytest.raises(ValueError, match="Ws % 4"):
        aug(torch.zeros(2, 40, 54, 3, dtype=torch.uint8, device=DEV))
    (out,) = aug(u8)  # black images: every pixel is -mean / std
    want = A.normalise(torch.zeros(3, 16, 16))
    assert torch.equal(out.cpu(), want.expand(2, 3, 16, 16))
