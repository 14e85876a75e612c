"""CPU-side checks of the reconstruction evaluation (vtp_amd/recon_eval.py, csrc/recon_eval.hip): the reference the GPU tests
compare against (tests/recon_ref.py: SSIM the library's way) against the valid-convolution form and closed forms, the PNG
numbering and files, the aggregation of the accumulator block, the argument checks of the entry points, and what the class does
without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import recon_ref as R

F64 = torch.float64


def _pair(B, H, W, seed):
    x, y = R.smooth_pair(B, H, W, seed)
    return R.denorm(x, F64), R.denorm(y, F64)


@pytest.mark.parametrize("H,W", [(16, 16), (48, 32), (64, 64)])
def test_reference_ssim_is_the_valid_convolution(H, W):
    """reflect pad 5 -> convolution -> crop 5 keeps exactly the window positions whose window lies inside the image: in fp64 the
    two forms differ by exactly 0"""
    p, t = _pair(2, H, W, seed=H + W)
    a, b = R.ssim_library(p, t), R.ssim_valid(p, t)
    assert a.shape == (2,) and float((a - b).abs().max()) == 0.0
    assert 0.0 < float(a.min()) and float(a.max()) < 1.0


def test_reference_ssim_closed_forms():
    p, _ = _pair(2, 32, 48, seed=3)
    assert R.ssim_library(p, p).tolist() == [1.0, 1.0]  # identical images: numerator and denominator are the same numbers
    for a, b in ((0.3, 0.6), (1.0, 0.0), (0.5, 0.5)):
        pa, pb = torch.full((1, 3, 24, 20), a, dtype=F64), torch.full((1, 3, 24, 20), b, dtype=F64)
        want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)  # zero variances and covariance: the luminance term alone
        assert abs(float(R.ssim_library(pa, pb)) - want) < 1e-9, (a, b)
    k = R.gaussian_kernel(F64)
    assert k.shape == (3, 1, 11, 11) and abs(float(k[0].sum()) - 1.0) < 1e-15 and float(k[0, 0, 5, 5]) == float(k.max())


def test_png_index_is_the_tools_expression():
    from vtp_amd.recon_eval import png_index
    batch_size, world, total = 4, 3, 41  # 41 images over 3 ranks in fours: the last batch of a rank is short
    seen = []
    for local_rank in range(world):
        for batch_idx in range(4):
            for i in range(batch_size):
                global_idx = batch_idx * batch_size * world + local_rank * batch_size + i  # :405
                assert png_index(batch_idx, batch_size, world, local_rank, i) == global_idx
                if global_idx < total:
                    seen.append(global_idx)
    assert sorted(seen) == list(range(total))
    assert png_index(2, 32, 1, 0, 5) == 69


def test_save_pngs_round_trips_the_bytes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vtp_amd.recon_eval import ReconBatch, save_pngs
    g = torch.Generator().manual_seed(0)
    ref = torch.randint(0, 256, (3, 12, 16, 3), dtype=torch.uint8, generator=g)
    rec = torch.randint(0, 256, (3, 12, 16, 3), dtype=torch.uint8, generator=g)
    out = ReconBatch(None, None, None, None, ref, rec)
    (tmp_path / "ref").mkdir()
    (tmp_path / "rec").mkdir()
    assert save_pngs(out, str(tmp_path / "ref"), str(tmp_path / "rec"), first_index=8, limit=10) == 2  # index 10 reaches the limit
    assert sorted(p.name for p in (tmp_path / "ref").iterdir()) == ["ref_000008.png", "ref_000009.png"]
    assert sorted(p.name for p in (tmp_path / "rec").iterdir()) == ["rec_000008.png", "rec_000009.png"]
    for i in range(2):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "ref" / f"ref_{8 + i:06d}.png")), ref[i].numpy())
        assert np.array_equal(np.asarray(Image.open(tmp_path / "rec" / f"rec_{8 + i:06d}.png")), rec[i].numpy())
    with pytest.raises(ValueError, match="want_u8"):
        save_pngs(ReconBatch(None, None, None, None, None, None), str(tmp_path), str(tmp_path), 0)


def test_results_arithmetic_from_a_hand_filled_block():
    """three batches of 4, 4 and 1 images: PSNR is averaged over the 9 images, SSIM and LPIPS over the 3 batch means (the short
    batch weighs like a full one), and the per-image means are there as well"""
    from vtp_amd.recon_eval import ACC_SLOTS, aggregate
    psnr = [[30.0, 31.0, 32.0, 33.0], [20.0, 21.0, 22.0, 23.0], [40.0]]
    ssim = [[0.9, 0.8, 0.7, 0.6], [0.5, 0.4, 0.3, 0.2], [1.0]]
    lp = [[0.1, 0.2, 0.3, 0.4], [0.5, 0.6, 0.7, 0.8], [0.0]]
    flat = lambda v: [x for b in v for x in b]
    acc = [sum(flat(psnr)), 9, 0, sum(flat(ssim)), sum(np.mean(b) for b in ssim), 3, sum(np.mean(b) for b in lp), sum(flat(lp))]
    assert len(acc) == ACC_SLOTS
    res = aggregate(acc, True)
    assert res["num_samples"] == 9 and res["identical_images"] == 0
    assert res["psnr"] == pytest.approx(np.mean(flat(psnr)), rel=1e-15)
    assert res["ssim"] == pytest.approx(np.mean([np.mean(b) for b in ssim]), rel=1e-15)
    assert res["lpips"] == pytest.approx(np.mean([np.mean(b) for b in lp]), rel=1e-15)
    assert res["ssim_per_image"] == pytest.approx(np.mean(flat(ssim)), rel=1e-15)
    assert res["lpips_per_image"] == pytest.approx(np.mean(flat(lp)), rel=1e-15)
    assert abs(res["ssim"] - res["ssim_per_image"]) > 0.05  # the two rules differ on this data: (0.75 + 0.35 + 1) / 3 vs 5.4 / 9
    # the same through the reference's aggregation of the tool
    batches = [{"psnr": torch.tensor(p, dtype=F64), "ssim": torch.tensor(s, dtype=F64)} for p, s in zip(psnr, ssim)]
    tool = R.aggregate_tool(batches, [torch.tensor(v) for v in lp])
    for k in ("psnr", "ssim", "lpips", "ssim_per_image", "lpips_per_image"):
        assert res[k] == pytest.approx(tool[k], rel=1e-6), k
    # without an LPIPS the two entries are None; an identical pair makes the PSNR mean inf, as np.mean of the tool's list does
    acc[0], acc[2] = math.inf, 1
    res = aggregate(acc, False)
    assert res["psnr"] == math.inf and res["identical_images"] == 1 and res["lpips"] is None and res["lpips_per_image"] is None
    assert np.mean([30.0, math.inf]) == math.inf
    with pytest.raises(RuntimeError, match="nothing evaluated"):
        aggregate([0.0] * ACC_SLOTS, False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(64)
    f3 = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    err = lambda: lib.vtp_last_error()
    assert lib.vtp_recon_scratch_doubles(2, 16, 16) == 2 * 2 and lib.vtp_recon_scratch_doubles(5, 80, 48) == 2 * 5 * 3 * 2
    assert lib.vtp_recon_scratch_doubles(32, 256, 256) == 2 * 32 * 64
    assert lib.vtp_recon_scratch_doubles(1, 10, 16) == -1 and lib.vtp_recon_scratch_doubles(1, 16, 30) == -1
    # metrics: images recon B H W sub3 div3 ref_u8 rec_u8 ref_lp rec_lp scratch scratch_len
    ok = [p, p, 2, 16, 16, f3, f3, None, None, None, None, p, 4, None]
    for i in (0, 1, 5, 6, 11):
        a = list(ok)
        a[i] = None
        assert lib.vtp_recon_metrics(*a) == -1 and b"null" in err(), i
    for i, v, msg in ((4, 30, b"W % 4"), (3, 10, b">= 11"), (4, 8, b">= 11"), (2, 0, b"B >= 1"), (12, 3, b"scratch too small")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_recon_metrics(*a) == -1 and msg in err(), (i, err())
    a = list(ok)
    a[0] = ctypes.c_void_p(68)
    assert lib.vtp_recon_metrics(*a) == -1 and b"aligned" in err()
    # finalize: scratch scratch_len B H W psnr ssim sse lpips acc
    ok = [p, 4, 2, 16, 16, p, p, None, None, p, None]
    for i in (0, 5, 6, 9):
        a = list(ok)
        a[i] = None
        assert lib.vtp_recon_finalize(*a) == -1 and b"null" in err(), i
    for i, v, msg in ((4, 30, b"W % 4"), (3, 10, b">= 11"), (2, 0, b"B >= 1"), (1, 3, b"scratch too small")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_recon_finalize(*a) == -1 and msg in err(), (i, err())


def test_no_cpu_path_and_export():
    import vtp_amd
    from vtp_amd import ops
    from vtp_amd.recon_eval import ReconEval
    assert vtp_amd.ReconEval is ReconEval
    assert ops.recon_scratch_size(3, 32, 48) == 2 * 3 * 1 * 2
    with pytest.raises(ValueError, match="W % 4"):
        ops.recon_scratch_size(1, 32, 30)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ReconEval(None)
