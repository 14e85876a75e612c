"""GPU: the reconstruction-evaluation kernels (csrc/recon_eval.hip: vtp_recon_metrics / vtp_recon_finalize) and vtp_amd.ReconEval
against the restated tool (tests/recon_ref.py: SSIM the library's way, PSNR by oracle.tools_oracle), and through the model against
the fixture of the real tool.

Bars.  Byte images and LPIPS inputs: torch.equal with the tool's fp32 expressions on the CPU.  Squared error of a pair that
differs in one pixel: equal to that pixel's (o * 255 - r * 255) ** 2.  PSNR and SSIM per image against the reference in fp64 on the
same fp32 inputs: max(4 dev, 1e-4 dB) and max(4 dev, 1e-5), dev = the deviation of the fp32 torch formulation from fp64 on the
same case, evaluated here on the CPU; the floors are about 1/50 of the digit the tool prints (:.2f dB, :.4f).

Measured on one MI355X (the worst image of each case; dev is the fp32 torch formulation's own deviation from fp64;
profiles/recon_eval.log):
    case      PSNR err   dev       err/bar    SSIM err   dev       err/bar
    16x16     2.7e-6 dB  2.2e-6    0.027      2.6e-8     3.4e-6    0.002
    32x48     1.6e-6     3.0e-7    0.016      2.8e-8     2.3e-6    0.003
    80x48     1.1e-6     8.1e-7    0.011      2.8e-8     1.7e-4    0.000   (dev: the pair of constant images in fp32)
    256x256   1.6e-6     6.2e-7    0.016      1.3e-8     9.0e-7    0.001
    model     3.4e-4 dB against 2 x 1.7e-4 or 5e-3;  SSIM 6.0e-5 against 2 x 4.4e-5"""
import os

import pytest
import torch
from safetensors.torch import load_file

import recon_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, F64 = torch.float32, torch.float64

# B, H, W, index of the identical pair (or None), index of the constant pair (or None)
CASES = {"16x16": (1, 16, 16, None, None), "32x48": (3, 32, 48, 1, None), "80x48": (5, 80, 48, 2, 4), "256x256": (2, 256, 256, None, None)}
CONST_A, CONST_B = 0.3, 0.6


def _inputs(name):
    B, H, W, ident, const = CASES[name]
    x, y = R.smooth_pair(B, H, W, seed=100 + H + W)
    if ident is not None:
        y[ident] = x[ident]
    if const is not None:
        x[const] = R.normalise(torch.full((1, 3, H, W), CONST_A))[0]
        y[const] = R.normalise(torch.full((1, 3, H, W), CONST_B))[0]
    return x, y


def _launch(x, y, lp=True, u8=True):
    """both launches through vtp_amd.ops with every optional output; everything comes back on the CPU"""
    from vtp_amd import ops
    from vtp_amd.recon_eval import ReconEval
    ev = ReconEval(None)
    B, _, H, W = x.shape
    xd, yd = x.to(DEV), y.to(DEV)
    scratch = torch.full((ops.recon_scratch_size(B, H, W),), float("nan"), device=DEV, dtype=F64)
    o = {"ref_u8": torch.zeros(B, H, W, 3, device=DEV, dtype=torch.uint8) if u8 else None,
         "rec_u8": torch.zeros(B, H, W, 3, device=DEV, dtype=torch.uint8) if u8 else None,
         "ref_lp": torch.full((B, 3, H, W), float("nan"), device=DEV) if lp else None,
         "rec_lp": torch.full((B, 3, H, W), float("nan"), device=DEV) if lp else None}
    ops.recon_metrics(xd, yd, ev.sub, ev.div, scratch, o["ref_u8"], o["rec_u8"], o["ref_lp"], o["rec_lp"])
    psnr, ssim = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    sse, acc = torch.empty(B, device=DEV, dtype=F64), torch.zeros(8, device=DEV, dtype=F64)
    ops.recon_finalize(scratch, B, H, W, psnr, ssim, acc, sse)
    torch.cuda.synchronize()
    o.update(psnr=psnr, ssim=ssim, sse=sse, acc=acc, scratch=scratch.view(B, -1, 2))
    return {k: (v.cpu() if v is not None else None) for k, v in o.items()}


@pytest.fixture(scope="module")
def runs():
    """every case once: inputs, kernel outputs, the reference in fp64 and the fp32 torch formulation"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for name in CASES:
        x, y = _inputs(name)
        out[name] = {"x": x, "y": y, "ours": _launch(x, y), "ref64": R.batch(x, y, F64), "ref32": R.batch(x, y, F32)}
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_byte_images_and_lpips_inputs_are_bit_identical(runs, name):
    r = runs[name]
    for src, u8, lp in ((r["x"], "ref_u8", "ref_lp"), (r["y"], "rec_u8", "rec_lp")):
        want_u8, want_lp = R.bytes_and_lpips_inputs(src)
        assert torch.equal(r["ours"][u8], want_u8), (name, u8, int((r["ours"][u8] != want_u8).sum()))
        assert torch.equal(r["ours"][lp], want_lp), (name, lp, int((r["ours"][lp] != want_lp).sum()))
    d = R.denorm(r["x"], F32)
    frac = float(((d == 0) | (d == 1)).float().mean())
    print(f"RECON {name}: clamped fraction of the images {frac:.3f}")
    if CASES[name][4] is None:
        assert 0.01 < frac < 0.15  # the clamp is exercised


@pytest.mark.parametrize("name", list(CASES))
def test_psnr_and_ssim_per_image(runs, name):
    B, H, W, ident, const = CASES[name]
    r = runs[name]
    ours, ref, f32 = r["ours"], r["ref64"], r["ref32"]
    fin = torch.isfinite(ref["psnr"])
    assert fin.tolist() == [i != ident for i in range(B)]
    dev_p = float((f32["psnr"][fin] - ref["psnr"][fin]).abs().max())
    dev_s = float((f32["ssim"] - ref["ssim"]).abs().max())
    bar_p, bar_s = max(4 * dev_p, 1e-4), max(4 * dev_s, 1e-5)
    err_p = float((ours["psnr"].double()[fin] - ref["psnr"][fin]).abs().max())
    err_s = float((ours["ssim"].double() - ref["ssim"]).abs().max())
    print(f"RECON {name}: PSNR {[round(float(v), 2) for v in ref['psnr']]} dB  err={err_p:.2e} dev32={dev_p:.2e} err/bar={err_p / bar_p:.3f}")
    print(f"RECON {name}: SSIM {[round(float(v), 4) for v in ref['ssim']]}  err={err_s:.2e} dev32={dev_s:.2e} err/bar={err_s / bar_s:.3f}")
    lo, hi = float(ref["psnr"][fin].min()), float(ref["psnr"][fin].max())
    assert 2.0 < lo and hi < 60.0  # 12 .. 54 dB of noise, the constant pair below it
    assert err_p <= bar_p, (name, err_p, bar_p)
    assert err_s <= bar_s, (name, err_s, bar_s)
    rel = float(((ours["sse"] - ref["sse"]).abs() / ref["sse"].clamp_min(1e-30))[fin].max())
    assert rel < 1e-5, rel  # fp32 roundings of o * 255 and r * 255 against fp64 ones
    if ident is not None:
        assert float(ours["psnr"][ident]) == float("inf") and float(ours["sse"][ident]) == 0.0
        assert float(ours["ssim"][ident]) == 1.0  # exactly: numerator and denominator are the same numbers at every position
        assert ours["acc"].tolist()[2] == 1.0
    if const is not None:
        a, b = R.denorm(r["x"], F64)[const, :, 0, 0], R.denorm(r["y"], F64)[const, :, 0, 0]
        closed = float(((2 * a * b + R.C1) / (a * a + b * b + R.C1)).mean())  # variances and covariance vanish
        assert abs(float(ours["ssim"][const]) - closed) < 1e-6, (float(ours["ssim"][const]), closed)
    acc = ours["acc"].tolist()
    assert acc[1] == B and acc[5] == 1.0 and acc[6] == 0.0 and acc[7] == 0.0
    assert acc[3] == pytest.approx(float(ref["ssim"].sum()), abs=B * bar_s) and acc[4] == pytest.approx(acc[3] / B, rel=1e-14)
    assert acc[0] == (float("inf") if ident is not None else pytest.approx(float(ref["psnr"].sum()), abs=B * bar_p))


def test_every_pixel_is_counted_exactly_once():
    """pairs that differ in one pixel: the squared error is that pixel's contribution exactly, and one tile -- the owner -- holds
    it.  80 x 48 has 3 x 2 tiles of window positions (70 x 38 of them); rows 70..79 and columns 38..47 lie outside the window grid
    and belong to the last tile row / column."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    H, W = 80, 48
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H - 1, 20), (40, W - 1), (31, 31), (32, 32), (31, 32), (32, 31),
             (63, 31), (64, 32), (69, 37), (70, 38), (75, 45), (79, 33), (5, 40)]
    B = len(spots)
    x, _ = R.smooth_pair(B, H, W, seed=7)
    y = x.clone()
    lo, hi = R.normalise(torch.full((1, 3, 1, 1), 0.4))[0, :, 0, 0], R.normalise(torch.full((1, 3, 1, 1), 0.6))[0, :, 0, 0]
    for b, (py, px) in enumerate(spots):
        c = b % 3
        x[b, c, py, px], y[b, c, py, px] = lo[c], hi[c]
    ours = _launch(x, y, lp=False, u8=False)
    df = R.denorm(x, F32) * 255.0 - R.denorm(y, F32) * 255.0  # fp32, as the tool forms it
    for b, (py, px) in enumerate(spots):
        want = float(df[b, b % 3, py, px].double() ** 2)
        assert int((df[b] != 0).sum()) == 1 and 2000.0 < want < 3000.0  # (0.2 * 255) ** 2 = 2601
        assert float(ours["sse"][b]) == want, (b, py, px, float(ours["sse"][b]), want)
        owner = min(py // 32, 2) * 2 + min(px // 32, 1)
        part = ours["scratch"][b, :, 0]
        assert part.shape == (6,) and float(part[owner]) == want and int((part != 0).sum()) == 1, (b, py, px, part.tolist())
    # a single tile: the halo is larger than the core and the one tile owns all 16 x 16 pixels
    x, _ = R.smooth_pair(4, 16, 16, seed=8)
    y = x.clone()
    for b, (py, px) in enumerate([(0, 0), (0, 15), (15, 0), (15, 15)]):
        x[b, 1, py, px], y[b, 1, py, px] = lo[1], hi[1]
    ours = _launch(x, y, lp=False, u8=False)
    df = R.denorm(x, F32) * 255.0 - R.denorm(y, F32) * 255.0
    assert ours["sse"].tolist() == (df.double() ** 2).flatten(1).sum(1).tolist()


def test_results_repeat_bit_for_bit():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vtp_amd.recon_eval import ReconEval
    x, y = _inputs("80x48")
    xd, yd = x.to(DEV), y.to(DEV)
    got = []
    for _ in range(2):
        ev = ReconEval(None)
        out = ev.update_pair(xd, yd, want_u8=True)
        got.append((out.psnr.cpu(), out.ssim.cpu(), out.sse.cpu(), ev.accumulators()))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert got[0][3][1] == 5 and torch.isinf(got[0][3][0])


@pytest.fixture(scope="module")
def lp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vtp_amd import LPIPS
    m = LPIPS()
    m.reset_parameters(seed=0)
    return m.to(DEV).eval()


def test_accumulation_is_the_tools_aggregation(lp):
    """batches of 4, 4 and 1 images: PSNR over the 9 images, SSIM and LPIPS over the 3 batch means, the per-image means as well --
    and no host synchronisation before results()"""
    from vtp_amd.recon_eval import ReconEval
    H, W = 32, 48
    pairs = [R.smooth_pair(n, H, W, seed=20 + i) for i, n in enumerate((4, 4, 1))]
    dev_pairs = [(x.to(DEV), y.to(DEV)) for x, y in pairs]
    ev = ReconEval(None, lpips=lp)
    ev.update_pair(*dev_pairs[0])  # warm-up: workspaces and the LPIPS weights are prepared once
    ev.update_pair(*dev_pairs[2])
    ev.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [ev.update_pair(xd, yd) for xd, yd in dev_pairs]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res = ev.results()
    refs = [R.batch(x, y, F64) for x, y in pairs]
    direct = []
    for x, y in pairs:
        (_, ref_lp), (_, rec_lp) = R.bytes_and_lpips_inputs(x), R.bytes_and_lpips_inputs(y)
        direct.append(lp(ref_lp.to(DEV), rec_lp.to(DEV)).flatten().cpu())
    for o, d in zip(outs, direct):
        # the same kernels on bit-identical inputs; a tap's workgroups add their shares with float atomics, in any order
        assert torch.allclose(o.lpips.cpu(), d, rtol=1e-5, atol=1e-8), (o.lpips.cpu(), d)
    tool = R.aggregate_tool(refs, direct)
    print(f"RECON accumulate: ours={res}\nRECON accumulate: tool={tool}")
    assert res["num_samples"] == 9 and res["identical_images"] == 0
    assert res["psnr"] == pytest.approx(tool["psnr"], abs=1e-4)
    assert res["ssim"] == pytest.approx(tool["ssim"], abs=1e-5) and res["ssim_per_image"] == pytest.approx(tool["ssim_per_image"], abs=1e-5)
    assert res["lpips"] == pytest.approx(tool["lpips"], rel=1e-5) and res["lpips_per_image"] == pytest.approx(tool["lpips_per_image"], rel=1e-5)
    assert abs(tool["ssim"] - tool["ssim_per_image"]) > 1e-4  # the short batch makes the two rules differ on this data
    ev.reset()
    with pytest.raises(RuntimeError, match="nothing evaluated"):
        ev.results()


def test_model_path_against_the_tools_fixture(golden_sd, lp):
    from oracle import tools_oracle as T
    from oracle.ref_stubs import TINY
    from vtp_amd import VTPConfig, VTPModel
    from vtp_amd.recon_eval import ReconEval
    tg = load_file(os.path.join(ROOT, "tests", "golden", "tools_tiny.safetensors"))
    images = tg["in.images"]
    model = VTPModel(VTPConfig(**TINY))
    model.load_state_dict(golden_sd, strict=True)
    model = model.to(DEV).eval()
    ev = ReconEval(model, lpips=lp)
    out = ev.update(images.to(DEV), want_u8=True)
    # E_ref: the oracle model under bf16 autocast through the restated tool, as tests/test_tools_gpu.py takes it
    _, noisy_rec, noisy_psnr = T.reconstruct_and_psnr(T.OracleModel(golden_sd, 2, 2, 2, autocast_dtype=torch.bfloat16), images)
    ref_psnr = tg["out.rec.psnr"]
    e, e_ref = float((out.psnr.cpu() - ref_psnr).abs().max()), float((torch.tensor(noisy_psnr) - ref_psnr).abs().max())
    print(f"RECON model: PSNR max|err| ours={e:.3e} ref={e_ref:.3e}  values={[round(float(v), 3) for v in out.psnr.cpu()]}")
    assert e <= max(2.0 * e_ref, 5e-3), (e, e_ref)
    o64 = R.denorm(images, F64)
    ref_ssim = R.ssim_library(o64, tg["out.rec.recon_denorm"].double())
    e = float((out.ssim.cpu().double() - ref_ssim).abs().max())
    e_ref = float((R.ssim_library(o64, noisy_rec.double()) - ref_ssim).abs().max())
    print(f"RECON model: SSIM max|err| ours={e:.3e} ref={e_ref:.3e}  values={[round(float(v), 5) for v in out.ssim.cpu()]}")
    assert e <= max(2.0 * e_ref, 5e-5), (e, e_ref)
    # LPIPS is called on the buffers the metric kernel wrote: the same as calling it on the tool's two expressions
    with torch.no_grad():
        recon = model.get_latents_decoded_images(model.get_reconstruction_latents(images.to(DEV))).float()
    (ref_u8, ref_lp), (rec_u8, rec_lp) = R.bytes_and_lpips_inputs(images), R.bytes_and_lpips_inputs(recon)
    direct = lp(ref_lp.to(DEV), rec_lp.to(DEV)).flatten().cpu()
    assert out.lpips.shape == (images.shape[0],) and torch.allclose(out.lpips.cpu(), direct, rtol=1e-4, atol=1e-7), (out.lpips.cpu(), direct)
    assert torch.equal(out.ref_u8.cpu(), ref_u8)
    assert out.rec_u8.shape == rec_u8.shape and float((out.rec_u8.cpu() != rec_u8).float().mean()) < 1e-3  # a second model call
    res = ev.results()
    assert res["num_samples"] == images.shape[0] and res["psnr"] == pytest.approx(float(out.psnr.double().mean()), abs=1e-5)
    assert res["lpips"] == pytest.approx(float(out.lpips.double().mean()), rel=1e-6)


def test_shapes_that_are_refused_and_lpips_sizes(lp):
    from vtp_amd.recon_eval import ReconEval
    x, y = R.smooth_pair(2, 20, 20, seed=5)
    xd, yd = x.to(DEV), y.to(DEV)
    with pytest.raises(ValueError, match="multiple of 16"):
        ReconEval(None, lpips=lp).update_pair(xd, yd)
    ev = ReconEval(None)
    out = ev.update_pair(xd, yd)
    ref = R.batch(x, y, F64)
    assert out.lpips is None and out.ref_u8 is None
    assert float((out.psnr.cpu().double() - ref["psnr"]).abs().max()) < 1e-4
    assert float((out.ssim.cpu().double() - ref["ssim"]).abs().max()) < 1e-5
    assert ev.results()["lpips"] is None
    for shape in ((1, 3, 10, 16), (1, 3, 16, 8), (1, 3, 16, 30)):
        with pytest.raises(ValueError):
            ev.update_pair(torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError, match="CPU tensor"):
        ev.update_pair(x, y)
    with pytest.raises(RuntimeError, match="without a model"):
        ev.update(xd)
