"""GPU checks of LPIPS.enable_fp32_forward (vtp_amd/lpips.py, csrc/lpips_f32.hip) against fp64 evaluations.

Bounds.  gamma_n = n u / (1 - n u), u = 2^-24 (tests/fid_ref.py).  A convolution output is one fmaf chain over K = 9 Cin terms that
starts at the bias: |err| <= gamma_{K+2} (|x| (*) |w| + |b|), the bound of tests/test_fid_gpu.py; the blocked sum the fp32 LPIPS
uses (a chain per 32 k, the block sums added in order) rounds an operand at most 32 + K / 32 + 1 times and is held to the same
bound.  The head and the whole distance
have no a-priori bound worth stating (a division by a norm that may be tiny); they carry the bar of tests/test_fp32_forward_gpu.py,
    E_ours <= max(4 E_32, 2e-6 max|ref64|)   and, end to end,   E_ours <= 0.1 E_bf16,
E_32 = the error of the same expression evaluated by torch in fp32 (on the fixture: of the real reference class's fp32 output),
E_bf16 = the error of this module's own bf16 forward.  The five tap feature maps carry the network bar of tests/test_fid_gpu.py:
max|f - f64| / max|f64| within twice that of the oracle's fp32 runs (CPU and GPU).  Every figure is printed before it is asserted.
Scale / repack and max-pool are bit-equal to torch; a pair's value does not depend on the batch, the chunk or the run."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

import fid_ref as R

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- scale and repack
@pytest.mark.parametrize("cout", [3, 4])
def test_scale_and_repack_are_torchs_bits(cout):
    from oracle import lpips_oracle as L
    from vtp_amd import ops
    dev = _dev()
    sd = L.make_state(0)
    shift, scale = sd["scaling_layer.shift"], sd["scaling_layer.scale"]
    x = 2 * torch.rand(3, 3, 16, 20, generator=torch.Generator().manual_seed(1)) - 1
    x[0, :, 0, 0], x[1, :, 3, 5] = -1.0, 1.0
    x[2, :, 15, 19] = shift.flatten()
    x[2, :, 7, 7] = torch.tensor([1e-30, -0.0, 3e38])
    want = ((x - shift) / scale).permute(0, 2, 3, 1).contiguous()
    y = torch.full((3, 16, 20, cout), -7.25, device=dev)
    ops.lpips_scale_nhwc_f32(x.to(dev), y, shift.flatten().tolist(), scale.flatten().tolist())
    assert torch.equal(_bits(y[..., :3].cpu()), _bits(want))
    assert bool((want[2, 15, 19] == 0).all())
    if cout == 4:
        assert torch.equal(_bits(y[..., 3].cpu()), _bits(torch.zeros(3, 16, 20)))
    on_gpu = ((x.to(dev) - shift.to(dev)) / scale.to(dev)).permute(0, 2, 3, 1)
    print(f"scale Cout={cout}: torch on the device gives the same bits: {torch.equal(_bits(on_gpu), _bits(y[..., :3]))}")


# ---------------------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("shape", [(3, 8, 12, 64), (1, 2, 2, 512)])
def test_maxpool_is_torchs_bits(shape):
    from vtp_amd import ops
    dev = _dev()
    B, H, W, C = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(H))
    x[0, 0:2, 0:2, :C // 2] = x[0, 0:1, 0:1, :C // 2]  # a tie among the four taps
    x[0, 0, 1, C // 2:] = x[0, 1, 0, C // 2:]          # and one between two of them
    x[0, 1, 1, 0] = float("nan")
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
    y = torch.full((B, H // 2, W // 2, C), -7.25, device=dev)
    ops.maxpool2_f32(x.to(dev), y)
    assert torch.equal(_bits(y.cpu()), _bits(want))
    with pytest.raises(ValueError):
        ops.maxpool2_f32(torch.zeros(1, 3, 4, 8, device=dev), torch.zeros(1, 1, 2, 8, device=dev))


# ---------------------------------------------------------------------------------------------------------------- convolution
# (Cin of the data, Cin of the operands, Cout, H, W): VGG16's corners -- the first layer (scalar loads, and zero-padded to 4
# channels), K = 576 on a full 64-pixel tile, K = 4608 on 1 x 1 and 2 x 2 images (every tap but the centre / all but four in the
# padding), 256 -> 512
CONV_CASES = {"3-64_16x20": (3, 3, 64, 16, 20), "3+1-64_16x20": (3, 4, 64, 16, 20), "64-64_8x8": (64, 64, 64, 8, 8),
              "512-512_1x1": (512, 512, 512, 1, 1), "512-512_2x2": (512, 512, 512, 2, 2), "256-512_4x4": (256, 256, 512, 4, 4)}


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    cin, cop, cout, H, W = CONV_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(3, H, W, cin, generator=g)
    w = torch.randn(cout, 3, 3, cin, generator=g) * (9 * cin) ** -0.5
    b = torch.randn(cout, generator=g)
    xd, wd = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    ref = F.relu(F.conv2d(xd, wd, b.double(), 1, 1)).permute(0, 2, 3, 1).contiguous()
    mag = F.conv2d(xd.abs(), wd.abs(), b.double().abs(), 1, 1).permute(0, 2, 3, 1).contiguous()
    if cop > cin:  # the zero channel adds fmaf(0, 0, acc) = acc: the bound stays that of the 9 Cin real terms
        x = torch.cat([x, torch.zeros(3, H, W, cop - cin)], 3)
        w = torch.cat([w, torch.zeros(cout, 3, 3, cop - cin)], 3)
    return x.contiguous(), w.contiguous(), b, ref, R.gamma(9 * cin + 2) * mag


@pytest.mark.parametrize("blocked", [False, True], ids=["chain", "blocked"])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_at_vggs_corners_within_the_chain_bound_and_batch_independent(name, blocked):
    from vtp_amd import ops
    dev = _dev()
    _, _, cout, H, W = CONV_CASES[name]
    x, w, b, ref, bound = _conv_case(name)
    xg, wg, bg = x.to(dev), w.to(dev), b.to(dev)
    y = torch.full((3, H, W, cout), -7.25, device=dev)
    ops.conv2d_f32(xg, wg, bg, y, stride=1, pad=(1, 1), relu=True, blocked=blocked)
    err = (y.double().cpu() - ref).abs()
    print(f"conv {name} blocked={blocked}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    for i in range(3):
        y1 = torch.full((1, H, W, cout), -7.25, device=dev)
        ops.conv2d_f32(xg[i:i + 1].contiguous(), wg, bg, y1, stride=1, pad=(1, 1), relu=True, blocked=blocked)
        assert torch.equal(_bits(y1[0]), _bits(y[i])), f"image {i} differs between a batch of 3 and a batch of 1"


# ---------------------------------------------------------------------------------------------------------------- head
def _head_expr(f, w, n):
    """lpips.py:169-171, 90-94 on NHWC features [2 n, H, W, C] in f's dtype -> [n]"""
    f0, f1 = f[:n], f[n:]
    a = f0 / (torch.sqrt((f0 ** 2).sum(-1, keepdim=True)) + 1e-10)
    b = f1 / (torch.sqrt((f1 ** 2).sum(-1, keepdim=True)) + 1e-10)
    return (((a - b) ** 2) * w).sum(-1).mean((1, 2))


# the issue's cases (C = 64 and 512 at 1 x 1, 4 x 4, 8 x 12) plus the two other channel counts and a map of more than one segment
@pytest.mark.parametrize("C,H,W", [(64, 1, 1), (64, 4, 4), (64, 8, 12), (512, 1, 1), (512, 4, 4), (512, 8, 12), (128, 20, 20),
                                   (256, 4, 4), (64, 16, 17)])
def test_head_against_fp64(C, H, W):
    from vtp_amd import ops
    dev = _dev()
    n = 3
    g = torch.Generator().manual_seed(C + H)
    f = F.relu(torch.randn(2 * n, H, W, C, generator=g))
    f[1, 0, 0], f[n + 1, 0, 0] = 0.0, 0.0  # pair 1: a pixel all zero in both images
    f[2, H - 1, W - 1] = 0.0                # pair 2: a pixel zero in one image only
    w = torch.rand(C, generator=g) * (2.0 / C)
    ref = _head_expr(f.double(), w.double(), n)
    e32 = float((_head_expr(f, w, n).double() - ref).abs().max())
    segs = ops.lpips_head_segments(H * W)
    assert segs == (H * W + 255) // 256
    parts = []
    for _ in range(2):
        part = torch.full((n, segs), float("nan"), dtype=torch.float64, device=dev)
        ops.lpips_head_f32(f.to(dev), w.to(dev), part)
        parts.append(part)
    assert torch.equal(parts[0].view(torch.int64), parts[1].view(torch.int64)), "two runs differ"
    assert bool(torch.isfinite(parts[0]).all())
    ours = parts[0].cpu().sum(1) / (H * W)
    e = float((ours - ref).abs().max())
    print(f"head C={C} {H}x{W}: E_ours {e:.3e}  E_32 {e32:.3e}  floor {2e-6 * float(ref.abs().max()):.3e}")
    assert e <= max(4 * e32, 2e-6 * float(ref.abs().max()))
    if H * W == 1:
        assert float(ours[1]) == 0.0  # 0 / (0 + 1e-10) on both sides: 0, not NaN


# ---------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _golden():
    from oracle import lpips_oracle as L
    g = load_file(os.path.join(os.path.dirname(__file__), "golden", "lpips_tiny.safetensors"))
    sd = L.make_state(int(g["seed"]))
    return g, sd, {k: v.double() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _module(fp32):
    from vtp_amd import LPIPS
    _, sd, _ = _golden()
    m = LPIPS(use_dropout=True)
    m.load_state_dict(sd, strict=True)
    m.to(_dev())
    return m.enable_fp32_forward() if fp32 else m


def _close_pair(B, H, W):
    g = torch.Generator().manual_seed(B * H + W)
    a = 2 * torch.rand(B, 3, H, W, generator=g) - 1
    return a, (a + 0.1 * torch.randn(B, 3, H, W, generator=g)).clamp(-1, 1)


@functools.lru_cache(maxsize=None)
def _e2e_case(name):
    """(x0, x1, ref64, E_32) -- the fp64 oracle once per case"""
    from oracle import lpips_oracle as L
    g, sd, sd64 = _golden()
    if name == "golden":
        x0, x1 = g["x0"], g["x1"]
    else:
        x0, x1 = _close_pair(*name)
    with torch.no_grad():
        ref64 = L.lpips(sd64, x0.double(), x1.double()).flatten()
        fp32 = g["lpips"].flatten() if name == "golden" else L.lpips(sd, x0, x1).flatten()  # golden: the real reference class
    return x0, x1, ref64, float((fp32.double() - ref64).abs().max())


def _check_bar(tag, val, val_bf16, ref64, e32):
    e = float((val.double().cpu().flatten() - ref64).abs().max())
    ebf = float((val_bf16.double().cpu().flatten() - ref64).abs().max())
    floor = 2e-6 * float(ref64.abs().max())
    print(f"lpips fp32 {tag}: value {float(ref64.mean()):.4e}  E_ours {e:.3e}  E_32 {e32:.3e}  floor {floor:.3e}  E_bf16 {ebf:.3e}")
    assert e <= max(4 * e32, floor), f"{tag}: E_ours {e:.3e} > max(4 E_32, floor), E_32 {e32:.3e}, floor {floor:.3e}"
    assert e <= 0.1 * ebf, f"{tag}: E_ours {e:.3e} > 0.1 E_bf16 = {0.1 * ebf:.3e}"


@pytest.mark.parametrize("name", ["golden", (3, 16, 16), (2, 32, 48)], ids=["golden_2x64x64", "3x16x16", "2x32x48"])
def test_end_to_end_against_fp64(name):
    dev = _dev()
    x0, x1, ref64, e32 = _e2e_case(name)
    val = _module(True)(x0.to(dev), x1.to(dev))
    assert val.shape == (x0.shape[0], 1, 1, 1) and val.dtype == torch.float32 and bool(torch.isfinite(val).all())
    _check_bar(str(name), val, _module(False)(x0.to(dev), x1.to(dev)), ref64, e32)


@functools.lru_cache(maxsize=None)
def _tap_case():
    """per tap: (ours NCHW, fp64 oracle, E_cpu, E_gpu) on the fixture's first input"""
    from oracle import lpips_oracle as L
    dev = _dev()
    g, sd, sd64 = _golden()
    x = g["x0"]

    def taps(state, t):
        with torch.no_grad():
            return L.vgg_features(state, (t - state["scaling_layer.shift"]) / state["scaling_layer.scale"])

    f64 = taps(sd64, x.double())
    cpu = taps(sd, x)
    gpu = taps({k: v.to(dev) for k, v in sd.items()}, x.to(dev))
    ours = _module(True).tap_features_fp32(x.to(dev))
    assert len(ours) == 5
    rel = lambda f, r: float((f.double().cpu() - r).abs().max() / r.abs().max())
    return [(ours[k].permute(0, 3, 1, 2), f64[k], rel(cpu[k], f64[k]), rel(gpu[k], f64[k])) for k in range(5)]


@pytest.mark.parametrize("k", range(5))
def test_tap_feature_maps_within_twice_the_oracles_own_fp32_error(k):
    """max|f - f64| / max|f64| of tap k within twice that of the oracle's fp32 runs (the larger of CPU and GPU).

    Measured on one MI355X (E_ours / E_ref): 1.9e-7 / 3.7e-7, 3.2e-7 / 4.4e-7, 5.6e-7 / 8.0e-7, 9.5e-7 / 6.7e-7, 5.9e-7 / 6.1e-7 =
    ratios 0.52, 0.73, 0.70, 1.41, 0.97.  With vtp_conv2d_f32's single chain over K = 576 .. 4608 products the same run gave
    6.5e-7, 1.0e-6, 2.2e-6, 2.5e-6, 1.9e-6 = ratios 1.75, 2.31, 3.1 .. 3.3, 3.3 .. 3.7, 3.0 .. 3.8 and missed the bar at taps
    1 to 4: that is why the module sums in blocks of 32 (vtp_conv2d_f32_blocked)."""
    o, f64, e_cpu, e_gpu = _tap_case()[k]
    assert o.shape == f64.shape
    e, e_ref = float((o.double().cpu() - f64).abs().max() / f64.abs().max()), max(e_cpu, e_gpu)
    print(f"lpips fp32 tap {k} {tuple(o.shape)}: E_ours {e:.3e}  E_ref {e_ref:.3e} (cpu {e_cpu:.3e}, gpu {e_gpu:.3e})  "
          f"ratio {e / e_ref:.2f}")
    assert e <= 2 * e_ref, f"tap {k}: E_ours {e:.3e} > 2 E_ref = {2 * e_ref:.3e}"


# ---------------------------------------------------------------------------------------------------------------- invariance
def test_value_does_not_depend_on_batch_chunk_or_run():
    from vtp_amd.lpips import FP32_CHUNK
    dev = _dev()
    m = _module(True)
    x0, x1 = (t.to(dev) for t in _close_pair(3, 16, 32))
    assert m.fp32_chunk == FP32_CHUNK
    try:
        whole = m(x0, x1)
        assert torch.equal(_bits(m(x0, x1)), _bits(whole)), "two runs differ"
        for i in range(3):
            assert torch.equal(_bits(m(x0[i:i + 1], x1[i:i + 1])), _bits(whole[i:i + 1])), f"pair {i} alone differs from the batch"
        for chunk in (1, 2):
            m.enable_fp32_forward(chunk=chunk)
            assert torch.equal(_bits(m(x0, x1)), _bits(whole)), f"chunk {chunk} differs from the default"
    finally:
        m.enable_fp32_forward(chunk=FP32_CHUNK)
    assert float(whole.min()) > 0
    same = m(x0, x0)
    assert torch.equal(_bits(same), _bits(torch.zeros_like(same))), "forward(x, x) must be exactly 0"


def test_minimum_size_and_refused_sizes():
    dev = _dev()
    m = _module(True)
    x = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    assert bool(torch.isfinite(m(x, -x)).all())
    for H, W in ((24, 16), (16, 40)):
        with pytest.raises(ValueError, match="multiple of 16"):
            m(torch.zeros(1, 3, H, W, device=dev), torch.zeros(1, 3, H, W, device=dev))
    with pytest.raises(ValueError, match="no CPU path"):
        m(x.cpu(), x.cpu())


# ---------------------------------------------------------------------------------------------------------------- nothing else moves
def test_loss_and_grad_and_the_bf16_forward_keep_their_bits():
    """the trainer's entry is the bf16 kernel set whatever the switch says, and switching off restores the bf16 forward"""
    from vtp_amd import LPIPS
    dev = _dev()
    _, sd, _ = _golden()
    m = LPIPS(use_dropout=True)
    m.load_state_dict(sd, strict=True)
    m.to(dev)
    B, H, W = 1, 16, 16
    x0, x1 = (t.to(dev) for t in _close_pair(B, H, W))
    tok = F.pixel_unshuffle(x0, 16).permute(0, 2, 3, 1).reshape(B * (H // 16) * (W // 16), 768).to(torch.bfloat16).contiguous()
    d0 = (1e-5 * torch.randn(tok.shape, generator=torch.Generator().manual_seed(2))).to(torch.bfloat16).to(dev)

    def grad():
        dt = d0.clone()
        val = m.loss_and_grad(tok, x1.contiguous(), dt, 3.0, B, H, W).clone()
        return val, dt

    grad()  # warm-up: the first call allocates the workspace and loads the kernels
    val_off, dt_off = grad()
    fwd_off = m(x0, x1)
    m.enable_fp32_forward()
    val_on, dt_on = grad()
    fwd_on = m(x0, x1)
    m.disable_fp32_forward()
    fwd_back = m(x0, x1)
    assert torch.equal(dt_on.view(torch.int16), dt_off.view(torch.int16))
    # A value of the bf16 kernel set (val of loss_and_grad, forward) is a sum of float atomics, one per workgroup of vtp_lpips_tap,
    # that land in any order: two calls of the same code agree only up to that order (tests/test_recon_eval_gpu.py allows for the
    # same; measured here: equal bits in one run, one ulp apart in the next).  All terms are >= 0, so two orders of n terms differ
    # by at most 2 gamma_n val.  n = the workgroups per image of the five launches (csrc/lpips.hip: min(ceil((H_k + 2) (W_k + 2) /
    # (4 * 512 / C_k)), 96)) = 30 here; the bf16 and the fp32 value lie 700 times further apart.
    adds = sum(min(-(-((H >> k) + 2) * ((W >> k) + 2) // (4 * 512 // c)), 96) for k, c in enumerate((64, 128, 256, 512, 512)))
    assert adds == 30

    def same_up_to_the_order_of_the_atomics(what, a, b):
        diff, bound = float((a.double() - b.double()).abs().max()), 2 * R.gamma(adds) * float(b.double().abs().max())
        print(f"{what}: {a.flatten().tolist()} / {b.flatten().tolist()}, |diff| {diff:.3e}, bound {bound:.3e}, equal bits "
              f"{torch.equal(_bits(a), _bits(b))}")
        return diff <= bound

    assert same_up_to_the_order_of_the_atomics("loss_and_grad val, switch on / off", val_on, val_off)
    assert same_up_to_the_order_of_the_atomics("forward, switched off again / before", fwd_back, fwd_off)
    assert not same_up_to_the_order_of_the_atomics("forward, switch on / off", fwd_on, fwd_off), "the switch did not move forward"


# ---------------------------------------------------------------------------------------------------------------- ReconEval
def test_recon_eval_reports_the_fp32_lpips():
    import recon_ref as RR
    from oracle import lpips_oracle as L
    from vtp_amd.recon_eval import ReconEval
    dev = _dev()
    _, sd, sd64 = _golden()
    images, recon = RR.smooth_pair(2, 32, 32, seed=7)
    (_, ref_lp), (_, rec_lp) = RR.bytes_and_lpips_inputs(images), RR.bytes_and_lpips_inputs(recon)  # the tool's d * 2 - 1
    lp = _module(True)
    ev = ReconEval(None, lpips=lp)
    out = ev.update_pair(images.to(dev), recon.to(dev))
    direct = lp(ref_lp.to(dev), rec_lp.to(dev)).flatten()
    assert torch.equal(_bits(out.lpips), _bits(direct))
    assert ev.results()["lpips"] == pytest.approx(float(direct.double().mean()), rel=1e-6)
    with torch.no_grad():
        ref64 = L.lpips(sd64, ref_lp.double(), rec_lp.double()).flatten()
        e32 = float((L.lpips(sd, ref_lp, rec_lp).flatten().double() - ref64).abs().max())
    _check_bar("ReconEval 2x32x32", out.lpips, _module(False)(ref_lp.to(dev), rec_lp.to(dev)), ref64, e32)
