"""The kernels of the LPIPS training path one by one against tests/lpips_ref.py: lpips_unfold3, lpips_fold3_bwd, maxpool2_fwd / _bwd and
lpips_tap (csrc/lpips.hip), the calls of vtp_conv3x3 (csrc/gemm.hip) that tests/test_lpips_gpu.py leaves out, and LPIPS.loss_and_grad
at the smallest legal image and at an oblong one.  tests/test_lpips_ref_host.py shows without a GPU that the bars used here separate
the references from their wrong variants.

Buffers: vtp_conv3x3 reads pixel rows up to W+3 rows before and behind the stack it is given, so every activation operand is a
`_Stack(...).t` view or the view of `stack()`, which carry those zero guard rows.  Outputs are prefilled with the finite sentinel 7.0:
rows a kernel must write as zeros are compared with 0, rows it must not touch with the sentinel.

Every test prints `lpips_kernels: <kernel> <case>: <figure>`: the worst error / bar of the case (profiles/lpips_kernels.log)."""
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = 7.0


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    """two bf16 tensors, bit for bit (the sign of a zero included)"""
    return a.dtype == BF and b.dtype == BF and a.shape == b.shape and torch.equal(bits(a), bits(b))


def ratio(got, ref, bar):
    """worst |got - ref| / bar; an element whose bar is 0 must be met exactly"""
    err = (got.to(F64) - ref.to(F64)).abs()
    bar = torch.as_tensor(bar, dtype=F64, device=err.device).expand_as(err)
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def report(kernel, case, text):
    print(f"lpips_kernels: {kernel} {case}: {text}")


def borders(t, NB, H, W, C):
    """the border rows of a stack view [NB*(H+2)*(W+2), C] as one flat tensor"""
    v = t.view(NB, H + 2, W + 2, C)
    return torch.cat([v[:, 0].flatten(), v[:, -1].flatten(), v[:, 1:-1, 0].flatten(), v[:, 1:-1, -1].flatten()])


def sentinel_stack(NB, C, H, W):
    """an output stack: guard rows zero, every row of the stack 7.0"""
    buf, v = R.stack(torch.zeros(NB, C, H, W, device=DEV))
    v.fill_(SENTINEL)
    return buf, v


def guards_are_zero(buf, rows, W, C):
    g = (W + 3) * C
    return not bool(buf[:g].any()) and not bool(buf[g + rows * C:].any())


# ------------------------------------------------------------------------------------------------------------ unfold / fold
@pytest.mark.parametrize("n,H,W", R.UNFOLD_CASES)
@pytest.mark.parametrize("shift,scale", [(R.SHIFT, R.SCALE), (R.SHIFT_WIDE, R.SCALE_WIDE)], ids=["module", "wide"])
def test_unfold3_bits(n, H, W, shift, scale):
    from vtp_amd import ops
    from vtp_amd.lpips import _Stack
    img_c, tok_c = R.unfold_case(n, H, W)                 # the references are formed on the CPU
    img, tok = img_c.to(DEV), tok_c.to(DEV)
    rows = n * (H + 2) * (W + 2)
    a0 = _Stack(2 * n, H, W, 32, DEV)
    a0.t.fill_(SENTINEL)
    ops.lpips_unfold3(None, img, a0.t, n, H, W, shift, scale)
    want_img = R.unfold3_ref(img_c, H, W, shift, scale).view(rows, 32).to(DEV)
    assert same_bits(a0.t[:rows], want_img)
    assert bool((a0.t[rows:] == SENTINEL).all())          # one launch writes n stacks and no row more
    ops.lpips_unfold3(tok, None, a0.t[rows:], n, H, W, shift, scale)    # the second stack of the same buffer, as forward does
    assert same_bits(a0.t[rows:], R.unfold3_ref(tok_c, H, W, shift, scale).view(rows, 32).to(DEV))
    assert same_bits(a0.t[:rows], want_img)
    assert guards_are_zero(a0.buf, 2 * rows, W, 32)
    report("lpips_unfold3", (n, H, W, scale[0]), "bit-equal (image and token source)")


@pytest.mark.parametrize("n,H,W", R.UNFOLD_CASES)
@pytest.mark.parametrize("scale", [R.SCALE, R.SCALE_WIDE], ids=["module", "wide"])
def test_fold3_bwd(n, H, W, scale):
    from vtp_amd import ops
    from vtp_amd.lpips import _Stack
    dA, dt0 = R.fold_case(n, H, W)
    s = _Stack(n, H, W, 32, DEV)
    s.t.copy_(dA.view(-1, 32))
    dt = dt0.to(DEV).clone()
    ops.lpips_fold3_bwd(s.t, dt, n, H, W, scale)
    ref, sumabs = R.fold3_ref(dA, dt0, H, W, scale)
    r = ratio(dt.cpu(), ref, R.fold_bar(ref, sumabs))
    report("lpips_fold3_bwd", (n, H, W, scale[0]), f"worst error/bar = {r:.3f}")
    assert r <= 1.0, r
    assert same_bits(s.t.cpu(), dA.view(-1, 32))          # the operand is read only


# ------------------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("NB,H,W,C", R.POOL_CASES)
def test_maxpool2_fwd_bwd_bits(NB, H, W, C):
    from vtp_amd import ops
    Y, dP, tap = (t.to(DEV) for t in R.pool_case(NB, H, W, C))
    Ho, Wo = H // 2, W // 2
    _, ys = R.stack(Y)
    pbuf, ps = sentinel_stack(NB, C, Ho, Wo)
    ops.maxpool2_fwd(ys, ps, NB, H, W, C)
    assert torch.equal(R.unstack(ps, NB, Ho, Wo, C), R.maxpool2_fwd_ref(Y))
    assert not bool(borders(ps, NB, Ho, Wo, C).any())     # the forward writes its borders as zeros
    assert guards_are_zero(pbuf, NB * (Ho + 2) * (Wo + 2), Wo, C)
    _, dps = R.stack(dP)
    _, ts = R.stack(tap)
    for name, t, tref in (("no tap", None, None), ("tap", ts, tap)):
        dbuf, dys = sentinel_stack(NB, C, H, W)
        ops.maxpool2_bwd(ys, dps, t, dys, NB, H, W, C)
        want = R.maxpool2_bwd_ref(Y, dP, tref)
        got = dys.view(NB, H + 2, W + 2, C)[:, 1:-1, 1:-1, :]
        assert same_bits(got.contiguous(), want.permute(0, 2, 3, 1).to(BF).contiguous()), name
        assert not bool(got[0, 0:2, 0:2, 8:16].any()), name          # the all-zero window: masked wherever it is routed
        # the backward never writes a border row: the engine relies on zero-initialised workspaces
        assert bool((borders(dys, NB, H, W, C) == SENTINEL).all()), name
        assert guards_are_zero(dbuf, NB * (H + 2) * (W + 2), W, C), name
    report("maxpool2_fwd/_bwd", (NB, H, W, C), "bit-equal (with and without a tap)")


# ------------------------------------------------------------------------------------------------------------ the head of one tap
@pytest.mark.parametrize("C,n,H,W", R.TAP_CASES)
@pytest.mark.parametrize("arrangement", ["one stack", "two stacks"])
def test_lpips_tap(C, n, H, W, arrangement):
    from vtp_amd import ops
    f0, f1, w = R.tap_case(C, n, H, W)
    if arrangement == "one stack":   # the engine's call: the targets' features are the second half of the same stack
        _, ys = R.stack(torch.cat([f0, f1]).to(DEV))
        half = n * (H + 2) * (W + 2)
        s0, s1 = ys[:half], ys[half:]
    else:
        _, s0 = R.stack(f0.to(DEV))
        _, s1 = R.stack(f1.to(DEV))
    wd = w.to(DEV)
    same = R.tap_identical(n, H, W)
    e32 = R.tap_pixel_error_f32(f0, f1, w)          # the reference alone: fp32 torch against float64, worst pixel
    worst_v, worst_d = 0.0, 0.0
    for gs in (None,) + R.GSCALES:
        val = torch.full((n,), R.VAL_PREFILL, dtype=F32, device=DEV)  # the kernel accumulates into val
        if gs is None:
            ops.lpips_tap(s0, s1, wd, val, None, n, H, W, C, 0.0)
        else:
            dbuf, df = sentinel_stack(n, C, H, W)
            ops.lpips_tap(s0, s1, wd, val, df, n, H, W, C, gs)
        ref_v, ref_d = R.tap_ref(f0, f1, w, 1.0 if gs is None else gs, H, W)
        got_v = val.cpu().to(F64) - R.VAL_PREFILL
        assert bool(torch.isfinite(val).all())
        if same is not None:  # f0 == f1: the block sums are 0 and the atomic is skipped
            assert float(val[same]) == R.VAL_PREFILL
        worst_v = max(worst_v, ratio(got_v, ref_v, R.VAL_FACTOR * e32 * ref_v))
        if gs is not None:
            got_d = R.unstack(df, n, H, W, C).cpu()
            assert bool(torch.isfinite(got_d).all())
            assert not bool(got_d[0, :, 0, 0].any())                 # |f0| = 0: the row is exactly 0
            worst_d = max(worst_d, ratio(got_d, ref_d, R.tap_df_bar(ref_d)))
            assert bool((borders(df, n, H, W, C) == SENTINEL).all())  # df0 of a border row is never written
            assert guards_are_zero(dbuf, n * (H + 2) * (W + 2), W, C)
    v_err = worst_v * R.VAL_FACTOR * e32
    report("lpips_tap", (C, n, H, W, arrangement), f"df0 worst error/bar = {worst_d:.3f}   val relative error = {v_err:.2e}, fp32 torch "
           f"alone = {e32:.2e} per pixel, bar = {R.VAL_FACTOR:g} x that: error/bar = {worst_v:.3f}")
    assert worst_d <= 1.0, worst_d
    assert worst_v <= 1.0, (worst_v, v_err, e32)


# ------------------------------------------------------------------------------------------------------------ conv3x3: the missing calls
def _conv_check(name, case, out, ref, NB, H, W, C):
    """interior against the float64 reference under the project's bar; the border rows the kernel writes are zero"""
    r = ratio(R.unstack(out, NB, H, W, C), ref, R.conv_bar(ref))
    report("conv3x3 " + name, case, f"worst error/bar = {r:.3f}")
    assert r <= 1.0, r
    assert not bool(borders(out, NB, H, W, C).any())


def _first_layer(g):
    """conv1_1's operands as LPIPS._prep lays them out: forward [64, 32] = 27 (ky, kx, c) columns + 5 zero columns, and its transpose"""
    w = R.bf_round(torch.randn(64, 27, device=DEV, generator=g) * (2.0 / 27) ** 0.5)
    wf = torch.cat([w, torch.zeros(64, 5, device=DEV)], 1)
    return wf, wf.to(BF).contiguous(), wf.t().to(BF).contiguous()


@pytest.mark.parametrize("NB,H,W", [(2, 16, 16), (3, 16, 48)])
def test_conv_taps1_forward_and_input_grad(NB, H, W):
    """the unfolded first layer: K = 32 is less than one 64-wide k-tile; its input gradient has N = 32, below the narrowest tile"""
    from vtp_amd import ops
    g = torch.Generator(device=DEV).manual_seed(NB * 100 + W)
    x = R.bf_round(torch.randn(NB, 32, H, W, device=DEV, generator=g))     # columns 27..31: finite junk the zero weights must hide
    b = torch.randn(64, device=DEV, generator=g) * 0.1
    wf, wf_bf, wd_bf = _first_layer(g)
    _, xs = R.stack(x)
    ybuf, ys = sentinel_stack(NB, 64, H, W)
    ops.conv3x3(xs, wf_bf, b, ys, NB, H, W, 32, 64, taps=1, mode=0)
    x_live = x.clone()
    x_live[:, 27:] = 0
    _conv_check("taps=1 mode=0", (NB, H, W, 32, 64), ys, R.rows_ref(x_live, wf, b), NB, H, W, 64)
    assert guards_are_zero(ybuf, NB * (H + 2) * (W + 2), W, 64)
    dy = R.bf_round(torch.randn(NB, 64, H, W, device=DEV, generator=g))
    _, dys = R.stack(dy)
    dbuf, dxs = sentinel_stack(NB, 32, H, W)
    ops.conv3x3(dys, wd_bf, None, dxs, NB, H, W, 64, 32, taps=1, mode=1, relu_mask=None)
    _conv_check("taps=1 mode=1 no mask", (NB, H, W, 64, 32), dxs, R.rows_ref(dy, wf.t()), NB, H, W, 32)
    assert not bool(R.unstack(dxs, NB, H, W, 32)[:, 27:].any())           # zero weight rows: exact zeros
    assert guards_are_zero(dbuf, NB * (H + 2) * (W + 2), W, 32)


CONV9 = [  # NB, H, W, Cin, Cout, modes
    (2, 8, 8, 64, 128, ("dgrad no mask",)),          # the input gradient in front of a max-pool: 128 -> 64 channels, no ReLU mask
    (1, 1, 1, 512, 512, ("fwd", "dgrad")),           # last stage of a 16 x 16 image: M = 9, every neighbour of the one pixel is a border
    (3, 2, 2, 512, 512, ("fwd", "dgrad")),           # last stage of a 32 x 32 image
    (1, 16, 24, 64, 64, ("fwd", "dgrad")),           # M = 468: a tail behind one 256-row tile
]


@pytest.mark.parametrize("NB,H,W,Cin,Cout,modes", CONV9)
def test_conv_taps9_small_and_tail(NB, H, W, Cin, Cout, modes):
    """Cin, Cout are those of the forward layer; the input gradient runs Cout -> Cin on the flipped, transposed weights of _prep"""
    from vtp_amd import ops
    g = torch.Generator(device=DEV).manual_seed(NB * 100 + H * 10 + W)
    w = R.bf_round(torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) * (2.0 / (9 * Cin)) ** 0.5)
    rows = NB * (H + 2) * (W + 2)
    if "fwd" in modes:
        x = R.bf_round(torch.randn(NB, Cin, H, W, device=DEV, generator=g))
        b = torch.randn(Cout, device=DEV, generator=g) * 0.1
        _, xs = R.stack(x)
        ybuf, ys = sentinel_stack(NB, Cout, H, W)
        wf = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).to(BF).contiguous()
        ops.conv3x3(xs, wf, b, ys, NB, H, W, Cin, Cout, taps=9, mode=0)
        _conv_check("taps=9 mode=0", (NB, H, W, Cin, Cout), ys, R.conv3x3_fwd_ref(x, w, b), NB, H, W, Cout)
        assert guards_are_zero(ybuf, rows, W, Cout)
    dy = R.bf_round(torch.randn(NB, Cout, H, W, device=DEV, generator=g))
    _, dys = R.stack(dy)
    mask, ms = None, None
    if "dgrad" in modes:
        mask = torch.randn(NB, Cin, H, W, device=DEV, generator=g)
        _, ms = R.stack(mask)
    dbuf, dxs = sentinel_stack(NB, Cin, H, W)
    wd = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout).to(BF).contiguous()
    ops.conv3x3(dys, wd, None, dxs, NB, H, W, Cout, Cin, taps=9, mode=1, relu_mask=ms)
    _conv_check("taps=9 mode=1" + ("" if ms is not None else " no mask"), (NB, H, W, Cout, Cin), dxs,
                R.conv3x3_dgrad_ref(dy, w, None if mask is None else R.bf_round(mask)), NB, H, W, Cin)
    assert guards_are_zero(dbuf, rows, W, Cin)


# ------------------------------------------------------------------------------------------------------------ the composed path
SIZES = [(1, 16, 16), (3, 32, 48)]   # the smallest legal image; an oblong one with three images
WEIGHT = 3.0


def _tokens(x):
    B, _, H, W = x.shape
    return torch.nn.functional.pixel_unshuffle(x, 16).permute(0, 2, 3, 1).reshape(B * (H // 16) * (W // 16), 768)


@pytest.fixture(scope="module")
def composed():
    """one module, four calls: size 0, size 1, size 0, size 1 -- every size is run again after a call at the other one"""
    from oracle import lpips_oracle as L
    from vtp_amd import LPIPS
    sd = L.make_state(11)
    m = LPIPS(use_dropout=True)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    data, runs = [], []
    for i, (B, H, W) in enumerate(SIZES):
        g = torch.Generator().manual_seed(20 + i)
        x1 = torch.rand(B, 3, H, W, generator=g) * 2 - 1
        x0 = (x1 + 0.3 * torch.randn(B, 3, H, W, generator=g)).clamp(-1, 1)
        tok = _tokens(x0).to(BF).contiguous()
        d0 = (1e-5 * torch.randn(tok.shape[0], 768, generator=g)).to(BF)   # stands for the L1 gradient already in dt
        data.append((tok, x1, d0))
    for i in (0, 1, 0, 1):
        (B, H, W), (tok, x1, d0) = SIZES[i], data[i]
        dt = d0.clone().to(DEV)
        val = m.loss_and_grad(tok.to(DEV), x1.to(DEV).contiguous(), dt, WEIGHT, B, H, W).clone()
        torch.cuda.synchronize()
        runs.append((val.cpu(), dt.cpu()))
    return sd, data, runs


@pytest.mark.parametrize("i", [0, 1], ids=["1x16x16", "3x32x48"])
def test_loss_and_grad_vs_float64_oracle(composed, i):
    from oracle import lpips_oracle as L
    sd, data, runs = composed
    (B, H, W), (tok, x1, d0), (val, dt) = SIZES[i], data[i], runs[i]
    x0r = torch.nn.functional.pixel_shuffle(tok.float().view(B, H // 16, W // 16, 768).permute(0, 3, 1, 2), 16)  # the bf16-rounded input
    sd64 = {k: v.to(F64) for k, v in sd.items()}
    xr = x0r.to(F64).requires_grad_(True)
    ref_val = L.lpips(sd64, xr, x1.to(F64))
    (WEIGHT * ref_val.mean()).backward()
    ref_grad = _tokens(xr.grad)
    xb = x0r.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=BF):
        vb = L.lpips(sd, xb, x1)
        (WEIGHT * vb.float().mean()).backward()
    ref_v = ref_val.detach().flatten()
    e_ref_v = float((vb.detach().flatten().to(F64) - ref_v).abs().max())
    e_v = float((val.to(F64) - ref_v).abs().max())
    bar_v = 1.5 * e_ref_v + 2e-3 * float(ref_v.abs().max())
    got = dt.to(F64) - d0.to(F64)
    err = float((got - ref_grad).norm() / ref_grad.norm())
    e_ref = float((_tokens(xb.grad).to(F64) - ref_grad).norm() / ref_grad.norm())
    bar_g = 1.5 * e_ref + 2.0 ** -6
    report("loss_and_grad", SIZES[i], f"value error/bar = {e_v / bar_v:.3f} (bf16 CPU oracle error {e_ref_v:.2e})   gradient norm error/bar = "
           f"{err / bar_g:.3f} (kernel {err:.2e}, bf16 CPU oracle {e_ref:.2e})")
    assert e_v <= bar_v, (e_v, e_ref_v)
    assert err <= bar_g, (err, e_ref)
    assert float(ref_grad.norm()) > 0 and bool((val > 0).all())


@pytest.mark.parametrize("i", [0, 1], ids=["1x16x16", "3x32x48"])
def test_loss_and_grad_again_after_another_size(composed, i):
    """workspaces are not dirtied by a call at another size, and the gradient does not depend on launch order"""
    _, _, runs = composed
    (val_a, dt_a), (val_b, dt_b) = runs[i], runs[i + 2]
    assert same_bits(dt_a, dt_b)
    torch.testing.assert_close(val_b, val_a, rtol=1e-5, atol=0)   # the atomics of the head may land in another order


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_raise_before_any_launch():
    from vtp_amd import ops
    from vtp_amd.lpips import _Stack
    f = _Stack(2, 2, 2, 96, DEV)
    val = torch.zeros(1, dtype=F32, device=DEV)
    w = torch.zeros(96, dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="C must be"):
        ops.lpips_tap(f.t, f.t[16:], w, val, None, 1, 2, 2, 96, 0.0)
    a0 = _Stack(1, 32, 16, 32, DEV)
    img = torch.zeros(1, 3, 32, 16, device=DEV)
    tok = torch.zeros(2, 768, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="exactly one"):
        ops.lpips_unfold3(tok, img, a0.t, 1, 16, 16, R.SHIFT, R.SCALE)
    with pytest.raises(RuntimeError, match="exactly one"):
        ops.lpips_unfold3(None, None, a0.t, 1, 16, 16, R.SHIFT, R.SCALE)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.lpips_unfold3(None, img, a0.t, 1, 24, 16, R.SHIFT, R.SCALE)
    x, y = _Stack(1, 4, 4, 16, DEV), _Stack(1, 2, 2, 16, DEV)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.maxpool2_fwd(x.t, y.t, 1, 3, 4, 16)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.maxpool2_fwd(x.t, y.t, 1, 4, 4, 12)
    xs, ys = _Stack(1, 4, 4, 64, DEV), _Stack(1, 4, 4, 64, DEV)
    wt = torch.zeros(64, 9 * 64, dtype=BF, device=DEV)
    b = torch.zeros(64, dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="Cin must be"):
        ops.conv3x3(xs.t, wt, b, ys.t, 1, 4, 4, 32, 64, taps=9, mode=0)
    with pytest.raises(RuntimeError, match="needs a bias"):
        ops.conv3x3(xs.t, wt, None, ys.t, 1, 4, 4, 64, 64, taps=9, mode=0)
    torch.cuda.synchronize()
    assert not bool(ys.t.any()) and float(val) == 0.0     # nothing ran
