"""The row kernels behind the wide trunks (vit_so400m 1152, vit_huge2 1280, vit_giant2 1536) and every width- or length-dependent
branch that the narrower tests never reach: the 8-chunk norm instantiation (D = 1025 .. 2048, one row in flight, the residual gradient
read after the reductions), ragged last chunks, the grid-stride trips of the norm backward at its three block caps, the SwiGLU backward
with fused bias gradients at several column blocks and a second row trip, GELU / QuickGELU backward past the grid cap, the token-row
backward at more than one 1024-column slab, and the small row kernels at D = 1152 / 1536.

Every kernel is called through vtp_amd.ops.  References are plain PyTorch in float64 on the CPU, evaluated on the same f32 / bf16-rounded
inputs the kernel gets; inputs come from seeded CPU generators.  Tolerances are those of tests/test_kernels_gpu.py (`check`, SURVEY.md
§8c: 1e-3 max|ref| + one bf16 ulp for bf16 outputs) with the `scale=` that file uses for the same quantity; copies and rotations are
bit-exact as there.  Outputs are allocated with a guard band behind their last row (a sentinel that must survive): a store past the
row width lands in the next row everywhere else and is caught by the values, behind the last row only by the band."""
import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import DEV, bf, check, interleave, ops  # noqa: F401  (same helpers / tolerance)

pytestmark = pytest.mark.gpu
F64 = torch.float64
GUARD = 64  # elements behind every output


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vtp_amd import _lib
    _lib.load()


def relF(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def guarded(shape, dtype, fill=float("nan")):
    """(view of `shape`, guard band): one allocation, the band directly behind the view's last element"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return flat[:n].view(*shape), flat[n:]


def untouched(band, fill=float("nan")):
    b = band.float().cpu()
    return bool(torch.isnan(b).all()) if fill != fill else bool((b == fill).all())


# ------------------------------------------------------------------------------------------------------------------------------ norms
def _norm_ref64(x, w, b, eps, kind, dy=None):
    """float64 RMSNorm (kind 0) / LayerNorm (kind 1) of the f32 inputs: y, mean, rstd and, given dy, (dx, dw, db)"""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if kind else None
    if kind == 0:
        mean = torch.zeros(x.shape[0], dtype=F64)
        rstd = torch.rsqrt(xr.pow(2).mean(-1) + eps)
        y = xr * rstd[:, None] * wr
    else:
        mean = xr.mean(-1)
        rstd = torch.rsqrt((xr - mean[:, None]).pow(2).mean(-1) + eps)
        y = (xr - mean[:, None]) * rstd[:, None] * wr + br
    grads = None
    if dy is not None:
        y.backward(dy.double())
        grads = (xr.grad, wr.grad, br.grad if kind else None)
    return y.detach(), mean.detach(), rstd.detach(), grads


def _norm_run(x, w, b, dy, dres, eps, kind, full=True):
    """norm_fwd + norm_bwd on the device; full = with dres, dxb, dw, db and dx_colsum (preloaded with 3.0), else with none of them"""
    o = ops()
    M, D = x.shape
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), (b.to(DEV) if kind else None), dy.to(DEV)
    y, y_g = guarded((M, D), torch.bfloat16)
    st, st_g = guarded((M, 2), torch.float32)
    o.norm_fwd(xd, wd, bd, y, st, M, D, eps, kind)
    dx, dx_g = guarded((M, D), torch.float32)
    r = dict(y=y, st=st, dx=dx)
    bands = [y_g, st_g, dx_g]
    if full:
        dxb, dxb_g = guarded((M, D), torch.bfloat16)
        dw, dw_g = guarded((D,), torch.float32, 0.0)
        db, db_g = guarded((D,), torch.float32, 0.0) if kind else (None, None)
        dxs, dxs_g = guarded((D,), torch.float32, 3.0)  # accumulated into: column sums of the bf16 output
        o.norm_bwd(dyd, xd, wd, st, dres.to(DEV), dx, dxb, dw, db, M, D, kind, dx_colsum=dxs)
        r.update(dxb=dxb, dw=dw, db=db, dxs=dxs)
        bands += [dxb_g]
        assert untouched(dw_g, 0.0) and untouched(dxs_g, 3.0) and (not kind or untouched(db_g, 0.0)), "a store behind column D"
    else:
        o.norm_bwd(dyd, xd, wd, st, None, dx, None, None, None, M, D, kind)
    torch.cuda.synchronize()
    assert all(untouched(g) for g in bands), "a store behind the last row"
    return {k: (v.cpu() if v is not None else None) for k, v in r.items()}


def _norm_inputs(M, D, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    w = torch.rand(D, generator=g) + 0.5
    b = torch.randn(D, generator=g) * 0.1 if kind else None
    dy = bf(torch.randn(M, D, generator=g))
    dres = torch.randn(M, D, generator=g)
    return x, w, b, dy, dres


def _norm_check(tag, r, x, w, b, dy, dres, eps, kind, rows=None):
    """the quantities of test_kernels_gpu.test_norm_fwd_bwd at its bars, plus stats = (mean, rstd) at scale 1e-6.  rows: row sets
    whose y / dx are judged each against its own max|ref| (default: all rows at once)"""
    y64, mean64, rstd64, (dx64, dw64, db64) = _norm_ref64(x, w, b, eps, kind, dy)
    dx64 = dx64 + dres.double()
    M = x.shape[0]
    for nm, sel in (rows or {"": torch.arange(M)}).items():
        check(r["y"][sel], y64[sel], f"{tag} norm_fwd{nm}")
        check(r["dx"][sel], dx64[sel], f"{tag} norm_bwd dx{nm}", bf16_out=False, scale=2e-5)
        check(r["dxb"][sel], dx64[sel], f"{tag} norm_bwd dx bf16{nm}")
    check(r["st"][:, 0], mean64, f"{tag} stats mean", bf16_out=False, scale=1e-6)
    check(r["st"][:, 1], rstd64, f"{tag} stats rstd", bf16_out=False, scale=1e-6)
    cs = r["dxb"].double().sum(0) + 3.0
    e = float((r["dxs"].double() - cs).abs().max())
    print(f"[{tag} norm_bwd dx_colsum] max|err|={e:.3e}")
    assert e <= 1e-4 * float(r["dxb"].double().abs().sum(0).max()) + 1e-4, "norm_bwd dx_colsum"
    check(r["dw"], dw64, f"{tag} norm_bwd dw", bf16_out=False, scale=1e-4)
    if kind:
        check(r["db"], db64, f"{tag} norm_bwd db", bf16_out=False, scale=1e-4)


NORM_CASES = [
    # the 8-chunk kernel (one row in flight, dres read after the reductions), ragged (4.5, 5, 6 chunks) and full, at the launcher's
    # limit; 129 blocks against the cap of 128: one second trip
    (1152, 515), (1280, 515), (1536, 515), (2048, 515),
    # an almost empty last chunk (one live lane) for NC = 8, 3, 2, and a single live lane in all for NC = 1
    (1028, 37), (516, 37), (260, 37), (4, 37),
    # two rows in flight, a second trip with an odd row count: the clamped partner row min(row0 + 1, M - 1) inside a later trip
    (768, 1031), (384, 1031),
    # the 256-block cap (three trips) and the 512-block cap (seven trips)
    (128, 4099), (128, 24581),
]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("D,M", NORM_CASES)
def test_norm_fwd_bwd_wide_ragged_and_looping(D, M, kind):
    eps = 1e-5 if kind == 0 else 1e-6
    x, w, b, dy, dres = _norm_inputs(M, D, kind, 1000 * kind + D + M)
    r = _norm_run(x, w, b, dy, dres, eps, kind)
    _norm_check(f"D={D} M={M} kind={kind}", r, x, w, b, dy, dres, eps, kind)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("D", [1536, 516])
def test_norm_hard_rows(D, kind):
    """x = 1000 + 2 randn: a one-pass variance E[x^2] - E[x]^2 in f32 is off by ~0.1 absolute in y, the two-pass form of the kernel is
    not.  Row 5 is constant (7.0): LayerNorm returns the bias exactly, with mean 7 and rstd = rsqrt(eps).  Row 9 is all zero: RMSNorm
    returns exact zeros, and the backward of both kinds stays finite."""
    M = 64
    eps = 1e-5 if kind == 0 else 1e-6
    x, w, b, dy, dres = _norm_inputs(M, D, kind, 77 + D + kind)
    x = 1000.0 + (x - 0.3)
    x[5] = 7.0
    x[9] = 0.0
    r = _norm_run(x, w, b, dy, dres, eps, kind)
    for k, v in r.items():
        assert v is None or torch.isfinite(v.float()).all(), f"{k}: not finite"
    special = torch.tensor([5, 9])
    ordinary = torch.tensor([i for i in range(M) if i not in (5, 9)])
    _norm_check(f"hard D={D} kind={kind}", r, x, w, b, dy, dres, eps, kind, rows={" (1000 + 2 randn rows)": ordinary,
                                                                                " (constant and zero rows)": special})
    if kind:
        assert torch.equal(r["y"][5], bf(b)) and torch.equal(r["y"][9], bf(b)), "LayerNorm of a constant row is the bias, exactly"
        assert float(r["st"][5, 0]) == 7.0 and float(r["st"][9, 0]) == 0.0
        want = float(torch.rsqrt(torch.tensor(eps, dtype=torch.float32)))  # (to one ulp: the accuracy of the device's rsqrt)
        assert abs(float(r["st"][5, 1]) - want) <= 2.0 ** -23 * want and abs(float(r["st"][9, 1]) - want) <= 2.0 ** -23 * want, "rstd = rsqrt(eps)"
    else:
        assert float(r["y"][9].float().abs().max()) == 0.0, "RMSNorm of a zero row is zero, exactly"


@pytest.mark.parametrize("kind", [0, 1])
def test_norm_bwd_without_optional_outputs(kind):
    """dres, dxb, dw, db, dx_colsum all absent at D = 1536 (the reduction passes are skipped): dx equals, bit for bit, that of the
    full call fed a zero residual gradient"""
    D, M = 1536, 515
    eps = 1e-5 if kind == 0 else 1e-6
    x, w, b, dy, _ = _norm_inputs(M, D, kind, 31 + kind)
    bare = _norm_run(x, w, b, dy, None, eps, kind, full=False)
    full = _norm_run(x, w, b, dy, torch.zeros(M, D), eps, kind)
    assert torch.equal(bare["dx"], full["dx"])
    dx64 = _norm_ref64(x, w, b, eps, kind, dy)[3][0]
    check(bare["dx"], dx64, f"norm_bwd bare dx kind={kind}", bf16_out=False, scale=2e-5)


# ---------------------------------------------------------------------------------------------------------------------------- SwiGLU
@pytest.mark.parametrize("M,H", [
    (2741, 2904),  # so400m hidden: 6 column blocks, 43 live lanes in the last; gx = 341 blocks -> rows >= 2 * 1364 = 2728: second trip
    (130, 3416),   # huge2 hidden: 7 column blocks, 43 live lanes in the last
    (130, 4096),   # 8 full column blocks
    (9, 520),      # a second column block with one live lane; 2 row blocks for 9 rows
])
def test_swiglu_bwd_wide(M, H):
    o = ops()
    g = torch.Generator().manual_seed(M + H)
    x1, x2, dh = (bf(torch.randn(M, H, generator=g)) for _ in range(3))
    x12 = interleave(x1.T.contiguous(), x2.T.contiguous()).T.contiguous()
    x12d, dhd = x12.to(DEV), dh.to(DEV)
    fused, fused_g = guarded((M, 2 * H), torch.bfloat16)
    plain, plain_g = guarded((M, 2 * H), torch.bfloat16)
    db12, db12_g = guarded((2 * H,), torch.float32, 2.0)
    o.swiglu_bwd(dhd, x12d, fused, M, H, db12=db12)
    o.swiglu_bwd(dhd, x12d, plain, M, H)
    torch.cuda.synchronize()
    assert untouched(fused_g) and untouched(plain_g), "a store behind the last row of dx12"
    assert untouched(db12_g, 2.0), "a store behind db12"
    assert torch.equal(fused, plain), "the fused-bias kernel's dx12 must equal the plain kernel's"
    fused, db12 = fused.cpu(), db12.cpu()
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    (F.silu(a) * b).backward(dh.double())
    ref = interleave(a.grad.T.contiguous(), b.grad.T.contiguous()).T
    check(fused, ref, f"swiglu_bwd M={M} H={H}", scale=6e-3)
    g_ = torch.arange(2 * H)
    dest = (g_ // 16) * 8 + g_ % 8 + torch.where((g_ % 16) >= 8, H, 0)  # interleaved column -> [b1 | b2] slot
    cs = torch.zeros(2 * H, dtype=F64).index_add_(0, dest, fused.double().sum(0)) + 2.0
    e = float((db12.double() - cs).abs().max())
    print(f"[swiglu_bwd db12 M={M} H={H}] max|err|={e:.3e}")
    assert e <= 1e-4 * float(fused.double().abs().sum(0).max()) + 1e-4, "swiglu_bwd bias grads"


# ------------------------------------------------------------------------------------------------------------------------------ GELU
@pytest.mark.parametrize("quick", [False, True])
@pytest.mark.parametrize("n", [8 * 130 * 43, 8 * (4096 * 256 + 77)])  # the second: 77 element groups past the grid cap of 4096 blocks
def test_gelu_bwd_vs_float64(n, quick):
    o = ops()
    g = torch.Generator().manual_seed(n % 9973 + quick)
    pre, dy = bf(torch.randn(n, generator=g)), bf(torch.randn(n, generator=g))
    dx, dx_g = guarded((n,), torch.bfloat16)
    o.gelu_bwd(dy.to(DEV), pre.to(DEV), dx, n, quick=quick)
    torch.cuda.synchronize()
    assert untouched(dx_g)
    pr = pre.double().requires_grad_(True)
    (pr * torch.sigmoid(1.702 * pr) if quick else F.gelu(pr)).backward(dy.double())
    check(dx.cpu(), pr.grad, f"{'quick_' if quick else ''}gelu_bwd n={n}", scale=2e-3)


# ------------------------------------------------------------------------------------------------------------------ token-row backward
@pytest.mark.parametrize("D", [1152, 1536, 2048])  # two 1024-column slabs (the second ragged, half, full); 36 / 48 / 64 KiB of LDS
def test_token_rows_bwd_wide(D):
    o = ops()
    B, N = 5, 37
    g = torch.Generator().manual_seed(D)
    dx = torch.randn(B * N, D, generator=g)
    masks = (torch.rand(B, N - 1, generator=g) < 0.3).to(torch.uint8)
    masks[torch.arange(B), torch.arange(B) * 7] = 1  # at least one masked row per image
    mb = masks.bool()
    sum_mask = dx.view(B, N, D)[:, 1:][mb].double().sum(0)
    sum_cls = dx.view(B, N, D)[:, 0].double().sum(0)
    dxd, md = dx.to(DEV), masks.to(DEV)
    for which in ("token_rows masks", "token_rows no masks", "mask_rows"):
        use_m, use_c = which != "token_rows no masks", which != "mask_rows"
        dxb, dxb_g = guarded((B * N, D), torch.bfloat16)
        dxb.copy_(bf(dx))
        dm, dm_g = guarded((D,), torch.float32, 1.5)
        dc, dc_g = guarded((D,), torch.float32, 2.0)
        ref = bf(dx).view(B, N, D).clone()
        if use_c:
            ref[:, 0] = 0
        if use_m:
            ref[:, 1:][mb] = 0
        if which == "mask_rows":
            o.mask_rows_bwd(dxd, dxb, md, dm, B, N, D)
        else:
            o.token_rows_bwd(dxd, dxb, md if use_m else None, dm if use_m else None, dc, B, N, D)
        torch.cuda.synchronize()
        assert untouched(dxb_g) and untouched(dm_g, 1.5) and untouched(dc_g, 2.0), f"{which}: a store behind an output"
        assert torch.equal(dxb.cpu().view(B, N, D), ref), f"{which}: dxb"
        em = relF(dm, 1.5 + sum_mask) if use_m else float((dm.cpu() - 1.5).abs().max())
        ec = relF(dc, 2.0 + sum_cls) if use_c else float((dc.cpu() - 2.0).abs().max())
        print(f"[token_rows_bwd D={D} {which}] relF d_mask_token={em:.3e} d_cls_token={ec:.3e}")
        assert (em < 1e-5 if use_m else em == 0.0), f"{which}: d_mask_token"
        assert (ec < 1e-5 if use_c else ec == 0.0), f"{which}: d_cls_token"


# ---------------------------------------------------------------------------------------------------------- small row kernels, wide D
@pytest.mark.parametrize("D", [1152, 1536])
@pytest.mark.parametrize("N", [37, 257])
def test_pool_patch_rows_wide(D, N):
    o = ops()
    B = 3
    x = bf(torch.randn(B * N, D, generator=torch.Generator().manual_seed(D + N)))
    out, out_g = guarded((B, D), torch.float32)
    o.pool_patch_rows(x.to(DEV), out, B, N, D)
    torch.cuda.synchronize()
    assert untouched(out_g)
    ref = x.double().view(B, N, D)[:, 1:].mean(1)
    err = float((out.cpu().double() - ref).abs().max())
    print(f"[pool_patch_rows D={D} N={N}] max|err|={err:.3e} max|ref|={float(ref.abs().max()):.3e}")
    assert err <= 1e-5 * float(ref.abs().max()) + 1e-6


def test_assemble_tokens_and_strided_rowsum_wide():
    o = ops()
    B, N, D = 3, 10, 1152
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B * N, D, generator=g)
    cls, mt = torch.randn(D, generator=g), torch.randn(D, generator=g)
    masks = (torch.rand(B, N - 1, generator=g) < 0.4).to(torch.uint8)
    ref = x.clone().view(B, N, D)
    ref[:, 0] = cls
    ref[:, 1:][masks.bool()] = mt
    xd, xd_g = guarded((B * N, D), torch.float32)
    xd.copy_(x)
    o.assemble_tokens(xd, cls.to(DEV), mt.to(DEV), masks.to(DEV), B, N, D)
    torch.cuda.synchronize()
    assert untouched(xd_g) and torch.equal(xd.cpu().view(B, N, D), ref)
    acc, acc_g = guarded((D,), torch.float32, 1.0)
    o.strided_rowsum(xd, N * D, acc, B, D)
    torch.cuda.synchronize()
    assert untouched(acc_g, 1.0)
    check(acc.cpu(), 1 + ref[:, 0].double().sum(0), "strided_rowsum D=1152", bf16_out=False, scale=1e-6)


@pytest.mark.parametrize("heads", [18, 24])
def test_rope_bit_exact_vs_oracle_wide(heads):
    """forward against oracle.apply_rope, the inverse (the transpose of the rotation) against oracle.apply_rope with the sine negated:
    the table's two halves are equal, so both are the same three bf16 roundings"""
    from oracle import vtp_oracle as O
    o = ops()
    B, h, w = 2, 6, 6
    N, D = h * w + 1, heads * 64
    g = torch.Generator().manual_seed(heads)
    qkv = bf(torch.randn(B * N, 3 * D, generator=g))
    sin, cos = O.rope_table(h, w, O.rope_periods(64))
    q, k, v = qkv.view(B, N, 3, heads, 64).unbind(2)
    for inverse, s in ((False, sin), (True, -sin)):
        qr, kr = O.apply_rope(q.transpose(1, 2), k.transpose(1, 2), s, cos)
        ref = torch.stack([qr.transpose(1, 2), kr.transpose(1, 2), v], dim=2).reshape(B * N, 3 * D)
        dev, dev_g = guarded((B * N, 3 * D), torch.bfloat16)
        dev.copy_(qkv)
        o.rope_qk(dev, sin.to(DEV), cos.to(DEV), B, N, heads, 1, inverse=inverse)
        torch.cuda.synchronize()
        assert untouched(dev_g)
        assert torch.equal(dev.cpu().view(torch.int16), ref.contiguous().view(torch.int16)), f"RoPE inverse={inverse}: not bit-exact"


def test_qk_norm_fwd_bwd_wide():
    """QK normalisation at D = 1152 (18 heads of 64), M = 74.  The op (attention.py:67-68): out = bf16(bf16(x * rstd) * w) per head for
    q and k, v copied; backward in place on dq / dk, dw summed over rows and heads of dy * bf16(x * rstd) (the rounded normalised
    value is what the weight multiplied).  No kernel-level test of it existed; the bars are `check`'s for a bf16 output and those of
    the row norms for rstd (1e-6) and the weight gradient (1e-4)."""
    o = ops()
    M, heads = 74, 18
    D = heads * 64
    eps = 1e-5
    g = torch.Generator().manual_seed(5)
    qkv = bf(torch.randn(M, 3 * D, generator=g) * 1.5)
    wq, wk = torch.rand(64, generator=g) + 0.5, torch.rand(64, generator=g) + 0.5
    dqkv = bf(torch.randn(M, 3 * D, generator=g))
    out, out_g = guarded((M, 3 * D), torch.bfloat16)
    inv, inv_g = guarded((M, 2 * heads), torch.float32)
    qd = qkv.to(DEV)
    o.qk_norm_fwd(qd, wq.to(DEV), wk.to(DEV), out, inv, M, D, eps)
    dd, dd_g = guarded((M, 3 * D), torch.bfloat16)
    dd.copy_(dqkv)
    dwq, dwq_g = guarded((64,), torch.float32, 1.0)
    dwk, dwk_g = guarded((64,), torch.float32, 1.0)
    o.qk_norm_bwd(dd, qd, inv, wq.to(DEV), wk.to(DEV), dwq, dwk, M, D)
    torch.cuda.synchronize()
    assert untouched(out_g) and untouched(inv_g) and untouched(dd_g) and untouched(dwq_g, 1.0) and untouched(dwk_g, 1.0)
    out, inv, dd = out.cpu(), inv.cpu(), dd.cpu()
    x = qkv.double().view(M, 3, heads, 64)[:, :2].clone().requires_grad_(True)  # [M, part, head, 64]
    w2 = torch.stack([wq, wk]).double()[None, :, None, :]
    rstd = torch.rsqrt(x.pow(2).mean(-1) + eps)
    y = x * rstd[..., None] * w2
    dy = dqkv.double().view(M, 3, heads, 64)[:, :2]
    y.backward(dy)
    check(out.view(M, 3, heads, 64)[:, :2], y.detach(), "qk_norm_fwd q, k")
    assert torch.equal(out.view(M, 3, D)[:, 2], qkv.view(M, 3, D)[:, 2]), "v is copied"
    check(inv.view(M, 2, heads), rstd.detach(), "qk_norm_fwd rstd", bf16_out=False, scale=1e-6)
    check(dd.view(M, 3, heads, 64)[:, :2], x.grad, "qk_norm_bwd dq, dk")
    assert torch.equal(dd.view(M, 3, D)[:, 2], dqkv.view(M, 3, D)[:, 2]), "dv is left alone"
    xh = bf(x.detach() * rstd.detach()[..., None]).double()
    dw = 1.0 + (dy * xh).sum((0, 2))
    check(dwq.cpu(), dw[0], "qk_norm_bwd dwq", bf16_out=False, scale=1e-4)
    check(dwk.cpu(), dw[1], "qk_norm_bwd dwk", bf16_out=False, scale=1e-4)


def test_gemm_tn_rows_use_the_engines_splits():
    """the wide weight-gradient rows of test_kernels_gpu.test_gemm_tn_matches_reference name 2 slices: that is the engine's own choice"""
    o = ops()
    assert o.gemm_tn_splits(1152, 2904, 1620) == 2 and o.gemm_tn_splits(3456, 1152, 1620) == 2
    assert o.gemm_splits(1620, 2) == 2
