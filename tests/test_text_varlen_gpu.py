"""Packed captions in the text tower (MI355X): with causal attention and arg-max pooling only the rows up to a caption's EOT are live;
they are stored back to back and their count stays on the device, so every kernel keeps the launch geometry of B * T rows and reads a
device int.  Kernel by kernel: the row limit of the ring GEMM, of the norms and of the GELU backward (live rows bit-equal to the
unlimited launch, rows beyond the limit untouched, operand rows beyond it NaN), the varlen causal attention against the padded launch,
the grouped weight gradients with a device token count; then TextEngine packed against padded, and a captured step replayed with
caption batches of different total length.

Sentinels: every output is prefilled with a finite value and compared BIT FOR BIT where the launch must not write (a NaN sentinel would
hide a read-modify-write); every operand row at or beyond the limit is NaN, so anything that reads one shows up in the output."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import DEV, _sdpa_bf16_errors, bf, check, ops  # noqa: F401  (same helpers / tolerance)
from text_varlen_ref import packed_rows, row_plan

pytestmark = pytest.mark.gpu

SENT = -1024.0  # (exact in bf16)
NAN = float("nan")


@pytest.fixture(autouse=True)
def _restore_tuning():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vtp_amd import _lib
    lib = _lib.load()
    yield
    lib.vtp_set_gemm_tuning(-1, 3)  # process-global


def _force(cfg):
    from vtp_amd import _lib
    _lib.check(_lib.load().vtp_set_gemm_tuning(cfg, 3), "vtp_set_gemm_tuning")


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: not bit-equal ({int((_bits(a) != _bits(b)).sum())} elements differ)"


def _captions(lengths, T, vocab, seed):
    """ids int64 [B, T]: random tokens, EOT = vocab - 1 at position length - 1 (the arg-max), zeros behind it"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab - 1, (len(lengths), T), generator=g)
    for b, n in enumerate(lengths):
        ids[b, n - 1] = vocab - 1
        ids[b, n:] = 0
    return ids


# ------------------------------------------------------------------------------------------------------------ row plan
def test_row_plan_kernel_matches_host():
    o = ops()
    T = 77
    ids = _captions([1, 77, 9, 40, 33], T, 512, 0)
    ids[2, 3] = 511  # a tie in the arg-max: the first maximum (position 3, before the EOT at 8) wins
    ids = torch.cat([ids, torch.zeros(1, T, dtype=torch.int64)])  # an all-zero caption: length 1
    B = ids.shape[0]
    eot, cu, rows = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (B, B + 1, 1))
    o.text_row_plan(ids.to(DEV), eot, cu, rows, B, T)
    h_eot, h_cu, h_rows = row_plan(ids.numpy())
    assert eot.cpu().tolist() == h_eot.tolist() == [0, 76, 3, 39, 32, 0]
    assert cu.cpu().tolist() == h_cu.tolist() and int(rows) == h_rows == 1 + 77 + 4 + 40 + 33 + 1


# ------------------------------------------------------------------------------------------------------------ ring GEMM
M_G, N_G = 300, 192
LIMITS = (1, 127, 128, 129, 300)


@pytest.mark.parametrize("epi", ["bf16", "f32_resid", "gelu", "quick_gelu"])
@pytest.mark.parametrize("cfg", [7, 5])
@pytest.mark.parametrize("K", [128, 3072])
def test_gemm_row_limit(K, cfg, epi):
    """vtp_gemm_nt_limit on forced ring configurations: rows below the limit are bit-equal to the unlimited launch, rows at or above it
    keep the sentinel, and the A / residual rows at or above it are NaN"""
    o = ops()
    M, N = M_G, N_G
    g = torch.Generator(device=DEV).manual_seed(K + cfg)
    a = bf(torch.randn(M, K, device=DEV, generator=g) + torch.linspace(-1, 1, M, device=DEV)[:, None])
    w = bf(torch.randn(N, K, device=DEV, generator=g) * (0.1 if K == 128 else 0.02))
    bias = torch.randn(N, device=DEV, generator=g)
    resid = torch.randn(M, N, device=DEV, generator=g)
    f32 = epi == "f32_resid"
    odt = torch.float32 if f32 else torch.bfloat16

    def run(a_, resid_, m_rows):
        c = torch.full((M, N), SENT, dtype=odt, device=DEV)
        c2 = torch.full((M, N), SENT, dtype=torch.bfloat16, device=DEV) if "gelu" in epi else None
        if epi == "bf16":
            o.gemm_nt(a_, w, c, bias=bias, epi=o.EPI_BF16, m_rows=m_rows)
        elif f32:
            o.gemm_nt(a_, w, c, bias=bias, resid=resid_, epi=o.EPI_F32, m_rows=m_rows)
        else:
            o.gemm_nt(a_, w, c, c2=c2, bias=bias, epi=o.EPI_QUICK_GELU if epi == "quick_gelu" else o.EPI_GELU, m_rows=m_rows)
        return c, c2

    _force(cfg)
    ref, ref2 = run(a, resid, None)
    pre = a.float() @ w.float().T + bias  # the unlimited launch itself is right (tests/test_gemm_ring_gpu.py holds it to the full bar)
    if epi == "bf16":
        check(ref, pre, f"unlimited bf16 K={K} cfg={cfg}")
    elif f32:
        check(ref, pre + resid, f"unlimited f32 K={K} cfg={cfg}", bf16_out=False, scale=1e-5)
    else:
        check(ref2, pre, f"unlimited {epi} pre K={K} cfg={cfg}")
    sent = torch.full((M, N), SENT, dtype=odt, device=DEV)
    sent2 = torch.full((M, N), SENT, dtype=torch.bfloat16, device=DEV)
    for L in LIMITS:
        a_l, r_l = a.clone(), resid.clone()
        a_l[L:] = NAN
        r_l[L:] = NAN
        c, c2 = run(a_l, r_l, _i32(L))
        _same_bits(c[:L], ref[:L], f"{epi} K={K} cfg={cfg} limit={L}: live rows")
        _same_bits(c[L:], sent[L:], f"{epi} K={K} cfg={cfg} limit={L}: rows beyond the limit")
        if c2 is not None:
            _same_bits(c2[:L], ref2[:L], f"{epi} K={K} cfg={cfg} limit={L}: live rows of c2")
            _same_bits(c2[L:], sent2[L:], f"{epi} K={K} cfg={cfg} limit={L}: rows of c2 beyond the limit")
    # a count above the static M changes nothing
    c, _ = run(a, resid, _i32(M + 1000))
    _same_bits(c, ref, f"{epi} K={K} cfg={cfg}: limit above M")


def test_gemm_row_limit_refuses_persistent_kernels_and_keeps_ring_dispatch():
    """a forced 8-phase / half-size / one-wave configuration refuses a row limit; without a forced configuration a shape the dispatch
    gives to the half-size kernel (the text tower's c_proj dgrad, 2464 x 3072 x 768) runs -- on a ring configuration -- and agrees
    with the unlimited launch on that shape to the bf16 bar"""
    o = ops()
    a = bf(torch.randn(256, 512, device=DEV))
    w = bf(torch.randn(256, 512, device=DEV) * 0.05)
    c = torch.empty(256, 256, dtype=torch.bfloat16, device=DEV)
    for cfg in (8, 9, 10):
        _force(cfg)
        with pytest.raises(RuntimeError, match="row limit"):
            o.gemm_nt(a, w, c, epi=o.EPI_BF16, m_rows=_i32(100))
    _force(-1)
    M, N, K, L = 2464, 3072, 768, 1183
    g = torch.Generator(device=DEV).manual_seed(3)
    a = bf(torch.randn(M, K, device=DEV, generator=g))
    w = bf(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    a[L:] = NAN
    c = torch.full((M, N), SENT, dtype=torch.bfloat16, device=DEV)
    o.gemm_nt(a, w, c, epi=o.EPI_BF16, m_rows=_i32(L))
    check(c[:L], a[:L].float() @ w.float().T, "c_proj dgrad shape under a row limit")
    assert bool((c[L:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------ norms, GELU backward
@pytest.mark.parametrize("kind,D", [(1, 128), (1, 768), (0, 384)])
def test_norm_row_limit(kind, D):
    o = ops()
    M = 300
    g = torch.Generator(device=DEV).manual_seed(D + kind)
    x = torch.randn(M, D, device=DEV, generator=g) * 2 + 0.3
    w = torch.rand(D, device=DEV, generator=g) + 0.5
    b = torch.randn(D, device=DEV, generator=g) * 0.1 if kind else None
    dy = bf(torch.randn(M, D, device=DEV, generator=g))
    dres = torch.randn(M, D, device=DEV, generator=g)
    eps = 1e-5
    y_ref = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    st_ref = torch.empty(M, 2, device=DEV)
    o.norm_fwd(x, w, b, y_ref, st_ref, M, D, eps, kind)
    for L in (1, 127, 129, 300):
        x_l, dy_l, dres_l = x.clone(), dy.clone(), dres.clone()
        x_l[L:] = NAN
        dy_l[L:] = NAN
        dres_l[L:] = NAN
        y = torch.full((M, D), SENT, dtype=torch.bfloat16, device=DEV)
        st = torch.full((M, 2), SENT, device=DEV)
        o.norm_fwd(x_l, w, b, y, st, M, D, eps, kind, m_rows=_i32(L))
        _same_bits(y[:L], y_ref[:L], f"norm_fwd kind={kind} D={D} limit={L}: live rows")
        _same_bits(st[:L], st_ref[:L], "norm_fwd stats: live rows")
        assert bool((y[L:] == SENT).all()) and bool((st[L:] == SENT).all()), "norm_fwd wrote beyond the limit"
        # backward: dx / dx bf16 bit-equal to the launch over exactly L rows (the same per-row arithmetic); dw / db / the column sums
        # of the bf16 output against torch on the live rows, at the bar of tests/test_kernels_gpu.py::test_norm_fwd_bwd
        st_l = st_ref.clone()
        st_l[L:] = NAN
        dx_ref, dxb_ref = torch.empty(L, D, device=DEV), torch.empty(L, D, dtype=torch.bfloat16, device=DEV)
        o.norm_bwd(dy, x, w, st_ref, dres, dx_ref, dxb_ref, torch.zeros(D, device=DEV), torch.zeros(D, device=DEV) if kind else None, L, D,
                   kind)
        dx = torch.full((M, D), SENT, device=DEV)
        dxb = torch.full((M, D), SENT, dtype=torch.bfloat16, device=DEV)
        dw = torch.zeros(D, device=DEV)
        db = torch.zeros(D, device=DEV) if kind else None
        dxs = torch.full((D,), 3.0, device=DEV)
        o.norm_bwd(dy_l, x_l, w, st_l, dres_l, dx, dxb, dw, db, M, D, kind, dx_colsum=dxs, m_rows=_i32(L))
        _same_bits(dx[:L], dx_ref, f"norm_bwd kind={kind} D={D} limit={L}: live rows of dx")
        _same_bits(dxb[:L], dxb_ref, "norm_bwd: live rows of dx bf16")
        assert bool((dx[L:] == SENT).all()) and bool((dxb[L:] == SENT).all()), "norm_bwd wrote beyond the limit"
        xr = x[:L].clone().requires_grad_(True)
        wr = w.clone().requires_grad_(True)
        br = b.clone().requires_grad_(True) if kind else None
        ref = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + eps) * wr if kind == 0 else F.layer_norm(xr, (D,), wr, br, eps)
        ref.backward(dy[:L].float())
        check(dw, wr.grad, f"norm_bwd dw limit={L}", bf16_out=False, scale=1e-4)
        if kind:
            check(db, br.grad, f"norm_bwd db limit={L}", bf16_out=False, scale=1e-4)
        cs = dxb_ref.float().sum(0) + 3.0
        assert float((dxs - cs).abs().max()) <= 1e-4 * float(dxb_ref.float().abs().sum(0).max()) + 1e-4, "norm_bwd dx_colsum"


@pytest.mark.parametrize("quick", [False, True])
def test_gelu_bwd_row_limit(quick):
    o = ops()
    M, H = 300, 344
    g = torch.Generator(device=DEV).manual_seed(7)
    dy = bf(torch.randn(M, H, device=DEV, generator=g))
    pre = bf(torch.randn(M, H, device=DEV, generator=g) * 2)
    ref = torch.empty(M, H, dtype=torch.bfloat16, device=DEV)
    o.gelu_bwd(dy, pre, ref, M * H, quick=quick)
    for L in (1, 129, 300):
        dy_l, pre_l = dy.clone(), pre.clone()
        dy_l[L:] = NAN
        pre_l[L:] = NAN
        dx = torch.full((M, H), SENT, dtype=torch.bfloat16, device=DEV)
        o.gelu_bwd(dy_l, pre_l, dx, M * H, quick=quick, m_rows=_i32(L), H=H)
        _same_bits(dx[:L], ref[:L], f"gelu_bwd quick={quick} limit={L}: live rows")
        assert bool((dx[L:] == SENT).all()), "gelu_bwd wrote beyond the limit"


# ------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("lengths", [(1, 32, 33, 64), (65, 77, 9, 40)])
def test_varlen_causal_attention(lengths):
    """packed causal attention against the padded causal launch: forward bit-equal on the live rows; backward (dO = 0 on the dead rows
    of the padded launch's operands) at the bar of tests/test_kernels_gpu.py::test_attention_fwd_bwd -- E_ours <= 1.5 x (relF) / 2 x
    (max|err|) the error of stock bf16 SDPA + autograd against fp32.  Dead rows of the packed buffers are NaN."""
    o = ops()
    B, heads, T = 4, 2, 77
    D = heads * 64
    scale = 0.125
    g = torch.Generator(device=DEV).manual_seed(sum(lengths))
    cu_h = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    total = int(cu_h[-1])
    live = torch.from_numpy(packed_rows(cu_h, T)).to(DEV)  # padded row of every packed row
    cu = torch.from_numpy(cu_h).to(DEV)
    qkv_p = bf(torch.randn(B * T, 3 * D, device=DEV, generator=g))  # padded
    qkv_p[lengths[1] // 2, :64] *= 6  # (a spiked query / key pair, as in the padded test)
    do_p = torch.zeros(B * T, D, dtype=torch.bfloat16, device=DEV)
    do_p[live] = bf(torch.randn(total, D, device=DEV, generator=g))
    # padded causal launch
    out_p = torch.empty(B * T, D, dtype=torch.bfloat16, device=DEV)
    lse_p = torch.empty(B, heads, T, device=DEV)
    o.attn_fwd(qkv_p, qkv_p[:, D:], qkv_p[:, 2 * D:], out_p, lse_p, B, T, heads, T * 3 * D, 3 * D, T * D, D, scale, True)
    # packed buffers: live rows back to back, NaN behind them
    qkv = torch.full((B * T, 3 * D), NAN, dtype=torch.bfloat16, device=DEV)
    qkv[:total] = qkv_p[live]
    d_o = torch.full((B * T, D), NAN, dtype=torch.bfloat16, device=DEV)
    d_o[:total] = do_p[live]
    out = torch.full((B * T, D), SENT, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, heads, T), SENT, device=DEV)
    o.attn_fwd_varlen(qkv, qkv[:, D:], qkv[:, 2 * D:], out, lse, cu, B, T, heads, 3 * D, D, scale)
    _same_bits(out[:total], out_p[live], f"varlen attention forward {lengths}: live rows")
    assert bool((out[total:] == SENT).all()), "varlen attention forward wrote beyond the live rows"
    for b, n in enumerate(lengths):
        _same_bits(lse[b, :, :n], lse_p[b, :, :n], f"lse of caption {b}")
        assert bool((lse[b, :, n:] == SENT).all())
    # backward
    o_in = torch.full((B * T, D), NAN, dtype=torch.bfloat16, device=DEV)
    o_in[:total] = out[:total]
    dqkv = torch.full((B * T, 3 * D), SENT, dtype=torch.bfloat16, device=DEV)
    delta = torch.full((B, heads, T), SENT, device=DEV)
    o.attn_bwd_varlen(qkv, qkv[:, D:], qkv[:, 2 * D:], o_in, d_o, lse, delta, dqkv, dqkv[:, D:], dqkv[:, 2 * D:], cu, B, T, heads, 3 * D, D,
                      scale)
    assert bool((dqkv[total:] == SENT).all()), "varlen attention backward wrote beyond the live rows"
    q, k, v = qkv_p.view(B, T, 3, heads, 64).unbind(2)
    qr, kr, vr = (t.float().detach().requires_grad_(True) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qr.transpose(1, 2), kr.transpose(1, 2), vr.transpose(1, 2), is_causal=True).transpose(1, 2)
    ref.backward(do_p.view(B, T, heads, 64).float())
    e_ref = _sdpa_bf16_errors(q, k, v, do_p.view(B, T, heads, 64), True, (qr.grad, kr.grad, vr.grad))
    full = torch.zeros(B * T, 3 * D, dtype=torch.bfloat16, device=DEV)  # (the dead rows' gradients are exact zeros in the reference)
    full[live] = dqkv[:total]
    dq, dk, dv = full.view(B, T, 3, heads, 64).unbind(2)
    for nm, a, r in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        assert not torch.isnan(a.float()).any(), f"varlen attn_bwd {nm}: NaN"
        d = a.float() - r
        eF, eM = float(d.norm() / r.norm()), float(d.abs().max())
        rF, rM = e_ref[nm]
        print(f"[varlen attn_bwd {nm} {lengths}] relF ours={eF:.3e} ref(bf16 SDPA)={rF:.3e} ratio={eF / rF:.2f} | max|err| ours={eM:.3e} "
              f"ref={rM:.3e} ratio={eM / rM:.2f}")
        assert eF <= 1.5 * rF, f"varlen attn_bwd {nm}: relF {eF:.3e} > 1.5 x E_ref {rF:.3e}"
        assert eM <= 2.0 * rM, f"varlen attn_bwd {nm}: max|err| {eM:.3e} > 2 x E_ref {rM:.3e}"


# ------------------------------------------------------------------------------------------------------------ grouped weight gradients
@pytest.mark.parametrize("live", [70, 1000])
def test_grouped_wgrad_device_token_count(live):
    """ops.WgradGroup(k_rows=...) (vtp_gemm_tn_grouped_limit): the four weight gradients of a block over the first `live` of 1100 static
    token rows, against torch on the live rows at the bar of tests/test_gemm8p_gpu.py::test_grouped_wgrad_matches_torch; the dead rows
    are NaN; two launches on the same scratch accumulate twice"""
    o = ops()
    Ktok, D, H = 1100, 128, 344
    g = torch.Generator(device=DEV).manual_seed(Ktok + live)

    def operand(cols):
        t = bf(torch.randn(Ktok, cols, device=DEV, generator=g))
        t[live:] = NAN
        return t

    dqkv, dmid, dpre, dy = operand(3 * D), operand(D), operand(2 * H), operand(D)
    xn1, att, xn2, hid = operand(D), operand(D), operand(D), operand(H)
    probs = [(dy, hid, D, H, 0, False), (dpre, xn2, 2 * H, D, H, True), (dmid, att, D, D, 0, False), (dqkv, xn1, 3 * D, D, 0, True)]
    gws = [torch.randn(N * K, device=DEV, generator=g) for _, _, N, K, _, _ in probs]
    gbs = [torch.randn(N, device=DEV, generator=g) if cs else None for _, _, N, _, _, cs in probs]
    gw0 = [t.clone() for t in gws]
    gb0 = [None if t is None else t.clone() for t in gbs]
    grp = o.WgradGroup(Ktok, k_rows=_i32(live))
    for (a, x, N, K, sh, _), gw, gb in zip(probs, gws, gbs):
        grp.add(a, x, gw, gb, N, K, sh)
    scratch = {}
    grp.finalize(DEV, scratch)
    assert grp.splits == 1 and grp.kernel == 0 and not scratch, "a device token count runs one K slice on the 8-phase kernel, no scratch"
    grp.launch()
    grp.launch()  # accumulates twice
    torch.cuda.synchronize()
    for (a, x, N, K, sh, cs), gw, gb, w0, b0 in zip(probs, gws, gbs, gw0, gb0):
        ref = a[:live].float().T @ x[:live].float()  # [N, K]
        col = a[:live].float().sum(0)
        if sh:  # de-interleave the GEMM's rows: 16-row groups = 8 rows of w1 | 8 rows of w2
            idx = torch.arange(N, device=DEV)
            dst = ((idx >> 4) << 3) + (idx & 7) + torch.where((idx & 8) != 0, sh, 0)
            r2, c2 = torch.empty_like(ref), torch.empty_like(col)
            r2[dst], c2[dst] = ref, col
            ref, col = r2, c2
        check(gw.view(N, K), w0.view(N, K) + 2 * ref, f"grouped dW N={N} K={K} live={live}", bf16_out=False, scale=1e-4)
        if cs:
            check(gb, b0 + 2 * col, f"grouped db N={N} live={live}", bf16_out=False, scale=1e-4)
    # overwrite mode
    out = torch.full((D * H,), NAN, device=DEV)
    g1 = o.WgradGroup(Ktok, k_rows=_i32(live))
    g1.add(dy, hid, out, None, D, H, 0, accumulate=False)
    g1.finalize(DEV, {}).launch()
    check(out.view(D, H), dy[:live].float().T @ hid[:live].float(), "grouped dW overwrite", bf16_out=False, scale=1e-4)


# ------------------------------------------------------------------------------------------------------------ TextEngine
TXT_CFG = dict(image_size=64, vision_embed_dim=128, vision_depth=1, vision_num_heads=2, text_embed_dim=128, text_depth=2,
               text_num_heads=2, text_vocab_size=512, text_context_length=77, decoder_embed_dim=128, decoder_depth=1,
               decoder_num_heads=2)
LENGTHS_A = (9, 77, 40, 23, 64)  # 213 live rows of 385
LENGTHS_B = (77, 51, 12, 77, 30)  # 247


def relF(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def txt_sd():
    from vtp_amd import VTPConfig, VTPModel
    torch.manual_seed(4)
    m = VTPModel(VTPConfig(**TXT_CFG))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim <= 1 and n != "logit_scale":
                p.add_(0.02 * torch.randn_like(p))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _model(sd):
    from vtp_amd import VTPConfig, VTPModel
    m = VTPModel(VTPConfig(**TXT_CFG))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def test_text_engine_packed_features_bit_equal_to_padded(txt_sd, monkeypatch):
    """per-row arithmetic does not depend on where the row is stored, and the dispatch sees the same static M: the features of the
    packed pass are the padded pass's, bit for bit"""
    ids = _captions(LENGTHS_A, 77, 512, 1).to(DEV)
    m = _model(txt_sd)
    monkeypatch.setenv("VTP_TEXT_VARLEN", "0")
    f_full = m.get_clip_text_feature(ids).clone()
    assert m._text.stack.varlen is None
    monkeypatch.delenv("VTP_TEXT_VARLEN")
    m._text.ws.clear()  # fresh workspaces: nothing the padded pass computed is left in the rows the packed pass does not write
    f_packed = m.get_clip_text_feature(ids).clone()
    assert m._text.stack.varlen is not None, "the packed path was not taken"
    assert int(m._text.stack.varlen[1]) == sum(LENGTHS_A)
    assert torch.isfinite(f_packed).all()
    _same_bits(f_packed, f_full, "text features, packed against padded")


def test_text_engine_packed_gradients_vs_oracle(txt_sd):
    """one rec + clip step on packed captions: every text-tower and head gradient against the oracle's fp32 autograd, with the comparator
    and bar of tests/test_model_gpu.py::test_rec_plus_clip_step_gradients_vs_reference_autograd (E_ours <= 1.5 E_ref, E_ref = the
    oracle's own bf16-autocast backward; and E_ours < 8e-2)"""
    from oracle import vtp_oracle as O
    from vtp_amd import VTPTrainer
    ids = _captions(LENGTHS_A, 77, 512, 1)
    img = torch.randn(len(LENGTHS_A), 3, 64, 64, generator=torch.Generator().manual_seed(2))
    keys = [k for k, v in txt_sd.items() if not k.startswith(("trunk.", "pixel_decoder.")) and v.dtype == torch.float32]
    grads = {}
    for name, ctx in (("f32", torch.autocast("cpu", enabled=False)), ("bf16", torch.autocast("cpu", dtype=torch.bfloat16))):
        sd = {k: v.clone().requires_grad_(v.dtype == torch.float32) for k, v in txt_sd.items()}
        with ctx:
            l1, lc = O.rec_clip_train_loss(sd, img, ids, 2, 2, 2)
            (l1 + lc).backward()
        grads[name] = ({k: sd[k].grad for k in keys}, float(l1.detach()), float(lc.detach()))
    m = _model(txt_sd)
    tr = VTPTrainer(m, lr=0.0, weight_decay=0.0)
    rec, clip = tr.step(img.to(DEV), ids.to(DEV))
    torch.cuda.synchronize()
    assert m._text.stack.varlen is not None, "the packed path was not taken"
    print(f"rec {float(rec):.5f} (oracle {grads['f32'][1]:.5f}) clip {float(clip):.5f} (oracle {grads['f32'][2]:.5f})")
    assert abs(float(rec) - grads["f32"][1]) < 2e-3 * grads["f32"][1]
    assert abs(float(clip) - grads["f32"][2]) < 5e-3 * grads["f32"][2]
    params = dict(m.named_parameters())
    bad = []
    for k in keys:
        ref = grads["f32"][0][k]
        assert torch.isfinite(params[k].grad).all(), k
        e, e_ref = relF(params[k].grad, ref), relF(grads["bf16"][0][k], ref)
        print(f"packed grad {k}: E_ours={e:.3e} E_ref={e_ref:.3e} ratio={e / max(e_ref, 1e-30):.2f}")
        if not (e <= 1.5 * e_ref and e < 8e-2):
            bad.append(k)
    assert not bad, bad


def test_captured_step_replays_caption_batches_of_different_length(txt_sd):
    """one graph-captured rec + clip step, replayed with caption batches of different total length (213 and 247 live rows of 385),
    against the eager step on the same batches; criterion of tests/test_ssl_gpu.py::test_full_step_rec_clip_ssl_graphs_match_eager"""
    from vtp_amd import VTPTrainer
    img = torch.randn(len(LENGTHS_A), 3, 64, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    batches = [_captions(LENGTHS_A, 77, 512, 1).to(DEV), _captions(LENGTHS_B, 77, 512, 2).to(DEV)]
    res = []
    for use_graphs in (False, True):
        m = _model(txt_sd)
        tr = VTPTrainer(m, lr=5e-4, weight_decay=0.0, use_graphs=use_graphs)
        hist, rows = [], []
        for i in range(6):
            r, c = tr.step(img, batches[i & 1])
            hist.append((float(r), float(c)))
            rows.append(int(m._text.stack.varlen[1]))
        assert rows == [sum(LENGTHS_A), sum(LENGTHS_B)] * 3, rows
        res.append((hist, m._engine().flat_p.clone()))
    print("eager:", res[0][0])
    print("graph:", res[1][0])
    for a, b in zip(res[0][0], res[1][0]):
        for x, y in zip(a, b):
            assert abs(x - y) < 1e-2 * abs(x) + 2e-4
    assert torch.isfinite(res[1][1]).all()
    assert relF(res[1][1], res[0][1]) < 1e-3
