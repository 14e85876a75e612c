"""The kernels of the fp32 inference forward (vtp_amd/csrc/fp32.hip and the fp32 variants of the row kernels) on their own.

Bounds:
  * plain / bias GEMM: element-wise |err| <= gamma (|A| |W^T| + |bias|) against the fp64 product of the same fp32 inputs, gamma =
    (K + 2) u / (1 - (K + 2) u), u = 2^-24 -- the a-priori bound of one fmaf chain of K products plus the bias add (tests/probe_ref.py);
  * activation / residual epilogues: max |err| against the fp64 evaluation of the same expression <= max(4 x the same figure of torch's own
    fp32 evaluation on the CPU, 2 ulp of the largest output);
  * attention: relF and max |err| against the fp64 softmax attention <= max(4 x the same figure of F.scaled_dot_product_attention in fp32 on
    the CPU, 1e-6);
  * RoPE: torch.equal with the oracle's apply_rope; norm: a chain bound over D against fp64, and the bf16 kernel's output is the rounding
    of the fp32 one.
Every test prints its measured figures before it asserts (profiles/README.md quotes them)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def gamma(n):
    return n * U / (1 - n * U)


def ulp_of(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(abs(x), 1e-30))) - 23)


GEMM_SHAPES = [(51, 384, 128), (514, 688, 128), (51, 128, 344), (48, 128, 64), (3, 64, 128), (1, 8, 8)]


def _operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.2
    W2 = torch.randn(N, K, generator=g) * 0.2
    bias, bias2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    gam = torch.rand(N, generator=g) + 0.5
    resid = torch.randn(M, N, generator=g)
    return A, W, W2, bias, bias2, gam, resid


def _run(A, W, **kw):
    from vtp_amd import ops
    M, N = A.shape[0], W.shape[0]
    C = torch.full((M, N), float("nan"), device=DEV)
    dev = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    ops.gemm_nt_f32(A.to(DEV).contiguous(), W.to(DEV).contiguous(), C, **dev)
    torch.cuda.synchronize()
    return C.cpu()


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_plain_and_bias_chain_bound(M, N, K):
    A, W, _, bias, *_ = _operands(M, N, K, 1)
    ref = A.double() @ W.double().T
    mag = A.double().abs() @ W.double().abs().T
    for b in (None, bias):
        C = _run(A, W, bias=b)
        r = ref + (b.double() if b is not None else 0)
        bound = gamma(K + 2) * (mag + (b.double().abs() if b is not None else 0))
        err = (C.double() - r).abs()
        print(f"gemm ({M},{N},{K}) bias={b is not None}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert torch.isfinite(C).all() and bool((err <= bound).all())


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("epi", ["resid", "swiglu", "gelu", "quick_gelu"])
def test_gemm_activation_epilogues(M, N, K, epi):
    from vtp_amd import ops
    A, W, W2, bias, bias2, gam, resid = _operands(M, N, K, 2)

    def expr(dt):
        a, w, w2, b, b2, g, r = (t.to(dt) for t in (A, W, W2, bias, bias2, gam, resid))
        y = F.linear(a, w, b)
        if epi == "resid":
            return r + y * g
        if epi == "swiglu":
            return F.silu(y) * F.linear(a, w2, b2)
        if epi == "gelu":
            return F.gelu(y)
        return y * torch.sigmoid(1.702 * y)

    r64, r32 = expr(torch.float64), expr(torch.float32)
    kw = {"resid": dict(bias=bias, gamma=gam, resid=resid, epi=ops.F32_RESID),
          "swiglu": dict(w2=W2, bias=bias, bias2=bias2, epi=ops.F32_SWIGLU),
          "gelu": dict(bias=bias, epi=ops.F32_GELU), "quick_gelu": dict(bias=bias, epi=ops.F32_QUICK_GELU)}[epi]
    C = _run(A, W, **kw)
    e_ours = float((C.double() - r64).abs().max())
    e_torch = float((r32.double() - r64).abs().max())
    floor = 2 * ulp_of(float(r64.abs().max()))
    print(f"gemm {epi} ({M},{N},{K}): ours {e_ours:.3e} torch-fp32 {e_torch:.3e} ratio {e_ours / max(e_torch, 1e-300):.2f} floor {floor:.3e}")
    assert torch.isfinite(C).all() and e_ours <= max(4 * e_torch, floor)
    if epi == "resid":  # without LayerScale the same chain and one add
        C2 = _run(A, W, bias=bias, resid=resid, epi=ops.F32_RESID)
        r = resid.double() + F.linear(A.double(), W.double(), bias.double())
        assert float((C2.double() - r).abs().max()) <= max(4 * e_torch, floor)


def test_gemm_batch_invariance_repeatability_and_sentinels():
    from vtp_amd import ops
    M, N, K = 51, 384, 128
    A, W, _, bias, *_ = _operands(M, N, K, 3)
    full = _run(A, W, bias=bias)
    assert torch.equal(full, _run(A, W, bias=bias)), "two runs differ"
    head = _run(A[:17], W, bias=bias)
    assert torch.equal(head, full[:17]), "rows 0..16 alone differ from the same rows inside M = 51"
    # sentinels: two guard rows in front and behind, ldc = N + 24
    ldc, S = N + 24, 777.25
    buf = torch.full((M + 4, ldc), S, device=DEV)
    C = buf[2:2 + M]
    ops.gemm_nt_f32(A.to(DEV), W.to(DEV), C, M=M, N=N, K=K, ldc=ldc, bias=bias.to(DEV))
    # strided operands: A and W as column blocks of wider buffers
    Aw, Ww = torch.randn(M, K + 8, device=DEV), torch.randn(N, K + 16, device=DEV)
    Aw[:, :K], Ww[:, :K] = A.to(DEV), W.to(DEV)
    C3 = torch.empty(M, N, device=DEV)
    ops.gemm_nt_f32(Aw, Ww, C3, M=M, N=N, K=K, lda=K + 8, ldw=K + 16, bias=bias.to(DEV))
    torch.cuda.synchronize()
    b = buf.cpu()
    assert torch.equal(b[2:2 + M, :N], full)
    assert bool((b[:2] == S).all()) and bool((b[2 + M:] == S).all()) and bool((b[:, N:] == S).all()), "a sentinel around C was overwritten"
    assert torch.equal(C3.cpu(), full), "leading dimensions change the result"


def test_gemm_rejects_bad_arguments():
    from vtp_amd import ops
    a, w, c = torch.zeros(4, 12, device=DEV), torch.zeros(8, 12, device=DEV), torch.zeros(4, 8, device=DEV)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.gemm_nt_f32(a, w, c)
    with pytest.raises(ValueError, match="float32"):
        ops.gemm_nt_f32(a.bfloat16(), w, c)


# ---------------------------------------------------------------------------------------------------------------- attention
ATTN_SHAPES = [(3, 2, 17, False), (2, 2, 257, False), (2, 2, 256, False), (1, 1, 1, False), (1, 2, 1025, False), (3, 2, 16, True),
               (2, 2, 77, True)]
SCALE = 0.125


def _attn_ours(qkv, B, N, heads, causal):
    from vtp_amd import ops
    D = heads * 64
    q = qkv.to(DEV).contiguous()
    o = torch.full((B * N, D), float("nan"), device=DEV)
    ops.attn_fwd_f32(q, q[:, D:], q[:, 2 * D:], o, B, N, heads, N * 3 * D, 3 * D, N * D, D, SCALE, causal)
    torch.cuda.synchronize()
    return o.cpu()


def _split(qkv, B, N, heads):
    return [t.transpose(1, 2) for t in qkv.view(B, N, 3, heads, 64).unbind(2)]  # [B, heads, N, 64]


def _attn_ref64(qkv, B, N, heads, causal):
    q, k, v = _split(qkv.double(), B, N, heads)
    s = q @ k.transpose(-1, -2) * SCALE
    if causal:
        s = s.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), float("-inf"))
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B * N, heads * 64)


def _attn_bars(qkv, B, N, heads, causal, ours):
    ref = _attn_ref64(qkv, B, N, heads, causal)
    q, k, v = _split(qkv, B, N, heads)
    sd = F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=SCALE).transpose(1, 2).reshape(B * N, heads * 64).double()
    rel = lambda a: float((a - ref).norm() / ref.norm())
    mx = lambda a: float((a - ref).abs().max())
    return (rel(ours.double()), mx(ours.double())), (rel(sd), mx(sd))


@pytest.mark.parametrize("B,heads,N,causal", ATTN_SHAPES)
def test_attention_against_fp64(B, heads, N, causal):
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B * N, 3 * heads * 64, generator=g)
    ours = _attn_ours(qkv, B, N, heads, causal)
    (r_o, m_o), (r_t, m_t) = _attn_bars(qkv, B, N, heads, causal, ours)
    print(f"attn B={B} h={heads} N={N} causal={causal}: relF ours {r_o:.3e} sdpa {r_t:.3e} (x{r_o / max(r_t, 1e-300):.2f}); "
          f"max ours {m_o:.3e} sdpa {m_t:.3e} (x{m_o / max(m_t, 1e-300):.2f})")
    assert torch.isfinite(ours).all()
    assert r_o <= max(4 * r_t, 1e-6) and m_o <= max(4 * m_t, 1e-6)


def test_attention_batch_invariance_repeatability_and_large_logits():
    B, heads, N = 3, 2, 77
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * N, 3 * heads * 64, generator=g)
    qkv[N + 9, :heads * 64] *= 40.0  # one query row of image 1 with large logits
    for causal in (False, True):
        full = _attn_ours(qkv, B, N, heads, causal)
        assert torch.equal(full, _attn_ours(qkv, B, N, heads, causal)), "two runs differ"
        for b in range(B):
            alone = _attn_ours(qkv[b * N:(b + 1) * N], 1, N, heads, causal)
            assert torch.equal(alone, full[b * N:(b + 1) * N]), f"image {b} alone differs from the same image in its batch"
        (r_o, m_o), (r_t, m_t) = _attn_bars(qkv, B, N, heads, causal, full)
        print(f"attn large logits causal={causal}: relF ours {r_o:.3e} sdpa {r_t:.3e}; max ours {m_o:.3e} sdpa {m_t:.3e}")
        assert torch.isfinite(full).all() and r_o <= max(4 * r_t, 1e-6) and m_o <= max(4 * m_t, 1e-6)


def test_attention_leaves_the_rows_around_o_alone():
    from vtp_amd import ops
    B, heads, N, D = 2, 2, 17, 128
    qkv = torch.randn(B * N, 3 * D, device=DEV)
    buf = torch.full((B * N + 2, D), 5.5, device=DEV)
    ops.attn_fwd_f32(qkv, qkv[:, D:], qkv[:, 2 * D:], buf[1:1 + B * N], B, N, heads, N * 3 * D, 3 * D, N * D, D, SCALE, False)
    torch.cuda.synchronize()
    assert bool((buf[0] == 5.5).all()) and bool((buf[-1] == 5.5).all()) and torch.isfinite(buf).all()


# ---------------------------------------------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("B,h,w,prefix", [(2, 4, 4, 1), (3, 3, 5, 0)])
def test_rope_f32_equals_the_oracle(B, h, w, prefix):
    from oracle import vtp_oracle as O
    from vtp_amd import ops
    heads, N = 2, h * w + prefix
    D = heads * 64
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B * N, 3 * D, generator=g) * 3
    sin, cos = O.rope_table(h, w, O.rope_periods())
    q, k, v = _split(qkv, B, N, heads)
    q_ref, k_ref = O.apply_rope(q, k, sin, cos)
    dev = qkv.to(DEV).contiguous()
    ops.rope_qk_f32(dev, sin.to(DEV).contiguous(), cos.to(DEV).contiguous(), B, N, heads, prefix)
    torch.cuda.synchronize()
    q_o, k_o, v_o = _split(dev.cpu(), B, N, heads)
    assert q_ref.dtype == torch.float32
    assert torch.equal(q_o, q_ref) and torch.equal(k_o, k_ref) and torch.equal(v_o, v)


@pytest.mark.parametrize("kind,M,D", [(0, 51, 128), (1, 51, 128), (0, 7, 344), (1, 5, 768)])
def test_norm_f32_output(kind, M, D):
    from vtp_amd import ops
    g = torch.Generator().manual_seed(D + kind)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    w, b = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    eps = 1e-5 if kind == 0 else 1e-6
    xd, wd, bd = x.double(), w.double(), b.double()
    if kind == 0:
        rstd = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
        cen, ref = xd, xd * rstd * wd
    else:
        cen = xd - xd.mean(-1, keepdim=True)
        rstd = torch.rsqrt(cen.pow(2).mean(-1, keepdim=True) + eps)
        ref = cen * rstd * wd + bd
    xg, wg, bg = x.to(DEV), w.to(DEV), (b.to(DEV) if kind == 1 else None)
    y32, st = torch.empty(M, D, device=DEV), torch.empty(M, 2, device=DEV)
    y16 = torch.empty(M, D, device=DEV, dtype=torch.bfloat16)
    ops.norm_fwd_f32(xg, wg, bg, y32, st, M, D, eps, kind)
    ops.norm_fwd(xg, wg, bg, y16, st, M, D, eps, kind)
    torch.cuda.synchronize()
    # mean and sum of squares are sums of D terms (relative error <= gamma(D) of their absolute sums), rsqrt / the products / the bias
    # add a few roundings more: gamma(D + 8) on the row's magnitudes, plus one ulp of the result
    bound = gamma(D + 8) * (cen.abs() + xd.abs().mean(-1, keepdim=True)) * rstd * wd.abs() + 2 * U * ref.abs()
    err = (y32.cpu().double() - ref).abs()
    print(f"norm kind={kind} D={D}: max err / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    assert torch.equal(y16.cpu(), y32.cpu().to(torch.bfloat16)), "the bf16 output is not the rounding of the fp32 output"


def test_im2col_shuffle_and_pool_f32_move_the_exact_values():
    from vtp_amd import ops
    B, h, w, D = 2, 2, 3, 128
    img = torch.randn(B, 3, h * 16, w * 16, device=DEV)
    rows = torch.zeros(B * (h * w + 1), 768, device=DEV)
    ops.im2col16_rows_f32(img, rows, B, h * 16, w * 16, 1)
    ref = F.unfold(img, 16, stride=16).transpose(1, 2)  # [B, hw, 768], K order (c, ky, kx)
    got = rows.view(B, h * w + 1, 768)
    assert torch.equal(got[:, 1:], ref) and bool((got[:, 0] == 0).all())
    t = torch.randn(B * h * w, 768, device=DEV)
    out = torch.empty(B, 3, h * 16, w * 16, device=DEV)
    ops.pixel_shuffle16_f32(t, out, B, h, w)
    assert torch.equal(out, F.pixel_shuffle(t.view(B, h, w, 768).permute(0, 3, 1, 2), 16))
    N = 19
    x = torch.randn(B * N, D, device=DEV)
    pooled = torch.empty(B, D, device=DEV)
    ops.pool_patch_rows_f32(x, pooled, B, N, D)
    ref = x.view(B, N, D)[:, 1:].double().mean(1)
    assert float((pooled.double() - ref).abs().max()) <= gamma(N + 2) * float(x.abs().max())
