"""The fp8 (e4m3) kernels one by one against tests/fp8_ref.py: quantize_e4m3, amax, dequantize_e4m3 (csrc/fp8.hip), norm_fwd_e4m3
(the y8 branch of csrc/norm.hip) and gemm_nt_fp8 (csrc/gemm.hip -> the 256 x 256 8-phase kernel on the f8f6f4 MFMA) with its fp32,
bf16, SwiGLU and fused-RoPE epilogues, static and dynamic tiles.  The cases live in tests/fp8_ref.py; tests/test_fp8_ref_host.py
shows without a GPU that the GEMM inputs leave nothing to round and that wrong variants of a kernel break the comparisons.

Every comparison is an equality of BITS -- but for the SwiGLU hidden output, which goes against float64 under the one bar of the
suite (fp8_ref.swiglu_bar).  No test leaves out elements.

Buffers a kernel must fully write are prefilled with NaN (bytes: the NaN code 0x7F), the row past M and the columns [N, ldc) with a
sentinel that must survive, accumulators with a non-zero value.

Every test prints `fp8_kernels: <kernel> <case>: ...` (profiles/fp8_kernels.log)."""
import functools
import os

import numpy as np
import pytest
import torch

import fp8_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32
NAN = float("nan")
NAN_CODE, SENT_CODE = 0x7F, 0x07


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def report(kernel, case, what):
    print(f"fp8_kernels: {kernel} {case}: {what}")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def canon(q):
    """NaN codes -> 0x7F (the sign of a NaN is not part of the contract)"""
    return torch.where((q & 0x7F) == 0x7F, torch.full_like(q, 0x7F), q)


def n_diff(got, want):
    """number of elements whose bits differ (shapes and types must agree)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return int((R.bits(got) != R.bits(want.to(got.device))).sum())


def guarded(rows, cols, ld, dtype):
    """[rows + 1, ld]: NaN where the kernel must write, the sentinel in the row past `rows` and in the columns [cols, ld)"""
    t = torch.full((rows + 1, ld), R.SENTINEL, dtype=dtype, device=DEV)
    t[:rows, :cols] = NAN
    return t


def guards_untouched(t, rows, cols):
    return bool((t[rows] == R.SENTINEL).all()) and bool((t[:rows, cols:] == R.SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ quantize_e4m3
def run_quantize(x, scale, n=None):
    """n elements of x into a buffer of n + 8 bytes: the last 8 keep the sentinel"""
    from vtp_amd import ops
    n = x.numel() if n is None else n
    q = torch.full((n + 8,), NAN_CODE, dtype=U8, device=DEV)
    q[n:] = SENT_CODE
    ops.quantize_e4m3(x[:n], q[:n], scale)
    assert bool((q[n:] == SENT_CODE).all())
    return q[:n]


def check_quantize(x, scale, case):
    """x: device tensor (bf16 or f32); bytes equal to the reference for the host scale and the device scale"""
    ref = dev(R.canon(R.quantize_ref(x.float().cpu().numpy(), scale)))
    got = run_quantize(x, scale)
    bad = int((canon(got) != ref).sum())
    got_dev = run_quantize(x, torch.tensor([scale], dtype=F32, device=DEV))
    report("quantize_e4m3", case, f"{x.numel()} bytes, {bad} differ from the reference; device scale {'the same bytes' if torch.equal(got, got_dev) else 'DIFFERS'}")
    assert bad == 0, (case, bad, torch.nonzero(canon(got) != ref)[:8].flatten().tolist())
    assert torch.equal(got, got_dev)
    return got


@pytest.mark.parametrize("scale", R.QUANT_SCALES)
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_quantize_code_point_table(dtype, scale):
    x = dev(R.quant_input(scale), dtype)
    got = check_quantize(x, scale, (str(dtype)[6:], "code points", scale))
    nan_in = torch.isnan(x.float())
    assert int(nan_in.sum()) == 2 and torch.equal((got & 0x7F) == 0x7F, nan_in)      # NaN in, NaN code out -- and nowhere else
    inf_in = torch.isinf(x.float())
    assert int(inf_in.sum()) >= 2 and bool(((got[inf_in] & 0x7F) == 0x7E).all())     # +-inf saturates to +-448


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_quantize_smallest_and_grid_stride(dtype):
    table = R.code_point_table()
    x8 = dev(R.midpoints()[40:48].copy(), dtype)                                       # n = 8: one thread, eight ties
    check_quantize(x8, 1.0, (str(dtype)[6:], "n = 8", 1.0))
    n = R.GRID_STRIDE_N8                                                               # grid capped at 8192 blocks: a second sweep
    x = dev(table, dtype).repeat(n // len(table) + 1)[:n].contiguous()
    ref = R.canon(R.quantize_ref(dev(table, dtype).float().cpu().numpy(), 1.0))
    ref = dev(np.resize(ref, n))
    got = run_quantize(x, 1.0)
    bad = int((canon(got) != ref).sum())
    report("quantize_e4m3", (str(dtype)[6:], "grid stride", n), f"{bad} bytes differ from the reference")
    assert bad == 0


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_quantize_keeps_a_nan(dtype):
    g = torch.Generator(device=DEV).manual_seed(11)
    n = 8 * 4096
    for where in (0, n // 2 + 3, n - 1):
        x = (torch.randn(n, device=DEV, generator=g) * 3).to(dtype)
        clean = run_quantize(x, 5.0).clone()
        x[where] = NAN
        got = check_quantize(x, 5.0, (str(dtype)[6:], "NaN at", where))
        assert int(got[where]) & 0x7F == 0x7F, hex(int(got[where]))
        keep = torch.ones(n, dtype=torch.bool, device=DEV)
        keep[where] = False
        assert torch.equal(got[keep], clean[keep])                                     # every other byte as without the NaN


# ------------------------------------------------------------------------------------------------------------ amax
def run_amax(x, prefill):
    from vtp_amd import ops
    am = torch.tensor([prefill, R.SENTINEL], dtype=F32, device=DEV)
    ops.amax(x, am[:1])
    assert float(am[1]) == R.SENTINEL
    return am[:1]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_amax_accumulates_into_the_buffer(dtype):
    n = R.GRID_STRIDE_N8
    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn(n, device=DEV, generator=g).to(dtype)
    x[n - 3] = -1000.0                                                                 # the maximum in the last 8 elements
    true = float(x.float().abs().max())
    assert true == 1000.0
    for prefill, want in ((2000.0, 2000.0), (1.5, true), (0.0, true)):
        got = float(run_amax(x, prefill))
        report("amax", (str(dtype)[6:], "grid stride", n, "prefill", prefill), f"{got} (expected {want})")
        assert got == want
    small = x[:8 * 300]
    assert float(run_amax(small, 1e-3)) == float(small.float().abs().max())


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_amax_signs_zero_and_inf(dtype):
    n = 8 * 1000
    neg = -(torch.rand(n, device=DEV) + 0.5).to(dtype)
    got = run_amax(neg, 0.25)
    assert float(got) == float(neg.float().abs().max())
    mzero = torch.full((n,), -0.0, dtype=dtype, device=DEV)
    z = run_amax(mzero, 0.0)
    assert int(R.bits(z)) == 0                                                         # |-0| = +0
    inf = neg.clone()
    inf[n // 2] = float("-inf")
    got_inf = run_amax(inf, 3.0)
    assert float(got_inf) == float("inf")
    report("amax", (str(dtype)[6:], "all negative / -0 only / -inf"), f"{float(got)} / {float(z)} / {float(got_inf)}")


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_amax_keeps_a_nan(dtype):
    n = R.GRID_STRIDE_N8
    g = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(n, device=DEV, generator=g).to(dtype)
    for where in (0, n // 2 + 5, n - 1):
        y = x.clone()
        y[where] = NAN
        for prefill in (0.0, 5.0, float("inf")):
            got = float(run_amax(y, prefill))
            assert got != got, (where, prefill, got)
        report("amax", (str(dtype)[6:], "NaN at", where), "NaN over the prefills 0, 5 and inf")


# ------------------------------------------------------------------------------------------------------------ dequantize_e4m3
@pytest.mark.parametrize("inv_scale", [1.0, 0.37])
def test_dequantize_every_code_grid_stride(inv_scale):
    from vtp_amd import ops
    n = R.GRID_STRIDE_N4
    codes = np.resize(np.arange(256, dtype=np.uint8), n)
    out = torch.full((n + 4,), NAN, dtype=F32, device=DEV)
    out[n:] = R.SENTINEL
    ops.dequantize_e4m3(dev(codes), out[:n], inv_scale)
    assert bool((out[n:] == R.SENTINEL).all())
    ref = dev(np.resize(R.dequantize_ref(np.arange(256, dtype=np.uint8), inv_scale), n))
    nan = dev(np.resize(np.isin(np.arange(256), R.NAN_CODES), n))
    got = out[:n]
    bad = int((R.bits(got)[~nan] != R.bits(ref)[~nan]).sum())
    nan_ok = bool(torch.isnan(got[nan]).all())
    report("dequantize_e4m3", ("grid stride", n, "inv_scale", inv_scale), f"{bad} finite values differ in bits; NaN codes give NaN: {nan_ok}")
    assert bad == 0 and nan_ok


# ------------------------------------------------------------------------------------------------------------ norm_fwd_e4m3
def run_norm8(x, w, b, scale, stats, M, D, kind):
    from vtp_amd import ops
    y8 = torch.full((M + 1, D), NAN_CODE, dtype=U8, device=DEV)
    y8[M] = SENT_CODE
    ops.norm_fwd_e4m3(x, w, b if kind == 1 else None, y8, scale, stats, M, D, R.NORM_EPS, kind)
    assert bool((y8[M] == SENT_CODE).all())
    return y8[:M]


@pytest.mark.parametrize("kind", [0, 1], ids=["rms", "layernorm"])
@pytest.mark.parametrize("D", R.NORM_D)
def test_norm_fwd_e4m3_is_norm_then_quantize(D, kind):
    """the contract of the kernel's comment: the bf16-rounded output leaves as e4m3(y * q_scale)"""
    from vtp_amd import ops
    for M in R.NORM_M:
        x, w, b = (dev(t) for t in R.norm_case(M, D))
        y = torch.full((M, D), NAN, dtype=BF, device=DEV)
        st = torch.full((M + 1, 2), R.SENTINEL, dtype=F32, device=DEV)
        ops.norm_fwd(x, w, b if kind == 1 else None, y, st, M, D, R.NORM_EPS, kind)
        assert bool(torch.isfinite(y.float()).all())
        scale = (448.0 / torch.quantile(y.float().abs().flatten(), 0.97)).reshape(1).to(F32)   # a few percent saturate
        want = run_quantize(y.flatten(), scale).reshape(M, D)                         # the two-kernel form on the same inputs ...
        ref = dev(R.quantize_ref(y.float().cpu().numpy(), float(scale)))               # ... and the CPU reference of its bytes
        assert torch.equal(want, ref)
        st8 = torch.full((M + 1, 2), R.SENTINEL, dtype=F32, device=DEV)
        got = run_norm8(x, w, b, scale, st8, M, D, kind)
        got_nostats = run_norm8(x, w, b, scale, None, M, D, kind)                      # as the engine calls it
        bad, sat = int((got != want).sum()), float(((want & 0x7F) == 0x7E).float().mean())
        report("norm_fwd_e4m3", ("kind", kind, "M", M, "D", D), f"{bad} bytes differ from norm_fwd + quantize_e4m3; {100 * sat:.1f} % saturated; "
               f"stats bits {'equal' if n_diff(st8, st) == 0 else 'DIFFER'}")
        assert bad == 0 and torch.equal(got_nostats, got)
        assert n_diff(st8, st) == 0                                                    # (the row past M included: untouched)
        assert 0.005 < sat < 0.10 or M * D < 64


@pytest.mark.parametrize("kind", [0, 1], ids=["rms", "layernorm"])
def test_norm_fwd_e4m3_keeps_a_nan_row(kind):
    M, D = 5, 272
    x, w, b = (dev(t) for t in R.norm_case(M, D))
    scale = torch.tensor([100.0], dtype=F32, device=DEV)
    clean = run_norm8(x, w, b, scale, None, M, D, kind).clone()
    x[2, 100] = NAN
    got = run_norm8(x, w, b, scale, None, M, D, kind)
    nan_row = bool(((got[2] & 0x7F) == 0x7F).all())
    others = torch.equal(got[[0, 1, 3, 4]], clean[[0, 1, 3, 4]])
    report("norm_fwd_e4m3", ("kind", kind, "one NaN in row 2 of 5"), f"row 2 all NaN codes: {nan_row}; other rows unchanged: {others}")
    assert nan_row and others


# ------------------------------------------------------------------------------------------------------------ gemm_nt_fp8
@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, lda, ldb):
    c = R.exact_case(M, N, K, lda, ldb)
    return c, dev(c["a8"]), dev(c["b8"]), dev(c["bias"], F32)


def run_gemm(c, a8, b8, bias, kind, with_bias, with_resid, ldc):
    """one launch on guarded buffers -> the [M + 1, ldc] output"""
    from vtp_amd import ops
    M, N, K = c["M"], c["N"], c["K"]
    out = guarded(M, N, ldc, F32 if kind == "f32" else BF)
    resid = None
    if with_resid:
        resid = torch.full((M, ldc), NAN, dtype=F32, device=DEV)
        resid[:, :N] = dev(c["resid"], F32)
    ops.gemm_nt_fp8(a8, b8, out, M=M, N=N, K=K, alpha=R.ALPHA, lda=a8.shape[1], ldb=b8.shape[1], ldc=ldc, bias=bias if with_bias else None,
                    resid=resid, epi=ops.EPI_F32 if kind == "f32" else ops.EPI_BF16)
    return out


def grid_cap(monkeypatch, limit):
    from vtp_amd import _lib
    monkeypatch.setenv("VTP_DIAG", "1")
    _lib.check(_lib.load().vtp_gemm_debug(None, limit, 0), "vtp_gemm_debug")


def grid_cap_off():
    from vtp_amd import _lib
    _lib.load().vtp_gemm_debug(None, 0, 0)


@pytest.mark.parametrize("shape", R.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_gemm_nt_fp8_exact_sum_bit_for_bit(shape, monkeypatch):
    M, N, K, lda, ldb, ldc = shape
    c, a8, b8, bias = gemm_case(M, N, K, lda, ldb)
    capped = (M, N, K) == R.GRID_CAP_SHAPE       # 12 tiles on 8 workgroups: some compute two tiles back to back
    try:
        if capped:
            grid_cap(monkeypatch, 8)
        for kind, with_bias, with_resid in R.GEMM_EPILOGUES:
            out = run_gemm(c, a8, b8, bias, kind, with_bias, with_resid, ldc)
            torch.cuda.synchronize()
            want = R.expected(c, kind, with_bias, with_resid)
            bad = n_diff(out[:M, :N].contiguous(), want)
            report("gemm_nt_fp8", (f"{M}x{N}x{K}", f"lda {lda} ldb {ldb} ldc {ldc}", kind, "bias" if with_bias else "no bias",
                                   "resid" if with_resid else "no resid") + (("grid of 8",) if capped else ()),
                   f"{bad} of {M * N} elements differ in bits; guards {'untouched' if guards_untouched(out, M, N) else 'OVERWRITTEN'}")
            assert bad == 0, (shape, kind, with_bias, with_resid, bad)
            assert guards_untouched(out, M, N)
    finally:
        if capped:
            grid_cap_off()


def run_pair(a8, b8):
    from vtp_amd import ops
    out = guarded(256, 256, 264, F32)
    ops.gemm_nt_fp8(dev(a8), dev(b8), out, M=256, N=256, K=256, alpha=1.0, ldc=264, epi=ops.EPI_F32)
    torch.cuda.synchronize()
    assert guards_untouched(out, 256, 256)
    return out[:256, :256].contiguous()


@pytest.mark.parametrize("kind", ["identity", "37i"])
def test_gemm_nt_fp8_code_pair_table(kind):
    """every finite code times every finite code, one product per output element, in every k position of two k-tiles, in both
    operand slots; then one NaN code in row 5 of A"""
    a8, b8 = R.pair_case(kind)
    want = R.pair_expected()
    bad_ab = n_diff(run_pair(a8, b8), want)
    bad_ba = n_diff(run_pair(b8, a8), want.T.contiguous())
    a8n, _ = R.pair_case(kind, nan_row=5)
    got = run_pair(a8n, b8)
    row5 = bool(torch.isnan(got[5]).all())
    keep = [i for i in range(256) if i != 5]
    bad_rest = n_diff(got[keep], want[keep])
    report("gemm_nt_fp8", ("code pairs", kind), f"{bad_ab} of 65536 products differ in bits, {bad_ba} with the operands swapped; code 0x7F in "
           f"row 5 of A: row 5 of C all NaN: {row5}, {bad_rest} other elements differ")
    assert bad_ab == 0 and bad_ba == 0 and row5 and bad_rest == 0


# ------------------------------------------------------------------------------------------------------------ SwiGLU epilogue
@functools.lru_cache(maxsize=None)
def swiglu_case(M, N, K, lda, ldb):
    c = R.swiglu_case(M, N, K, lda, ldb)
    return c, dev(c["a8"]), dev(c["b8"]), dev(c["bias"], F32), R.swiglu_ref(c)


def run_swiglu(c, a8, b8, bias, with_c2):
    from vtp_amd import ops
    M, N, K, H = c["M"], c["N"], c["K"], c["N"] // 2
    hid = guarded(M, H, H + 8, BF)
    c2 = guarded(M, N, N + 8, BF) if with_c2 else None
    ops.gemm_nt_fp8(a8, b8, hid, M=M, N=N, K=K, alpha=R.ALPHA, lda=a8.shape[1], ldb=b8.shape[1], ldc=H + 8, c2=c2, ldc2=N + 8 if with_c2 else 0,
                    bias=bias, epi=ops.EPI_SWIGLU)
    torch.cuda.synchronize()
    assert guards_untouched(hid, M, H) and (c2 is None or guards_untouched(c2, M, N))
    return hid[:M, :H].contiguous(), None if c2 is None else c2[:M, :N].contiguous()


def check_swiglu(c, hid, x12, ref, case):
    xb, hid64, _ = ref
    bad = n_diff(x12, R.as_bf16(xb))
    r = R.ratio(hid.double().cpu().numpy(), hid64, R.swiglu_bar(hid64))
    report("gemm_nt_fp8 swiglu", case, f"{bad} of {xb.size} pre-activations differ in bits; hid worst error / bar = {r:.3f}")
    assert bad == 0 and r <= 1.0, (case, bad, r)


@pytest.mark.parametrize("shape", R.SWIGLU_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_gemm_nt_fp8_swiglu(shape):
    c, a8, b8, bias, ref = swiglu_case(*shape)
    hid, x12 = run_swiglu(c, a8, b8, bias, True)
    hid_alone, _ = run_swiglu(c, a8, b8, bias, False)      # as the engine calls it
    check_swiglu(c, hid, x12, ref, "x".join(map(str, shape[:3])))
    assert n_diff(hid_alone, hid) == 0


# ------------------------------------------------------------------------------------------------------------ fused RoPE
def rope_setup(reps=1, K=R.ROPE_D):
    """the case of test_gemm_qkv_rope_bit_identical_to_gemm_then_rope with exact-sum e4m3 operands: two resolutions and a cls prefix in one
    launch.  -> (case, a8, b8, bias, rope argument, [(row0, images, tokens, sin, cos)])"""
    from vtp_amd.engine import rope_tables
    segs = R.ROPE_SEGS * reps
    M, D = reps * R.rope_rows(), R.ROPE_D
    c = R.exact_case(M, 3 * D, K, seed=reps)
    per = (100.0 ** (2 * torch.arange(16, dtype=BF) / 32))
    pos, ts, tc, plan, r0, base = [], [], [], [], 0, 0
    for n, h, w in segs:
        sin, cos = rope_tables(per, h, w, torch.device(DEV))
        T = 1 + h * w
        pos.append(torch.cat([torch.tensor([-1], dtype=I32), torch.arange(h * w, dtype=I32) + base]).repeat(n))
        ts.append(sin)
        tc.append(cos)
        plan.append((r0, n, T, sin, cos))
        r0 += n * T
        base += h * w
    rope = (torch.cat(pos).to(DEV), torch.cat(ts).contiguous(), torch.cat(tc).contiguous(), 2 * D)
    return c, dev(c["a8"]), dev(c["b8"]), dev(c["bias"], F32), rope, plan


def run_rope_gemm(c, a8, b8, bias, rope):
    from vtp_amd import ops
    M, N, K = c["M"], c["N"], c["K"]
    out = guarded(M, N, N + 8, BF)
    ops.gemm_nt_fp8(a8, b8, out, M=M, N=N, K=K, alpha=R.ALPHA, ldc=N + 8, bias=bias, epi=ops.EPI_BF16, rope=rope)
    torch.cuda.synchronize()
    assert guards_untouched(out, M, N)
    return out[:M, :N].contiguous()


def test_gemm_nt_fp8_rope_is_gemm_then_rope():
    from vtp_amd import ops
    c, a8, b8, bias, rope, plan = rope_setup()
    M, N = c["M"], c["N"]
    ref = run_rope_gemm(c, a8, b8, bias, None)
    bad_plain = n_diff(ref, R.expected(c, "bf16", True, False))              # the unrotated launch is an exact-sum case of its own
    for r0, n, T, sin, cos in plan:
        ops.rope_qk(ref[r0:r0 + n * T], sin, cos, n, T, R.ROPE_HEADS, 1)
    got = run_rope_gemm(c, a8, b8, bias, rope)
    bad = n_diff(got, ref)
    report("gemm_nt_fp8 rope", (f"{M}x{N}x{c['K']}", "segments", R.ROPE_SEGS), f"{bad} of {M * N} elements differ in bits from gemm_nt_fp8 + "
           f"rope_qk; the unrotated launch: {bad_plain} differ from the reference")
    assert bad == 0 and bad_plain == 0


# ------------------------------------------------------------------------------------------------------------ dynamic tiles
@pytest.mark.parametrize("kind", ["f32 + resid", "swiglu", "rope"])
def test_gemm_nt_fp8_dynamic_tiles_bit_identical_to_static(kind, monkeypatch):
    """gemm8p_dyn_kernel<EPI, 8, XMODE>: what a trainer in the same process switches on with vtp_set_gemm_dynamic(1).  Grid of 8 workgroups,
    12 or more tiles, at least 4 k-tiles (K >= 512 bytes per row: below that the launch keeps the static lists), three launches back to back"""
    from vtp_amd import _lib
    if os.environ.get("VTP_GEMM_DYN") is not None:
        pytest.skip("VTP_GEMM_DYN in the environment overrides vtp_set_gemm_dynamic")
    lib = _lib.load()
    if kind == "f32 + resid":
        M, N, K = R.GRID_CAP_SHAPE
        c, a8, b8, bias = gemm_case(M, N, K, K, K)
        run = lambda: [run_gemm(c, a8, b8, bias, "f32", True, True, N + 8)]
    elif kind == "swiglu":
        M, N, K = R.GRID_CAP_SHAPE
        c, a8, b8, bias, _ = swiglu_case(M, N, K, K, K)
        run = lambda: list(run_swiglu(c, a8, b8, bias, True))
    else:
        c, a8, b8, bias, rope, _ = rope_setup(reps=2, K=512)                           # 2940 rows: 12 x 3 tiles
        assert c["M"] >= 2304
        run = lambda: [run_rope_gemm(c, a8, b8, bias, rope)]
    try:
        grid_cap(monkeypatch, 8)
        _lib.check(lib.vtp_set_gemm_dynamic(0), "vtp_set_gemm_dynamic")
        ref = run()
        torch.cuda.synchronize()
        _lib.check(lib.vtp_set_gemm_dynamic(1), "vtp_set_gemm_dynamic")
        bad = []
        for rep in range(3):   # back to back: the last workgroup of a launch leaves the queue words at zero for the next one
            got = run()
            torch.cuda.synchronize()
            bad.append(sum(n_diff(g, r) for g, r in zip(got, ref)))
    finally:
        lib.vtp_set_gemm_dynamic(0)
        grid_cap_off()
    report("gemm_nt_fp8 dynamic", (kind, f"{c['M']}x{c['N']}x{c['K']}", "grid of 8"), f"elements that differ in bits from the static launch, three launches: {bad}")
    assert bad == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ calibration
def test_fp8_calibration_refuses_a_nan_batch():
    """a NaN that arises in the calibration pass reaches the amax buffer (vtp_amax keeps it) and Stack.fp8_finalize refuses it"""
    from vtp_amd import VTPConfig, VTPModel
    torch.manual_seed(0)
    cfg = VTPConfig(image_size=64, vision_embed_dim=192, vision_depth=2, vision_num_heads=3, text_embed_dim=128, text_depth=1,
                    text_num_heads=2, text_vocab_size=64, text_context_length=8, decoder_embed_dim=192, decoder_depth=2, decoder_num_heads=3)
    m = VTPModel(cfg).to(DEV).eval()
    img = torch.randn(2, 3, 64, 64, device=DEV)
    with torch.no_grad():
        before = m.get_reconstruction_latents(img)
        bad = img.clone()
        bad[1, 2, 17, 40] = NAN
        with pytest.raises(ValueError, match=r"block 0, operand 0") as e:
            m.enable_fp8_forward(bad)
        report("fp8_finalize", "one NaN pixel in the calibration batch", f"ValueError: {e.value}")
        assert torch.equal(m.get_reconstruction_latents(img), before)                  # the bf16 path is still the one that runs
        m.enable_fp8_forward(img)                                                      # and a clean batch calibrates
        assert bool(torch.isfinite(m.get_reconstruction_latents(img).float()).all())
