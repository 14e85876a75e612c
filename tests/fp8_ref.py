"""CPU reference of the fp8 (e4m3) kernels and the cases tests/test_fp8_kernels_gpu.py runs (tests/test_fp8_ref_host.py proves both
without a GPU).

* An own e4m3 codec (OCP "fn": 4 exponent bits of bias 7, 3 mantissa bits, no infinity, S.1111.111 = NaN, maximum 448, subnormals =
  multiples of 2^-9) in integer / float64 arithmetic: DECODE (256 entries) and encode() = clamp to +-448, round to nearest, ties to
  the even code.  quantize_ref() is what vtp_quantize_e4m3 computes: ONE float32 product x * scale, clamp, encode -- exact bytes.
* GEMM operands for which the fp32 result does not depend on the order of summation, so that the device output is compared BIT FOR
  BIT: "exact-sum" operands (elements = the 49 e4m3 values that are multiples of 1/8 with |v| <= 4: every product is a multiple of
  2^-6 of magnitude <= 16 and every partial sum over K <= 16384 of them fits in 24 bits; alpha = 2^-4, bias multiples of 2^-6 in
  [-8, 8], residual multiples of 2^-6 in [-64, 64]: acc * alpha + bias (+ resid) is representable in fp32 in any order, fused or not)
  and the code-pair table (C[i, j] = the single product val(i) * val(j) of two codes, at most 8 significant bits).
* The SwiGLU epilogue with the rounding points csrc/gemm_common.h states, and the one bar of the suite (hid against float64).

A bit-exact comparison that fails on the device is an indexing or decode error: these inputs leave nothing to round."""
import numpy as np
import torch

SENTINEL = 7.0
E4M3_MAX = 448.0


# ------------------------------------------------------------------------------------------------------------------ the codec
def decode_table(bias=7):
    """float64 [256]: the value of every code (bias 7: OCP e4m3fn; bias 8 is the WRONG-variant table of the fnuz exponent bias)"""
    t = np.empty(256, np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** (1 - bias - 3)
        else:
            v = (8 + m) * 2.0 ** (e - bias - 3)
        t[c] = -v if c & 0x80 else v
    return t


DECODE = decode_table()
NAN_CODES = (0x7F, 0xFF)


def encode(v):
    """uint8 codes of float values (any float array; computed in float64, which holds every float32 exactly): clamp to +-448, round
    to nearest with ties to the even code; NaN -> 0x7F; the sign of a zero is kept"""
    v = np.asarray(v, np.float64)
    a = np.minimum(np.abs(v), E4M3_MAX)          # (NaN stays NaN through np.minimum)
    nan = np.isnan(v)
    a = np.where(nan, 0.0, a)
    _, ex = np.frexp(a)                          # a = m * 2^ex, m in [0.5, 1)
    e = np.where(a == 0, -6, np.maximum(ex - 1, -6))  # exponent of the code's binade; below 2^-6: the subnormal binade (step 2^-9)
    q = np.rint(np.ldexp(a, 3 - e)).astype(np.int64)  # multiples of the binade's step; np.rint rounds half to even
    # q in [0, 16]: q == 16 is the next binade's first code and q < 8 a subnormal -- (e + 6) * 8 + q is the code in every case
    # ((e + 7) << 3 | (q - 8) for a normal; q itself for a subnormal, e = -6)
    code = (e + 6) * 8 + q
    code = np.where(nan, 0x7F, code | np.where(np.signbit(v), 0x80, 0))
    return code.astype(np.uint8)


def canon(codes):
    """NaN codes (S.1111.111) -> 0x7F: the sign of a NaN is not part of the contract"""
    codes = np.asarray(codes, np.uint8)
    return np.where((codes & 0x7F) == 0x7F, 0x7F, codes).astype(np.uint8)


def quantize_ref(x, scale):
    """bytes of vtp_quantize_e4m3: x float32 (a bf16 input widened exactly), ONE IEEE float32 product, clamp, encode"""
    with np.errstate(invalid="ignore", over="ignore"):
        return encode(np.asarray(x, np.float32) * np.float32(scale))


def dequantize_ref(codes, inv_scale):
    with np.errstate(invalid="ignore"):
        return DECODE[np.asarray(codes, np.uint8)].astype(np.float32) * np.float32(inv_scale)


def bits(t):
    """torch tensor -> its bit pattern as integers (bf16 -> int16, f32 -> int32)"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def bf16_bits_ulp(x, k):
    """float32 array of bf16-representable values moved k bf16 ulps (away from zero for k > 0)"""
    u = np.asarray(x, np.float32).view(np.uint32)
    return ((u.astype(np.int64) + (k << 16)).astype(np.uint32)).view(np.float32)


def f32_bits_ulp(x, k):
    u = np.asarray(x, np.float32).view(np.uint32)
    return ((u.astype(np.int64) + k).astype(np.uint32)).view(np.float32)


def midpoints():
    """float32: the midpoint of every pair of neighbouring non-negative codes (0 | 2^-9 ... 416 | 448), both signs: 5 significant bits"""
    pos = DECODE[:0x7F]
    mid = (pos[:-1] + pos[1:]) / 2
    return np.concatenate([mid, -mid]).astype(np.float32)


def code_point_table():
    """float32 inputs at which a quantiser goes wrong: every code value (the two NaN codes give NaN inputs), every midpoint between
    neighbouring codes (ties), each midpoint +- one ulp of bf16 and of f32, the subnormal range in steps of 2^-11, 2^-10 (ties to
    zero), +-0, f32 denormals, 448 and beyond (464 = the last value that rounds to 448 unclamped, 465, 1e4, 3e38), +-inf.  Its length is a
    multiple of 8."""
    mid = midpoints()
    sub = (np.arange(0, 65) * 2.0 ** -11).astype(np.float32)  # 0 .. 2^-5 in quarter steps of the subnormal spacing
    hand = np.array([0.0, -0.0, 2.0 ** -10, -2.0 ** -10, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 2.0 ** -126, 448.0, -448.0, 464.0, -464.0,
                     465.0, -465.0, 1e4, -1e4, 3e38, -3e38, np.inf, -np.inf, 17.0, 19.0, 0.0156, 240.0], np.float32)
    t = np.concatenate([DECODE.astype(np.float32), mid, bf16_bits_ulp(mid, 1), bf16_bits_ulp(mid, -1), f32_bits_ulp(mid, 1),
                        f32_bits_ulp(mid, -1), sub, -sub, hand])
    return np.concatenate([t, np.zeros(-len(t) % 8, np.float32)])


QUANT_SCALES = (1.0, 2.0 ** -3, 1.7)
GRID_STRIDE_N8 = 8 * (8192 * 256 + 77)   # quantise / amax: 8 elements per thread, grid capped at 8192 blocks of 256 -> a second sweep
GRID_STRIDE_N4 = 4 * (8192 * 256 + 77)   # dequantise: 4 per thread


def quant_input(scale):
    """the code-point table placed so that x * scale lands ON the table for the power-of-two scales (exact division)"""
    t = code_point_table()
    with np.errstate(over="ignore"):
        return (t / np.float32(scale)).astype(np.float32) if scale in (1.0, 2.0 ** -3) else t


# ------------------------------------------------------------------------------------------------------------------ norm cases
NORM_D = (16, 192, 272, 768, 1040, 2048)   # one partly filled chunk, ragged second and fifth chunks, the maximum
NORM_M = (1, 5, 130)                       # a partly filled 4-row workgroup
NORM_EPS = 1e-6


def norm_case(M, D, seed=0):
    g = torch.Generator().manual_seed(1000 * D + M + seed)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    w = 1 + 0.2 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    return x, w, b


# ------------------------------------------------------------------------------------------------------------------ exact-sum GEMMs
EXACT_VALUES = np.array(sorted({float(v) for v in DECODE if np.isfinite(v) and abs(v) <= 4 and float(v * 8).is_integer()}))  # 49
ALPHA = 2.0 ** -4
# M, N, K, lda, ldb, ldc
GEMM_SHAPES = ((1, 4, 16, 16, 16, 4 + 8),            # the smallest legal launch
               (33, 36, 48, 48, 48, 36 + 8),         # all three tails inside one tile; K is three 16-byte pieces
               (256, 256, 128, 128, 128, 256 + 8),   # exactly one tile and one k-tile
               (257, 260, 144, 144, 144, 260 + 8),   # one row and four columns into the next tiles; one k-tile plus one piece
               (300, 520, 2736, 2752, 2768, 528),    # leading dimensions above the extents, NaN codes in the padding
               (768, 1024, 512, 512, 512, 1024 + 8))  # persistent grid capped at 8 workgroups: 12 tiles
GRID_CAP_SHAPE = (768, 1024, 512)
GEMM_EPILOGUES = (("f32", True, True), ("f32", True, False), ("f32", False, False), ("bf16", True, False), ("bf16", False, False))


def pad_codes(v, ld):
    """[rows, K] float64 values -> uint8 [rows, ld]: their codes, the columns [K, ld) filled with the NaN code 0x7F (a read past K
    poisons the output)"""
    out = np.full((v.shape[0], ld), 0x7F, np.uint8)
    out[:, :v.shape[1]] = encode(v)
    return out


def exact_case(M, N, K, lda=None, ldb=None, seed=0, extreme=True):
    """exact-sum operands: dict with the float64 values a [M, K], b [N, K], their bytes a8 [M, lda], b8 [N, ldb], bias [N], resid [M, N].
    extreme: the last row of a and the last row of b are all 4, so C[M-1, N-1] sums K products of 16 (the largest partial sums)"""
    rng = np.random.default_rng(100003 * M + 1009 * N + K + seed)
    a = EXACT_VALUES[rng.integers(0, len(EXACT_VALUES), (M, K))]
    b = EXACT_VALUES[rng.integers(0, len(EXACT_VALUES), (N, K))]
    if extreme:
        a[M - 1], b[N - 1] = 4.0, 4.0
    bias = rng.integers(-512, 513, N) / 64.0
    resid = rng.integers(-4096, 4097, (M, N)) / 64.0
    return dict(M=M, N=N, K=K, a=a, b=b, a8=pad_codes(a, lda or K), b8=pad_codes(b, ldb or K), bias=bias, resid=resid)


def gemm_ref(a, b, alpha=ALPHA, bias=None, resid=None, alpha_after_bias=False):
    """float64 [M, N] = alpha * a b^T (+ bias) (+ resid); exact for exact-sum operands (sums below 2^24 units of 2^-6 fit float64 by far)"""
    acc = a @ b.T
    if alpha_after_bias:
        c = (acc + (0 if bias is None else bias)) * alpha
    else:
        c = acc * alpha + (0 if bias is None else bias)
    return c if resid is None else c + resid


def as_f32(c):
    return torch.from_numpy(np.ascontiguousarray(c, np.float64)).to(torch.float32)


def as_bf16(c):
    """one round-to-nearest-even of a value that float32 holds exactly (asserted by the host test for every case)"""
    return as_f32(c).to(torch.bfloat16)


def expected(case, kind, with_bias, with_resid):
    c = gemm_ref(case["a"], case["b"], ALPHA, case["bias"] if with_bias else None, case["resid"] if with_resid else None)
    return as_f32(c) if kind == "f32" else as_bf16(c)


def wrong_variants(case):
    """name -> float64 result of a kernel that is wrong in one way, for the (bias + resid) fp32 epilogue; a variant that the shape has no
    room for (a neighbouring row at M = 1, a neighbouring 4-column group at N = 4) is left out"""
    a, b, bias, resid = case["a"], case["b"], case["bias"], case["resid"]
    out = {}
    a_cut = a.copy()
    a_cut[:, -16:] = 0
    out["last 16-byte K piece dropped"] = gemm_ref(a_cut, b, ALPHA, bias, resid)
    good = gemm_ref(a, b, ALPHA, bias, resid)
    if case["M"] >= 2:
        c = good.copy()
        c[-1] = c[-2]
        out["last row taken from its neighbour"] = c
    if case["N"] >= 8:
        c = good.copy()
        c[:, -4:] = c[:, -8:-4]
        out["last 4-column group taken from its neighbour"] = c
    out["alpha applied after the bias"] = gemm_ref(a, b, ALPHA, bias, resid, alpha_after_bias=True)
    fnuz = decode_table(8)
    out["table decoded with bias 8 (fnuz)"] = gemm_ref(fnuz[encode(a)], fnuz[encode(b)], ALPHA, bias, resid)
    return out


# ------------------------------------------------------------------------------------------------------------------ code-pair table
def pair_perm(kind):
    i = np.arange(256)
    return i if kind == "identity" else (37 * i) % 256


def pair_case(kind, nan_row=None):
    """a8[i, p(i)] = code i, zero elsewhere; b8[j, :] = code j; the NaN codes are replaced by 0.  C[i, j] = val(i) * val(j), a single
    product.  nan_row: the code 0x7F in one more element of that row of a8"""
    codes = np.arange(256, dtype=np.uint8)
    codes[list(NAN_CODES)] = 0
    p = pair_perm(kind)
    a8 = np.zeros((256, 256), np.uint8)
    a8[np.arange(256), p] = codes
    b8 = np.repeat(codes[:, None], 256, 1)
    if nan_row is not None:
        a8[nan_row, (p[nan_row] + 101) % 256] = 0x7F
    return a8, np.ascontiguousarray(b8)


def pair_expected():
    """float32 [256, 256]; a zero product leaves the accumulator at +0 (it starts there, and +0 + -0 = +0)"""
    v = np.where(np.isnan(DECODE), 0.0, DECODE)
    c = np.outer(v, v)
    return as_f32(np.where(c == 0, 0.0, c))


# ------------------------------------------------------------------------------------------------------------------ SwiGLU epilogue
SWIGLU_SHAPES = ((33, 32, 48, 48, 48), (257, 528, 144, 144, 144), (300, 688, 2736, 2752, 2768))  # M, 2H, K, lda, ldb
SWIGLU_X1_MAX = 30.0


def bf16_round(x):
    """float64 -> the nearest bf16 value (8 significant bits, ties to even), kept in float64; normal range only"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def swiglu_case(M, N, K, lda=None, ldb=None):
    """exact-sum operands whose x1 columns stay within +-30: the w1 rows of b hold the small values (|v| <= 1/2) only, and the bias of
    a column whose pre-activations still reach further is moved to the middle of the column's range (still a multiple of 2^-6)"""
    case = exact_case(M, N, K, lda, ldb, seed=7, extreme=False)
    is_x1 = (np.arange(N) % 16) < 8
    small = EXACT_VALUES[np.abs(EXACT_VALUES) <= 0.5]
    rng = np.random.default_rng(N + K)
    case["b"][is_x1] = small[rng.integers(0, len(small), (int(is_x1.sum()), K))]
    case["b8"] = pad_codes(case["b"], ldb or K)
    x = gemm_ref(case["a"], case["b"], ALPHA, case["bias"])
    lo, hi = x.min(0), x.max(0)
    shift = np.where(np.maximum(np.abs(lo), np.abs(hi)) > SWIGLU_X1_MAX - 1, -np.rint((lo + hi) / 2 * 64) / 64, 0.0)
    case["bias"] = case["bias"] + np.where(is_x1, shift, 0.0)
    return case


def silu(x):
    return x / (1.0 + np.exp(-x))


def swiglu_ref(case, swap=False, round_silu=True, group_shift=0):
    """-> (x12 float64 [M, 2H]: the bf16 pre-activations, exact; hid64 [M, H]: float64 silu(x1b) * x2b; hid_rp [M, H]: the same with the
    epilogue's rounding points hid = bf16(bf16(silu(x1b)) * x2b)).  gemm columns come in 16-column groups = 8 of x1 | 8 of x2; hidden
    column 8 g + e pairs the columns 16 g + e and 16 g + 8 + e.  swap / round_silu / group_shift: the wrong variants of the host test"""
    M, N = case["M"], case["N"]
    x = gemm_ref(case["a"], case["b"], ALPHA, case["bias"])
    xb = bf16_round(x)
    g = xb.reshape(M, N // 16, 2, 8)
    x1b, x2b = g[:, :, 0, :].reshape(M, N // 2), g[:, :, 1, :].reshape(M, N // 2)
    if swap:
        x1b, x2b = x2b, x1b
    hid64 = silu(x1b) * x2b
    s = bf16_round(silu(x1b)) if round_silu else silu(x1b)
    hid_rp = bf16_round(s * x2b)
    if group_shift:
        hid_rp = np.roll(hid_rp, 8 * group_shift, 1)
    return xb, hid64, hid_rp


def swiglu_bar(hid64):
    """two bf16 roundings at 2^-8 each, plus 2^-14 for the device expf / reciprocal, plus the smallest normal"""
    return (2.0 ** -7 + 2.0 ** -14) * np.abs(hid64) + 2.0 ** -126


def ratio(got, ref, bar):
    """worst |got - ref| / bar; a NaN anywhere is an infinite ratio"""
    r = np.abs(np.asarray(got, np.float64) - ref) / bar
    return float("inf") if np.isnan(r).any() else float(r.max())


# ------------------------------------------------------------------------------------------------------------------ fused RoPE
ROPE_HEADS, ROPE_D = 4, 256
ROPE_SEGS = ((3, 16, 16), (5, 6, 6), (2, 16, 16))   # (images, h, w): 1 + h * w tokens each (a cls prefix)


def rope_rows():
    return sum(n * (1 + h * w) for n, h, w in ROPE_SEGS)
