"""The data-movement and glue kernels of csrc/elementwise.hip and the text glue of csrc/clip.hip restated on the CPU, the case tables
of tests/test_glue_kernels_gpu.py, and the bars.  Not a test module; tests/test_glue_ref_host.py pins the references against the stock
torch ops and shows, at the GPU test's own inputs, that wrong variants are rejected.  Nothing here imports vtp_amd.

Permutations are stated as integer index maps (which flat source element lands in which output element), casts go through
Tensor.to(torch.bfloat16), deterministic fp32 sums are restated in the kernel's own order in float32, and atomic sums are computed in
float64 together with the sum of the absolute values of their terms.

Bars.  U = 2^-24 is the unit roundoff of fp32.  A sum whose longest chain has n fp32 additions (atomics onto one address counted as
sequential, in any order) is off by at most n U (|prefill| + sum|terms|), first order.  The integer cases use small integers whose
sum of absolute values, prefill included, stays below 2^24: every fp32 partial sum is then exact in any order and the result must
equal the float64 sum.  None of the constants was fitted to what the kernels give.

Wrong variants (`wrong=`): 'drop_last_pass' (the last pass of a grid-stride loop not run), 'swap_hw' (token -> (y, x) with h and w
swapped), 'prefix_const' (row offset pre instead of (b + 1) pre), 'skip_tile' (one 64 x 64 tile not written), 'drop_row' (one row missing
from a column sum), 'no_swiglu' (the SwiGLU destination remap left out), 'no_tail' (the scalar tail of the cast skipped), 'past_end'
(a packed scatter that writes the row cu[B]) and 'ignore_accumulate'."""
import functools

import numpy as np
import torch

from oracle import vtp_oracle as O

BF, F32, F64, I32, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64
U = 2.0 ** -24
NAN = float("nan")
SENTINEL = 7.0          # rows and tails a kernel must not touch
PREFILL = 3.0           # accumulators start here (an integer: the integer cases stay exact)
GUARD = 8               # elements / rows behind every output
CAP, L1_CAP, SLAB_CAP = 4096, 1024, 2048      # grid_for(): workgroups of 256 threads


def f32(x) -> float:
    """the fp32 value a C `float` argument holds"""
    return float(np.float32(x))


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 104729 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def cdiv(a, b):
    return -(-a // b)


def pad8(n):
    return cdiv(n, 8) * 8


def bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def same_bits(got, ref) -> bool:
    """bit for bit, except that a NaN need only stay a NaN"""
    got, ref = got.detach(), ref.detach().to(got.device)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    eq = bits(got) == bits(ref)
    if got.is_floating_point():
        eq = eq | (torch.isnan(got) & torch.isnan(ref))
    return bool(eq.all())


def ratio(got, ref, bar) -> float:
    """worst |got - ref| / bar; a non-finite `got` is an infinite ratio; a zero bar must be met exactly"""
    got, ref = torch.as_tensor(got).detach().to(F64).cpu(), torch.as_tensor(ref).detach().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    bar = torch.as_tensor(bar, dtype=F64).expand_as(err)
    inf = torch.full_like(err, float("inf"))
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    r = torch.where(torch.isfinite(got), r, inf)
    return float(r.max()) if r.numel() else 0.0


def atomic_bar(n_adds, sumabs, prefill=PREFILL):
    return n_adds * U * (abs(prefill) + torch.as_tensor(sumabs, dtype=F64))


def assert_exact_case(sumabs, prefill=PREFILL, *values):
    """the integer cases: integers only, and sum|terms| + |prefill| < 2^24 per output, so fp32 adds them exactly in any order"""
    assert float(abs(prefill) + torch.as_tensor(sumabs, dtype=F64).max()) < 2.0 ** 24
    for v in values:
        assert bool((v.double() == v.double().round()).all()) and bool((v.to(BF).double() == v.double()).all())


def draw(shape, g, integer, dtype=F32):
    """a normal draw, or small integers (exact in bf16)"""
    if integer:
        return torch.randint(-3, 4, tuple(shape), generator=g).to(dtype)
    return torch.randn(tuple(shape), generator=g).to(dtype)


def last_pass_start(items, cap):
    """first item of the last pass of `for (i = tid; i < items; i += grid * 256)` with grid = min(cdiv(items, 256), cap)"""
    step = min(max(cdiv(items, 256), 1), cap) * 256
    return (items - 1) // step * step


def passes(items, cap):
    return cdiv(items, min(max(cdiv(items, 256), 1), cap) * 256)


def guarded(shape, dtype, fill=NAN, guard=GUARD):
    """a buffer of `shape` (first dimension extended by `guard`) filled with `fill`, the guard with the sentinel"""
    shape = tuple(shape)
    t = torch.full((shape[0] + guard,) + shape[1:], fill, dtype=dtype)
    t[shape[0]:] = SENTINEL
    return t


# =========================================================================================================== patches and pixels
# One index map serves im2col16 (K order c, ky, kx), its inverse col2im16, PixelShuffle(16) (channel c * 256 + i * 16 + j) and its
# inverse: element k of token `tok` = image element src[tok, k].
PATCH_SHAPES = ((3, 1376, 1360), (2, 32, 48), (1, 16, 16))     # 3 x 86 x 85 = 21 930 tokens: 85 past the 4096 x 256 threads of one pass
PATCH_PREFIXES = (0, 1, 3)
L1_SHAPES = ((3, 43, 43), (2, 2, 3), (1, 1, 1))                # (B, h, w); 5547 tokens against 5461 in a pass of 1024 workgroups


@functools.lru_cache(maxsize=2)
def patch_src(B, H, W, swap=False):
    """int64 [B h w, 768]: the flat index into [B, 3, H, W] of element k = c * 256 + ky * 16 + kx of token (b, y, x)"""
    h, w = H // 16, W // 16
    tok = torch.arange(B * h * w)
    if swap:
        x, y = tok % h, (tok // h) % w
    else:
        x, y = tok % w, (tok // w) % h
    b = tok // (h * w)
    k = torch.arange(768)
    c, ky, kx = k // 256, (k % 256) // 16, k % 16
    src = ((b[:, None] * 3 + c) * H + y[:, None] * 16 + ky) * W + x[:, None] * 16 + kx
    return src % (B * 3 * H * W) if swap else src


def patch_rows(B, H, W, pre, wrong=None):
    """the output row of every token: b * (h w + pre) + pre + p = tok + (b + 1) pre"""
    hw = (H // 16) * (W // 16)
    tok = torch.arange(B * hw)
    return tok + (pre if wrong == "prefix_const" else (tok // hw + 1) * pre)


def patch_live(B, H, W, wrong, cap=CAP):
    """None, or which (tok, k) the variant still writes: a work item is (tok, c, ky), 16 contiguous elements"""
    if wrong != "drop_last_pass":
        return None
    T = B * (H // 16) * (W // 16)
    item = torch.arange(T)[:, None] * 48 + torch.arange(768) // 16
    return item < last_pass_start(T * 48, cap)


def rows_prefill(B, H, W, pre, dtype):
    """[B (h w + pre) + GUARD, 768]: NaN where a patch goes, the sentinel on the prefix rows and the guard"""
    hw = (H // 16) * (W // 16)
    t = guarded((B * (hw + pre), 768), dtype)
    v = t[:B * (hw + pre)].view(B, hw + pre, 768)
    v[:, :pre] = SENTINEL
    return t


def image_prefill(B, H, W):
    return guarded((B * 3 * H * W,), F32)


def im2col_ref(img, B, H, W, pre, dtype, wrong=None):
    """rows [B (h w + pre) + GUARD, 768] of `dtype` after im2col16 / im2col16_rows / _f32 / pixel_unshuffle16 (pre = 0, bf16)"""
    src = patch_src(B, H, W, wrong == "swap_hw")
    row, live = patch_rows(B, H, W, pre, wrong), patch_live(B, H, W, wrong)
    out = rows_prefill(B, H, W, pre, dtype)
    vals = img.reshape(-1)[src].to(dtype)
    out[row] = vals if live is None else torch.where(live, vals, out[row])
    return out


def fold_ref(tokens, B, H, W, wrong=None):
    """image [B 3 H W + GUARD] f32 after col2im16 (f32 tokens) / pixel_shuffle16 (bf16 tokens) / pixel_shuffle16_f32"""
    src, live = patch_src(B, H, W, wrong == "swap_hw"), patch_live(B, H, W, wrong)
    out = image_prefill(B, H, W)
    vals = tokens.to(F32)
    if live is None:
        out[src.reshape(-1)] = vals.reshape(-1)
    else:
        out[src[live]] = vals[live]
    return out


def patch_case(B, H, W):
    """the image, and bf16 decoder tokens"""
    g = gen(B, H, W, 11)
    T = B * (H // 16) * (W // 16)
    return torch.randn(B, 3, H, W, generator=g), torch.randn(T, 768, generator=g).to(BF)


def l1_case(B, h, w, integer):
    """bf16 tokens and an fp32 target with exact ties (d == 0) in one element of every eight"""
    g = gen(B, h, w, 13, integer)
    T = B * h * w
    t = draw((T, 768), g, integer, BF)
    target = draw((B * 3 * h * 16 * w * 16,), g, integer)
    src = patch_src(B, h * 16, w * 16)
    tie = torch.rand(T, 768, generator=g) < 0.125
    target[src[tie]] = t.float()[tie]
    gscale = f32(1.0 / (B * 3 * h * 16 * w * 16))      # the trainer's rec_weight / (B 3 H W) at rec_weight = 1
    return t, target.view(B, 3, h * 16, w * 16), gscale


def l1_ref(t, target, B, h, w, gscale, wrong=None):
    """dt bf16 [T + GUARD, 768] = sign(d) gscale with d = t - target in fp32, the float64 sum of |d| and the bar's addition count"""
    H, W = h * 16, w * 16
    src, live = patch_src(B, H, W, wrong == "swap_hw"), patch_live(B, H, W, wrong, L1_CAP)
    d = t.float() - target.reshape(-1)[src]                       # one fp32 subtraction, the kernel's own
    g = (torch.sign(d) * torch.tensor(gscale, dtype=F32)).to(BF)  # sign(0) = 0
    terms = d.abs().double()
    dt = guarded((B * h * w, 768), BF)
    if live is None:
        dt[:B * h * w] = g
    else:
        dt[:B * h * w] = torch.where(live, g, dt[:B * h * w])
        terms = terms * live
    items = B * h * w * 48
    nblocks = min(cdiv(items, 256), L1_CAP)
    n_adds = passes(items, L1_CAP) * 16 + 6 + 4 + nblocks         # a thread's 16 per pass, the wave tree, 4 wave sums, one atomic per block
    return dt, terms.sum(), n_adds


# =========================================================================================================== token glue
# 22 x 257 x 192 = 1 085 568 float4 items against 1 048 576 in a pass: the second pass is rows 5461 .. 5653, which hold masked rows but no
# cls row (the last is 21 x 257 = 5397); at B = 23 row 5654 is one, so the pass is seen without masks as well
ASSEMBLE_SHAPES = ((22, 257, 768), (23, 257, 768), (3, 10, 128), (2, 5, 4))


def assemble_case(B, N, D, with_masks):
    g = gen(B, N, D, 17)
    x = guarded((B * N, D), F32, 0.0)
    x[:B * N] = torch.randn(B * N, D, generator=g)
    cls, mt = torch.randn(D, generator=g), torch.randn(D, generator=g)
    masks = (torch.rand(B, N - 1, generator=g) < 0.4).to(torch.uint8) if with_masks else None
    return x, cls, mt, masks


def assemble_ref(x, cls, mt, masks, B, N, D, wrong=None):
    out = x.clone()
    v = out[:B * N].view(B, N, D)
    v[:, 0] = cls
    if masks is not None:
        v[:, 1:][masks.bool()] = mt
    if wrong == "drop_last_pass":
        start = last_pass_start(B * N * (D // 4), CAP) * 4
        out.view(-1)[start:B * N * D] = x.view(-1)[start:B * N * D]
    return out


# (B, N, D): 15 rows under the rpb = 16 floor; 259 rows, 16 to a workgroup, N = 37 odd against it and D ragged against the 64-lane chunks;
# 8481 rows at rpb = 17 (waves of 5, 5, 5, 2 rows) and the widest D; 131 070 rows at rpb = 256, a whole wave of 64 rows each
TOKEN_ROWS_SHAPES = ((3, 5, 128), (7, 37, 772), (33, 257, 2048), (510, 257, 128))


def token_rows_plan(rows):
    rpb = min(max(cdiv(rows, 512), 16), 256)
    return rpb, cdiv(rows, rpb)


def token_rows_case(B, N, D, integer):
    """dx f32, the bf16 copy (finite, never zero: a row the kernel must leave alone keeps these bits) and masks with image 0 fully
    masked and image 1 not at all"""
    g = gen(B, N, D, 19, integer)
    dx = draw((B * N, D), g, integer)
    dxb = guarded((B * N, D), BF, 1.0)
    dxb[:B * N] = (torch.randint(1, 4, (B * N, D), generator=g)).to(BF)
    masks = (torch.rand(B, N - 1, generator=g) < 0.5).to(torch.uint8)
    masks[0] = 1
    masks[1] = 0
    return dx, dxb, masks


def token_rows_ref(dx, dxb, masks, B, N, D, with_cls, wrong=None):
    """(dxb after, d_mask sum, its sum|terms|, d_cls sum, its sum|terms|, additions on the longest chain); masks may be None"""
    m = torch.zeros(B, N, dtype=torch.bool)
    if masks is not None:
        m[:, 1:] = masks.bool()
    c = torch.zeros(B, N, dtype=torch.bool)
    c[:, 0] = with_cls
    m, c = m.view(-1), c.view(-1)
    out = dxb.clone()
    out[:B * N][m | c] = 0
    xm, xc = dx[m].double(), dx[c].double()
    if wrong == "drop_row":
        xm, xc = xm[:-1], xc[:-1]
    rpb, nblocks = token_rows_plan(B * N)
    n_adds = cdiv(rpb, 4) + 3 + nblocks
    return out, xm.sum(0), xm.abs().sum(0), xc.sum(0), xc.abs().sum(0), n_adds


STRIDED_B = (1, 3, 4, 5, 257)
STRIDED_D = (64, 100, 1536)


def strided_case(B, D):
    g = gen(B, D, 23)
    stride = D + 36
    return torch.randn(B * stride, generator=g), stride


def strided_rowsum_ref(x, stride, prefill, B, D):
    """fp32, the kernel's order: wave w adds rows w, w + 4, ... onto 0, then out += (p0 + p1) + (p2 + p3)"""
    rows = x[:B * stride].view(B, stride)[:, :D]
    p = [torch.zeros(D) for _ in range(4)]
    for b in range(B):
        p[b % 4] = p[b % 4] + rows[b]
    return prefill + ((p[0] + p[1]) + (p[2] + p[3]))


# =========================================================================================================== layout
TRANSPOSE_R = (1, 63, 64, 65, 517)
TRANSPOSE_C = (8, 72, 352)
IN_REMAP = (7, 2)            # (group, prefix): input row r is read at r + (r // 7 + 1) * 2


def remap_rows(R, grp, pre):
    r = torch.arange(R)
    return r + (r // grp + 1) * pre if grp > 0 else r


def swiglu_h(C):
    return cdiv(C, 16) * 8   # the remap sends column c to (c >> 4) * 8 + (c & 7) (+ H if c & 8): a bijection into [0, 2 H) at this H


def swiglu_dst(C, H):
    c = torch.arange(C)
    return (c >> 4) * 8 + (c & 7) + torch.where((c & 8) != 0, H, 0)


def matrix_case(R, C, integer, remap, key=29):
    """bf16 [rows, C + 8] (ld_in > C; the pad columns and, with the remap, the rows it skips hold NaN: nothing may read them)"""
    g = gen(R, C, key, integer, remap)
    rin = remap_rows(R, *(IN_REMAP if remap else (0, 0)))
    x = torch.full((int(rin[-1]) + 1, C + 8), NAN, dtype=BF)
    x[rin, :C] = draw((R, C), g, integer, BF)
    return x, rin


def colsum_ref(x, rin, C, swiglu, wrong=None, n_rows=None):
    """(float64 column sums at their destinations [2 H or C], sum|terms| there)"""
    live = x[rin[:len(rin) if n_rows is None else n_rows], :C].double()
    if wrong == "drop_row":
        live = live[:-1]
    H = swiglu_h(C) if swiglu else 0
    dst = swiglu_dst(C, H) if swiglu and wrong != "no_swiglu" else torch.arange(C)
    n = 2 * H if swiglu else C
    return torch.zeros(n, dtype=F64).index_add_(0, dst, live.sum(0)), torch.zeros(n, dtype=F64).index_add_(0, dst, live.abs().sum(0))


def transpose_ld_out(R):
    return pad8(R) + 16      # two 8-groups of zero columns behind R


def transpose_ref(x, rin, R, C, wrong=None):
    """bf16 [C + GUARD, ld_out]: row c = column c of the live rows, zero in [R, ld_out), the guard rows untouched"""
    out = guarded((C, transpose_ld_out(R)), BF)
    out[:C] = 0
    out[:C, :R] = x[rin, :C].T
    if wrong == "skip_tile":
        r0, c0 = (R - 1) // 64 * 64, (C - 1) // 64 * 64
        out[c0:C, r0:] = NAN
    return out


def transpose_colsum_adds(R):
    return 3 + 8 + cdiv(transpose_ld_out(R), 64)     # the 3 shuffle levels, 8 LDS atomics per column, one atomic per row tile


COLSUM_R = (1, 255, 256, 257, 1000)
COLSUM_C = 136               # three column blocks, the last 8 wide
COLSUM_ROWS_RMAX = 257


def colsum_adds(R):
    return 8 + 32 + cdiv(R, 256)                     # a thread's 8 rows, 32 partials in sequence, one atomic per 256 rows


# ------------------------------------------------------------------------------------------------------------ casts
def _from_bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


SPECIALS = _from_bits([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000,      # +-0, +-inf, NaN
    0x00000001, 0x80000001, 0x00400000, 0x007FFFFF,                  # fp32 subnormals
    0x00008000, 0x00018000, 0x007F8000,                              # ... on ties: to 0, up to 0x0002, up to the smallest normal
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,                  # exact ties: to even downwards (0x3F80), upwards (0x3F82), and negative
    0x3F808001, 0x3F807FFF,                                          # one ulp either side of a tie
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF])                 # the largest finite fp32 -> inf; a tie -> inf; the largest that stays finite
CAST_N = (1, 2, 3, 5, 1001, 1002, 1003, 4 * (2 ** 20 + 77) + 3)


def cast_case(n):
    """a normal draw with the special values in front and again at the very end (the scalar tail)"""
    x = torch.randn(n, generator=gen(n, 31))
    k = min(n, len(SPECIALS))
    x[:k] = SPECIALS[:k]
    x[n - k:] = SPECIALS[len(SPECIALS) - k:]
    return x


def cast_special_cases():
    """n = 7 (one float4 and a tail of three) at every rotation of the special values: each is cast by the body and by the tail"""
    return [torch.roll(SPECIALS, s)[:7].clone() for s in range(len(SPECIALS))]


def cast_ref(x, wrong=None):
    n = x.numel()
    out = guarded((n,), BF)
    out[:n] = x.to(BF)
    if wrong == "no_tail" and n & 3:
        out[n - (n & 3):n] = NAN
    if wrong == "drop_last_pass":
        out[last_pass_start(n // 4 + 1, CAP) * 4:n - (n & 3)] = NAN     # the launch is sized for n / 4 + 1 items
    return out


CAST_T_SHAPES = ((1, 1), (63, 65), (64, 64), (203, 134), (1, 300))


def cast_t_case(R, C):
    x = torch.randn(R, C, generator=gen(R, C, 37))
    k = min(R * C, len(SPECIALS))
    x.view(-1)[:k] = SPECIALS[:k]
    return x


def cast_t_ref(x, wrong=None):
    R, C = x.shape
    out = guarded((C * R,), BF)
    t = x.to(BF).T.contiguous()
    if wrong == "skip_tile":
        t[(C - 1) // 64 * 64:, (R - 1) // 64 * 64:] = NAN
    out[:C * R] = t.reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------------------ reduce_slabs
SLAB_CASES = tuple((n, S, acc) for n in (4, 1028, 4 * (2 ** 19 + 33)) for S in (1, 3) for acc in (0, 1))   # 524 321 float4 past 2048 x 256


def slab_case(n, S):
    g = gen(n, S, 41)
    stride = n + 12
    dst = guarded((n,), F32, 0.0)
    dst[:n] = torch.randn(n, generator=g)
    return torch.randn(S * stride, generator=g), stride, dst


def reduce_slabs_ref(slabs, stride, S, dst, n, accumulate, wrong=None):
    """fp32, the kernel's order: the slabs in turn onto dst or onto 0"""
    if wrong == "ignore_accumulate":
        accumulate = not accumulate
    a = dst[:n].clone() if accumulate else torch.zeros(n)
    for s in range(S):
        a = a + slabs[s * stride:s * stride + n]
    out = dst.clone()
    out[:n] = a
    if wrong == "drop_last_pass":
        start = last_pass_start(n // 4, SLAB_CAP) * 4
        out[start:n] = dst[start:n]
    return out


# ------------------------------------------------------------------------------------------------------------ prep_weights
# One descriptor table.  (mode, R, C, source key, src offset, src2 offset, dst offset, dstT offset) with offsets in elements into the
# allocation (None: no such output): a non-zero one moves the pointer off its 16-byte (fp32) or 8-byte (bf16) alignment and the kernel
# takes the scalar path; so does a shape with R or C not a multiple of 4.  Descriptors with the same source key convert the same
# values, once on each path: they must give the same bits.  Mode 2 (bias interleave, fp32 -> fp32) has one path only.
PREP_TABLE = (
    (0, 200, 136, "w", 0, None, 0, 0),          # 16-byte path, both outputs; carries the special values
    (0, 203, 134, "odd", 0, None, 0, 0),        # scalar: odd shape
    (0, 200, 136, "w", 1, None, 0, None),       # scalar: source 4 bytes into its allocation; dst only
    (0, 200, 136, "w", 0, None, None, 1),       # scalar: bf16 destination 2 bytes in; dstT only
    (1, 176, 100, "w12", 0, 0, 0, 0),           # 16-byte path, SwiGLU interleave of (w1, w2) [88, 100]
    (1, 176, 100, "w12", 0, 1, 1, 0),           # scalar: w2 4 bytes in, dst 2 bytes in
    (2, 688, 1, "b12", 0, 0, 0, None),          # bias interleave, three tiles of 256
    (2, 688, 1, "b12", 1, 1, 0, None),
    (0, 64, 64, "sq", 0, None, 0, None),        # 16-byte path, one whole tile, dst only
    (0, 128, 196, "wide", 0, None, None, 0),    # 16-byte path, dstT only
    (1, 48, 6, "thin", 0, 0, 0, 0),             # scalar: C = 6
)
PREP_RUNS = ((0, 3), (3, 5), (5, 8), (8, 11), (0, 11)) + tuple((d, d + 1) for d in range(len(PREP_TABLE)))


def prep_tiles(mode, R, C):
    return cdiv(R, 256) if mode == 2 else cdiv(R, 64) * cdiv(C, 64)


def prep_tile_starts():
    s = [0]
    for mode, R, C, *_ in PREP_TABLE:
        s.append(s[-1] + prep_tiles(mode, R, C))
    return s


@functools.lru_cache(maxsize=None)
def prep_source(key):
    """(src, src2 or None) fp32 of the descriptors with this key"""
    mode, R, C = next((m, r, c) for m, r, c, k, *_ in PREP_TABLE if k == key)
    g = gen(len(key), R, C, 43)
    if mode == 0:
        w = torch.randn(R, C, generator=g)
        if key == "w":
            w.view(-1)[5:5 + len(SPECIALS)] = SPECIALS
            w[R - 1, C - len(SPECIALS):] = SPECIALS
        return w, None
    shape = (R // 2, C) if mode == 1 else (R // 2,)
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def interleave_index(R):
    """row g of the SwiGLU-interleaved matrix [8 rows w1 | 8 rows w2 | ...] = row (g >> 4) * 8 + (g & 7) of w2 if g & 8 else of w1"""
    g = torch.arange(R)
    return (g >> 4) * 8 + (g & 7), (g & 8) != 0


def prep_ref(d, wrong=None):
    """(dst, dstT) of descriptor d: bf16 W [R, C] and W^T, or for mode 2 the fp32 interleaved bias and None"""
    mode, R, C, key = PREP_TABLE[d][:4]
    src, src2 = prep_source(key)
    if mode == 0:
        w = src
    else:
        j, second = interleave_index(R)
        w = torch.where(second.view(-1, *([1] * (src.dim() - 1))), src2[j], src[j])
    if mode == 2:
        return w.clone(), None
    wb = w.to(BF)
    wt = wb.T.contiguous()
    if wrong == "skip_tile":
        wb, wt = wb.clone(), wt
        wb[(R - 1) // 64 * 64:, (C - 1) // 64 * 64:] = NAN
        wt[(C - 1) // 64 * 64:, (R - 1) // 64 * 64:] = NAN
    return wb, wt


# =========================================================================================================== RoPE
ROPE_CASES = ((8, 1025, 16, 1, 32, 32), (8, 1025, 16, 0, 25, 41), (2, 7, 3, 1, 2, 3))   # (B, N, heads, prefix, h, w): 1 049 600 items


def rope_case(B, N, heads, prefix, h, w):
    g = gen(B, N, heads, prefix, 47)
    sin, cos = O.rope_table(h, w, O.rope_periods(64))
    assert sin.shape == (N - prefix, 64) and sin.dtype == BF
    return torch.randn(B * N, 3 * heads * 64, generator=g), sin.contiguous(), cos.contiguous()


def rope_ref(qkv, sin, cos, B, N, heads, prefix, inverse=False, wrong=None):
    """eager bf16, three roundings: out = x cos + rot_half(x) sin with rot_half(x) = [-x2, x1]; the inverse is its transpose.  qkv bf16
    [B N, 3 D] -> the same, v and the prefix rows as they were.  qkv fp32 (rope_qk_f32): q and k, prefix rows included, go through bf16
    and come back widened; v keeps its fp32 bits."""
    is_f32 = qkv.dtype == F32
    x = qkv.view(B, N, 3, heads, 64)
    out = x.clone()
    s, c = sin.view(1, N - prefix, 1, 64), cos.view(1, N - prefix, 1, 64)
    s1, s2, c1, c2 = s[..., :32], s[..., 32:], c[..., :32], c[..., 32:]
    for part in (0, 1):
        p = x[:, :, part].to(BF)
        x1, x2 = p[:, prefix:, :, :32], p[:, prefix:, :, 32:]
        if not inverse:
            o1, o2 = x1 * c1 + (-x2) * s1, x2 * c2 + x1 * s2
        else:
            o1, o2 = x1 * c1 + x2 * s2, x2 * c2 + (-x1) * s1
        r = torch.cat((p[:, :prefix], torch.cat((o1, o2), -1)), 1) if is_f32 else torch.cat((x[:, :prefix, part], torch.cat((o1, o2), -1)), 1)
        out[:, :, part] = r.to(qkv.dtype)
    if wrong == "drop_last_pass":
        total = B * N * 2 * heads * 4
        live = (torch.arange(total) < last_pass_start(total, CAP)).view(B, N, 2, heads, 1, 4).expand(B, N, 2, heads, 2, 4)
        live = live.unsqueeze(-1).expand(B, N, 2, heads, 2, 4, 8).reshape(B, N, 2, heads, 64)
        out[:, :, :2] = torch.where(live, out[:, :, :2], x[:, :, :2])
    return out.view(B * N, 3 * heads * 64)


# =========================================================================================================== text glue
TEXT_D = (128, 768, 1284)
TEXT_T = (16, 77)
TEXT_V = 24                   # a small vocabulary: the captions repeat tokens and the atomics on d_table collide


def text_lengths(T, full):
    """caption lengths: 1, values in between and, with `full`, T itself; otherwise the longest is T - 3 and d_pos rows beyond it get nothing"""
    return [1, T if full else T - 3, 5, T // 2, 2, T - 4, 1]


def text_case(T, D, full, integer):
    g = gen(T, D, full, integer, 53)
    lens = text_lengths(T, full)
    B = len(lens)
    ids = torch.randint(1, TEXT_V - 1, (B, T), generator=g)
    ids[torch.arange(B), torch.tensor(lens) - 1] = TEXT_V - 1           # the EOT: the largest id, first at position len - 1
    ids[2, lens[2]:] = TEXT_V - 1                                       # ... and repeated behind it: the first maximum counts
    table, pos = draw((TEXT_V, D), g, integer), draw((T, D), g, integer)
    dy = draw((B, D), g, integer)
    dx = draw((B * T, D), g, integer)
    return ids, lens, table, pos, dy, dx


def text_plan_ref(ids):
    eot = ids.argmax(-1)
    first = (ids == ids.max(-1, keepdim=True).values).int().argmax(-1)      # the first maximum, stated without relying on argmax's tie rule
    assert torch.equal(eot, first)
    cu = torch.zeros(ids.shape[0] + 1, dtype=I64)
    cu[1:] = torch.cumsum(eot + 1, 0)
    return eot.to(I32), cu.to(I32)


def live_rows(cu, T):
    """packed row -> padded row b * T + t, for the rows [0, cu[B])"""
    B = cu.numel() - 1
    return torch.cat([b * T + torch.arange(int(cu[b + 1] - cu[b])) for b in range(B)])


def embed_ref(ids, table, pos):
    """x[b T + t] = table[ids[b, t]] + pos[t]: one fp32 addition"""
    B, T = ids.shape
    return (table[ids.reshape(-1)] + pos.repeat(B, 1))


def scatter_ref(dy, eot, B, T, D, dtype=F32):
    out = torch.zeros(B * T, D, dtype=dtype)
    out[torch.arange(B) * T + eot.long()] = dy.to(dtype)
    return out


def packed(padded, cu, T, fill=SENTINEL, wrong=None):
    """the live rows of a padded [B T, D] buffer back to back, `GUARD` sentinel rows behind cu[B]"""
    rows = live_rows(cu, T)
    out = guarded((rows.numel(), padded.shape[1]), padded.dtype, fill)
    out[:rows.numel()] = padded[rows]
    if wrong == "past_end":
        out[rows.numel()] = 0
    return out


def embed_bwd_ref(ids, dx, lens=None):
    """float64 d_table [V, D] and d_pos [T, D] with their sum|terms|, and the additions per output ([V, 1] and a number).  dx is padded
    [B T, D]; with `lens` only the rows t < len count (the packed form)."""
    B, T = ids.shape
    D = dx.shape[1]
    live = torch.ones(B, T, dtype=torch.bool) if lens is None else torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    g = (dx.view(B, T, D) * live[..., None]).double()
    flat_ids = ids.reshape(-1)
    d_table = torch.zeros(TEXT_V, D, dtype=F64).index_add_(0, flat_ids, g.view(B * T, D))
    a_table = torch.zeros(TEXT_V, D, dtype=F64).index_add_(0, flat_ids, g.view(B * T, D).abs())
    counts = torch.zeros(TEXT_V, dtype=F64).index_add_(0, flat_ids, live.reshape(-1).double())
    return d_table, a_table, counts.view(-1, 1), g.sum(0), g.abs().sum(0), B + 1
