"""The kernels of the LPIPS training path (csrc/lpips.hip, vtp_conv3x3 of csrc/gemm.hip) restated in plain torch: float64 arithmetic on
the bf16-rounded operands, or the exact bits where the operation can be reproduced.  Not a test module; imported by
tests/test_lpips_ref_host.py (which pins these references against independent torch code, no GPU) and by
tests/test_lpips_kernels_gpu.py.  Nothing here imports vtp_amd, and everything runs on the device of its arguments.

Layouts.  The references take and return plain tensors: images and feature maps NCHW (interior pixels only), the unfolded first
layer as [n, H+2, W+2, 32], tokens as [n*hw, 768] with column c*256 + (Y&15)*16 + (X&15) (the input of PixelShuffle(16)).  `stack` /
`unstack` convert NCHW to and from the kernels' zero-bordered pixel rows with their guard rows (on the GPU).

The input generators (`*_case`) and the bars (`*_bar`) live here too: the host test shows at the GPU test's own inputs that a wrong
variant of each reference misses the GPU test's bar."""
import numpy as np
import torch
import torch.nn.functional as F

from test_lpips_gpu import _stack as stack, _unstack as unstack  # noqa: F401  (the layout pair, shared with the existing tests)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64

SHIFT = (-0.030, -0.088, -0.188)       # the module's ScalingLayer
SCALE = (0.458, 0.448, 0.450)
SHIFT_WIDE = (1.5, -2.25, 0.3)         # values outside [-1, 1]
SCALE_WIDE = (0.37, 2.6, 1.1)


def bf_round(x: torch.Tensor) -> torch.Tensor:
    """f32 values that bf16 holds exactly"""
    return x.to(BF).to(F32)


# --------------------------------------------------------------------------------------------------------- token layout
def _token_index(n, H, W, device):
    """(row [n, 1, H, W], col [1, 3, H, W]) of pixel (b, c, Y, X) in the token matrix [n*hw, 768]"""
    Y = torch.arange(H, device=device).view(1, 1, H, 1)
    X = torch.arange(W, device=device).view(1, 1, 1, W)
    b = torch.arange(n, device=device).view(n, 1, 1, 1)
    c = torch.arange(3, device=device).view(1, 3, 1, 1)
    wt = W >> 4
    return b * ((H >> 4) * wt) + (Y >> 4) * wt + (X >> 4), c * 256 + (Y & 15) * 16 + (X & 15)


def tokens_to_image(tok: torch.Tensor, n, H, W) -> torch.Tensor:
    """[n*hw, 768] -> [n, 3, H, W], same dtype: a gather by the index formula (no pixel_shuffle)"""
    row, col = _token_index(n, H, W, tok.device)
    return tok[row.expand(n, 3, H, W), col.expand(n, 3, H, W)]


def image_to_tokens(img: torch.Tensor) -> torch.Tensor:
    """[n, 3, H, W] -> [n*hw, 768], same dtype: the scatter that inverts tokens_to_image"""
    n, _, H, W = img.shape
    row, col = _token_index(n, H, W, img.device)
    tok = torch.zeros(n * (H >> 4) * (W >> 4), 768, dtype=img.dtype, device=img.device)
    tok[row.expand(n, 3, H, W), col.expand(n, 3, H, W)] = img
    return tok


def _f32_inverse(scale):
    """fp32(1 / scale_c) as the launcher forms it: one IEEE division in fp32"""
    return [float(np.float32(1.0) / np.float32(s)) for s in scale]


# --------------------------------------------------------------------------------------------------------- unfold / fold
def unfold3_ref(img_or_tok: torch.Tensor, H, W, shift, scale) -> torch.Tensor:
    """lpips_unfold3, exact: bf16 [n, H+2, W+2, 32].  Interior row (y, x), column (ky*3+kx)*3+c = bf16(fp32(p - shift_c) * fp32(1/scale_c))
    of source pixel (Y, X) = (y-1+ky-1, x-1+kx-1), zero where (Y, X) is outside the image; columns 27..31 and the border rows are zero.
    Source: f32 NCHW [n, 3, H, W] or bf16 tokens [n*hw, 768]."""
    if img_or_tok.dtype == BF:
        n = img_or_tok.shape[0] // ((H >> 4) * (W >> 4))
        img = tokens_to_image(img_or_tok, n, H, W).to(F32)
    else:
        img = img_or_tok.to(F32)
        n = img.shape[0]
    dev = img.device
    sh = torch.tensor([float(np.float32(s)) for s in shift], dtype=F32, device=dev).view(1, 3, 1, 1)
    inv = torch.tensor(_f32_inverse(scale), dtype=F32, device=dev).view(1, 3, 1, 1)
    scaled = ((img - sh) * inv).to(BF)                      # two fp32 roundings, then round-to-nearest-even to bf16
    pad = torch.zeros(n, 3, H + 2, W + 2, dtype=BF, device=dev)
    pad[:, :, 1:-1, 1:-1] = scaled                          # pad[Y + 1, X + 1] = scaled[Y, X]
    out = torch.zeros(n, H + 2, W + 2, 32, dtype=BF, device=dev)
    for ky in range(3):
        for kx in range(3):
            # interior y = 1..H reads Y = y - 2 + ky, that is pad row y - 1 + ky
            src = pad[:, :, ky:ky + H, kx:kx + W]
            k = (ky * 3 + kx) * 3
            out[:, 1:-1, 1:-1, k:k + 3] = src.permute(0, 2, 3, 1)
    return out


def fold3_ref(dA: torch.Tensor, dt0: torch.Tensor, H, W, scale):
    """lpips_fold3_bwd in float64: dA bf16 [n, H+2, W+2, 32], dt0 bf16 [n*hw, 768] ->
    (dt0 + (sum over the <= 9 taps of dA[(b, Y+2-ky, X+2-kx), (ky*3+kx)*3+c]) / scale_c, sum of |terms|), both float64 [n*hw, 768].
    A tap whose row (y, x) = (Y+2-ky, X+2-kx) is a border row is left out, whatever that row holds."""
    n = dA.shape[0]
    d = dA.to(F64)
    g = torch.zeros(n, 3, H, W, dtype=F64, device=dA.device)
    ga = torch.zeros_like(g)
    for ky in range(3):
        for kx in range(3):
            k = (ky * 3 + kx) * 3
            # y = Y + 2 - ky for Y = 0..H-1 is rows 2-ky .. H+1-ky; interior rows are 1..H
            rows = d[:, 2 - ky:H + 2 - ky, 2 - kx:W + 2 - kx, k:k + 3].permute(0, 3, 1, 2).clone()
            if ky == 2:
                rows[:, :, 0, :] = 0       # y = 0
            if ky == 0:
                rows[:, :, -1, :] = 0      # y = H + 1
            if kx == 2:
                rows[:, :, :, 0] = 0
            if kx == 0:
                rows[:, :, :, -1] = 0
            g += rows
            ga += rows.abs()
    sc = torch.tensor([float(np.float32(s)) for s in scale], dtype=F64, device=dA.device).view(1, 3, 1, 1)
    t0 = dt0.to(F64)
    return t0 + image_to_tokens(g / sc), t0.abs() + image_to_tokens(ga / sc)


def fold_bar(ref: torch.Tensor, sumabs: torch.Tensor) -> torch.Tensor:
    """one bf16 ulp of the stored sum plus the fp32 summation of its terms"""
    return 2.0 ** -7 * ref.abs() + 2.0 ** -20 * sumabs


# --------------------------------------------------------------------------------------------------------- 2x2 max-pool
def _windows(x: torch.Tensor) -> torch.Tensor:
    """[NB, C, H, W] -> [NB, C, H/2, W/2, 4], the window in row-major order"""
    NB, C, H, W = x.shape
    return x.view(NB, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(NB, C, H // 2, W // 2, 4)


def _unwindows(w: torch.Tensor) -> torch.Tensor:
    NB, C, Ho, Wo, _ = w.shape
    return w.view(NB, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(NB, C, 2 * Ho, 2 * Wo)


def maxpool2_fwd_ref(Y: torch.Tensor) -> torch.Tensor:
    return _windows(Y).amax(-1)


def maxpool2_bwd_ref(Y: torch.Tensor, dP: torch.Tensor, tap=None) -> torch.Tensor:
    """maxpool2_bwd, exact: Y, tap f32 [NB, C, H, W] and dP f32 [NB, C, H/2, W/2], all holding bf16 values -> f32 [NB, C, H, W].
    dP goes to the first maximum of each window in row-major order; tap is added in fp32 and the sum rounded to bf16; the result is
    zero where Y <= 0."""
    win = _windows(Y.to(F32))
    hit = win == win.amax(-1, keepdim=True)
    first = hit & (hit.cumsum(-1) == 1)
    dPw = dP.to(F32).unsqueeze(-1).expand_as(win)
    g = _unwindows(torch.where(first, dPw, torch.zeros_like(dPw)))   # +0 where nothing is routed: the bits of a zero count too
    if tap is not None:
        g = bf_round(g + tap.to(F32))
    return torch.where(Y > 0, g, torch.zeros_like(g))


# --------------------------------------------------------------------------------------------------------- the head of one tap
def tap_ref(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor, gscale: float, H: int, W: int, relu_mask: bool = True):
    """lpips_tap in float64: f0, f1 [n, C, h, w] (bf16 values), w [C] -> (val float64 [n], df0 float64 [n, C, h, w]).
        n_i = f_i / (|f_i| + 1e-10),  d = sum_c w_c (n0_c - n1_c)^2,  val[b] = sum over the pixels of d / (H*W),
        df0 = gscale * d(d)/d(f0) where f0 > 0, else 0 (the ReLU in front of the tap).
    df0 is by autograd.  Where |f0| = 0 the derivative of the norm is 0/0; df0 is defined as 0 there, and such pixels are taken out of
    the graph (their d = sum_c w_c n1_c^2 still counts).  H, W are only the divisor of val: the maps are normally [n, C, H, W]."""
    f0 = f0.to(F64).detach().clone().requires_grad_(True)
    f1, w = f1.to(F64), w.to(F64).view(1, -1, 1, 1)
    live = (f0.detach() != 0).any(1, keepdim=True)
    safe = torch.where(live, f0, torch.ones_like(f0))
    n0 = torch.where(live, safe / (safe.pow(2).sum(1, keepdim=True).sqrt() + 1e-10), torch.zeros_like(f0))
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    d = (w * (n0 - n1) ** 2).sum(1)
    (g,) = torch.autograd.grad(d.sum(), f0)
    df0 = gscale * g
    if relu_mask:
        df0 = torch.where(f0.detach() > 0, df0, torch.zeros_like(df0))
    return d.detach().sum((1, 2)) / (H * W), df0


def tap_pixels_f32(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """d per pixel by the kernel's formulas in fp32 torch, [n, h, w]: what fp32 costs before any reordering of the sums"""
    f0, f1, w = f0.to(F32), f1.to(F32), w.to(F32).view(1, -1, 1, 1)
    inv0 = 1.0 / ((f0 * f0).sum(1, keepdim=True).sqrt() + 1e-10)
    inv1 = 1.0 / ((f1 * f1).sum(1, keepdim=True).sqrt() + 1e-10)
    df = f0 * inv0 - f1 * inv1
    return (w * df * df).sum(1)


def tap_pixel_error_f32(f0, f1, w) -> float:
    """largest relative error of a pixel's d in fp32 torch against float64 (pixels with d = 0 are exact in both)"""
    d32 = tap_pixels_f32(f0, f1, w).to(F64)
    f0d, f1d, wd = f0.to(F64), f1.to(F64), w.to(F64).view(1, -1, 1, 1)
    n0 = f0d / (f0d.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1d / (f1d.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    d64 = (wd * (n0 - n1) ** 2).sum(1)
    ok = d64 > 0
    return float(((d32 - d64).abs()[ok] / d64[ok]).max()) if bool(ok.any()) else 0.0


def tap_df_bar(ref: torch.Tensor) -> torch.Tensor:
    """ref [n, C, h, w]: one bf16 rounding of the stored value plus 2^-16 of the pixel's largest gradient (the cancellation in
    dn * inv0 - f0 * k2 is relative to that)"""
    return 2.0 ** -7 * ref.abs() + 2.0 ** -16 * ref.abs().amax(1, keepdim=True)


VAL_PREFILL = 2.0 ** -10   # of the size of one tap's val (about 0.7 / C): the engine adds the five taps into one number
VAL_FACTOR = 8.0           # times the fp32 error of one pixel: block sums in another order and up to 96 atomics per image


def tap_case(C, n, H, W, seed=0):
    """inputs of the head test, on the CPU: f0, f1 f32 [n, C, H, W] = bf16(relu(randn)), w f32 [C] as reset_parameters draws it.
    Image 0 has the f0 pixel (0, 0) all zero; the f1 pixel (H-1, W-1) of image 0 is all zero; with n >= 2 the last image has
    f0 == f1.  With one pixel per image the f1 pixel of image 1 is the zero one and no image has f0 == f1: an ordinary pixel has to be
    left (see tap_identical)."""
    g = torch.Generator().manual_seed(1000 * C + 10 * H + n + seed)
    f0 = bf_round(F.relu(torch.randn(n, C, H, W, generator=g)))
    f1 = bf_round(F.relu(torch.randn(n, C, H, W, generator=g)))
    w = torch.rand(C, generator=g) * (2.0 / C)
    f0[0, :, 0, 0] = 0
    if H * W > 1:
        f1[0, :, H - 1, W - 1] = 0
    else:
        f1[1, :, 0, 0] = 0
    if tap_identical(n, H, W) is not None:
        f1[n - 1] = f0[n - 1]
    return f0, f1, w


def tap_identical(n, H, W):
    """index of the image of tap_case with f0 == f1, or None"""
    return n - 1 if n >= 2 and H * W > 1 else None


TAP_CASES = [(64, 1, 2, 6), (64, 2, 64, 64), (128, 3, 8, 24), (256, 2, 4, 12), (512, 3, 1, 1), (512, 2, 18, 22)]
GSCALES = (1.0, 3.0 / 352)


def pool_case(NB, H, W, C, seed=0):
    """inputs of the max-pool test, on the CPU: Y = bf16(relu(randn)) f32 [NB, C, H, W], dP, tap bf16-valued.  Window (0, 0) of image 0
    holds a positive four-way tie in channels 0..7, only zeros in channels 8..15 and a tie of its second and third pixel in 16..23."""
    g = torch.Generator().manual_seed(100 * NB + 10 * H + W + seed)
    Y = bf_round(F.relu(torch.randn(NB, C, H, W, generator=g)))
    Y[0, 0:8, 0:2, 0:2] = 1.5
    Y[0, 8:16, 0:2, 0:2] = 0
    Y[0, 16:24, 0:2, 0:2] = 0.25
    Y[0, 16:24, 0, 1] = 2.0
    Y[0, 16:24, 1, 0] = 2.0
    dP = bf_round(torch.randn(NB, C, H // 2, W // 2, generator=g))
    tap = bf_round(torch.randn(NB, C, H, W, generator=g))
    return Y, dP, tap


POOL_CASES = [(1, 2, 2, 512), (3, 2, 6, 512), (2, 8, 12, 64), (1, 32, 16, 128)]
UNFOLD_CASES = [(1, 16, 16), (3, 16, 48), (2, 32, 16)]


def unfold_case(n, H, W, seed=0):
    """image f32 [n, 3, H, W] (values beyond [-1, 1]) and tokens bf16 [n*hw, 768] of another image, on the CPU"""
    g = torch.Generator().manual_seed(100 * n + H + W + seed)
    img = 2.0 * torch.randn(n, 3, H, W, generator=g)
    tok = (2.0 * torch.randn(n * (H >> 4) * (W >> 4), 768, generator=g)).to(BF)
    return img, tok


def fold_case(n, H, W, seed=0):
    """dA bf16 [n, H+2, W+2, 32] with zero border rows (columns 27..31 hold finite junk the kernel must not read into the sum) and
    dt0 bf16 [n*hw, 768], on the CPU"""
    g = torch.Generator().manual_seed(100 * n + H + W + 7 + seed)
    dA = torch.zeros(n, H + 2, W + 2, 32, dtype=BF)
    dA[:, 1:-1, 1:-1, :] = torch.randn(n, H, W, 32, generator=g).to(BF)
    dt0 = torch.randn(n * (H >> 4) * (W >> 4), 768, generator=g).to(BF)
    return dA, dt0


# --------------------------------------------------------------------------------------------------------- convolutions
def conv3x3_fwd_ref(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """x [NB, Cin, H, W], w [Cout, Cin, 3, 3] (bf16 values), b f32 [Cout] -> relu(conv2d) in float64"""
    return F.relu(F.conv2d(x.to(F64), w.to(F64), b.to(F64), padding=1))


def conv3x3_dgrad_ref(dy: torch.Tensor, w: torch.Tensor, mask=None) -> torch.Tensor:
    """dy [NB, Cout, H, W], w [Cout, Cin, 3, 3] -> conv_transpose2d in float64, times (mask > 0) when there is a ReLU in front"""
    g = F.conv_transpose2d(dy.to(F64), w.to(F64), padding=1)
    return g if mask is None else g * (mask > 0)


def rows_ref(x: torch.Tensor, w: torch.Tensor, b=None) -> torch.Tensor:
    """the taps = 1 form on NCHW maps: x [NB, Cin, H, W], w [Cout, Cin] -> [NB, Cout, H, W] = x_rows @ w^T in float64 (+ b, ReLU when
    b is given)"""
    y = torch.einsum("nchw,oc->nohw", x.to(F64), w.to(F64))
    return y if b is None else F.relu(y + b.to(F64).view(1, -1, 1, 1))


def conv_bar(ref: torch.Tensor) -> torch.Tensor:
    """the project's bar for the bf16 implicit GEMM (tests/test_lpips_gpu.py)"""
    return 1e-3 * float(ref.abs().max()) + 2.0 ** -7 * ref.abs()
