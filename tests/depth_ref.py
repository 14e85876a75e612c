"""Helper of the depth-probe tests (not a test): an fp64 torch restatement of the linear depth probe -- logits upsampled with the
taps of tests/seg_ref.py (ATen's upsample_bilinear2d, align_corners=False), the linear normalisation a_c = max(z_c, 0) + 0.1 over
uniform bin centres, the scale-invariant log loss over the valid pixels, its gradient with respect to the low-resolution logits as
the explicit sum over pixels, the evaluation counters and metrics, and one SGD-with-momentum step.  tests/test_depthprobe_host.py
pins it to torch's own CPU ops (F.interpolate, relu, autograd); tests/test_depthprobe_gpu.py checks the kernels
(csrc/depthprobe.hip) against it."""
import math

import torch

import seg_ref as S

F64 = torch.float64
gamma, taps, tap_matrix, upsample, sgd_step, cosine_lr = S.gamma, S.taps, S.tap_matrix, S.upsample, S.sgd_step, S.cosine_lr


def f32(x):
    """the fp32 value a kernel receives for the Python float x"""
    return float(torch.tensor(x, dtype=torch.float32))


MIN_DEPTH, MAX_DEPTH, LAM = f32(0.001), 10.0, f32(0.85)


def bin_centres(C, lo=MIN_DEPTH, hi=MAX_DEPTH):
    """e_c = lo + (hi - lo) c / (C - 1), fp64 [C]"""
    return lo + (hi - lo) * torch.arange(C, dtype=F64) / (C - 1)


def valid_mask(gt, hi=MAX_DEPTH):
    """bool [B, Hl, Wl]: 0 < gt <= hi; NaN and inf are invalid"""
    return (gt > 0) & (gt <= hi)


def loss_and_grad(z, gt, lo=MIN_DEPTH, hi=MAX_DEPTH, lam=LAM):
    """z [B, h, w, C] (any float dtype, taken to fp64), gt float [B, Hl, Wl] -> dict with up [B, Hl, Wl, C], S and dhat [B, Hl, Wl],
    valid, n, g (0 on invalid pixels), m1, m2, loss L = sqrt(max(m2 - lam m1^2, 0)) (0 without a valid pixel), q [B, Hl, Wl] =
    (g - lam m1) / (n L dhat S) on the valid pixels, and G [B, h, w, C] = sum_p w_p(i, j) q_p [z_p[c] > 0] (e_c - dhat_p): the explicit
    sum, the weight of cell (i, j) in pixel p being the product of the axis weights of tap_matrix; 0 when n = 0 or L = 0"""
    z = z.to(F64)
    B, h, w, C = z.shape
    Hl, Wl = gt.shape[1:]
    e = bin_centres(C, lo, hi)
    up = upsample(z, Hl, Wl)
    a = up.clamp_min(0.0) + 0.1
    Ssum = a.sum(-1)
    dhat = (a * e).sum(-1) / Ssum
    ok = valid_mask(gt, hi)
    n = int(ok.sum())
    gt64 = torch.where(ok, gt.to(F64), torch.ones((), dtype=F64))
    g = torch.where(ok, dhat.log() - gt64.log(), torch.zeros((), dtype=F64))
    m1 = float(g.sum() / n) if n else 0.0
    m2 = float((g * g).sum() / n) if n else 0.0
    L = math.sqrt(max(m2 - lam * m1 * m1, 0.0))
    if n and L > 0:
        q = (g - lam * m1) / (n * L * dhat * Ssum) * ok
    else:
        q = torch.zeros_like(g)
    d = q[..., None] * (up > 0) * (e - dhat[..., None])
    G = torch.einsum("yi,xj,byxc->bijc", tap_matrix(Hl, h), tap_matrix(Wl, w), d)
    return dict(up=up, S=Ssum, dhat=dhat, valid=ok, n=n, g=g, m1=m1, m2=m2, loss=L, q=q, G=G, e=e)


def counters(dhat, gt, hi=MAX_DEPTH):
    """(int64 [4] = valid pixels and those with max(dhat / gt, gt / dhat) < 1.25^k for k = 1, 2, 3; fp64 [6] = sums over the valid
    pixels of g, g^2, |dhat - gt| / gt, (dhat - gt)^2 / gt, (dhat - gt)^2, |g| / ln 10) of dhat, gt [..., Hl, Wl]"""
    ok = valid_mask(gt, hi)
    d, t = dhat.to(F64)[ok], gt.to(F64)[ok]
    g = d.log() - t.log()
    ratio = torch.maximum(d / t, t / d)
    counts = torch.tensor([d.numel()] + [int((ratio < 1.25 ** k).sum()) for k in (1, 2, 3)], dtype=torch.int64)
    diff = d - t
    sums = torch.stack([g.sum(), (g * g).sum(), (diff.abs() / t).sum(), (diff * diff / t).sum(), (diff * diff).sum(),
                        (g.abs() / math.log(10.0)).sum()])
    return counts, sums


def metrics(counts, sums):
    """the reported numbers from the counters, by their direct formulas"""
    n = int(counts[0])
    s = [float(v) / n for v in sums]
    return dict(abs_rel=s[2], sq_rel=s[3], rmse=math.sqrt(s[4]), rmse_log=math.sqrt(s[1]), log10=s[5],
                silog=100.0 * math.sqrt(max(s[1] - s[0] ** 2, 0.0)), d1=int(counts[1]) / n, d2=int(counts[2]) / n, d3=int(counts[3]) / n,
                valid=n)


class RefDepth:
    """heads: [(key, n_blocks, lr)]; weights: key -> (W [C, n Dc], b [C]).  X_all [B h w, n_max Dc]: a head reads its trailing n Dc columns."""

    def __init__(self, heads, weights, Dc, momentum=0.9, max_iter=None, lo=MIN_DEPTH, hi=MAX_DEPTH, lam=LAM):
        self.heads, self.Dc, self.momentum, self.max_iter, self.lo, self.hi, self.lam = list(heads), Dc, momentum, max_iter, lo, hi, lam
        self.n_max = max(h[1] for h in self.heads)
        self.W = {k: weights[k][0].detach().cpu().to(F64).clone() for k, *_ in self.heads}
        self.b = {k: weights[k][1].detach().cpu().to(F64).clone() for k, *_ in self.heads}
        self.mW = {k: torch.zeros_like(v) for k, v in self.W.items()}
        self.mb = {k: torch.zeros_like(v) for k, v in self.b.items()}
        self.steps = 0

    def logits(self, x_all, hw, B, key, n):
        x = x_all.detach().cpu().to(F64)[:, (self.n_max - n) * self.Dc:]
        return x, (x @ self.W[key].T + self.b[key]).view(B, hw[0], hw[1], -1)

    def forward(self, x_all, hw, gt):
        """key -> loss_and_grad of the head at its current weights"""
        gt = gt.detach().cpu()
        return {k: loss_and_grad(self.logits(x_all, hw, gt.shape[0], k, n)[1], gt, self.lo, self.hi, self.lam) for k, n, _ in self.heads}

    def step(self, x_all, hw, gt):
        """one optimizer step of every head; returns key -> loss_and_grad dict (before the step)"""
        gt = gt.detach().cpu()
        out = {}
        for k, n, base in self.heads:
            x, z = self.logits(x_all, hw, gt.shape[0], k, n)
            r = loss_and_grad(z, gt, self.lo, self.hi, self.lam)
            sgd_step(self.W[k], self.b[k], self.mW[k], self.mb[k], r["G"].reshape(x.shape[0], -1), x,
                     cosine_lr(base, self.steps, self.max_iter), self.momentum)
            out[k] = r
        self.steps += 1
        return out


# (B, h, w, Hl, Wl, C, K): the smallest shapes at which each kernel can still go wrong; case i is drawn from seed 300 + i
CASES = [(1, 1, 1, 5, 7, 2, 40),         # every tap clamps, two bins
         (3, 2, 3, 32, 48, 64, 132),     # one full 64-bin chunk
         (2, 5, 4, 37, 23, 65, 260),     # a chunk boundary crossed by one bin, non-integer scale
         (2, 5, 4, 3, 2, 256, 40),       # downsampling
         (1, 4, 4, 4, 4, 256, 132),      # scale 1: the identity
         (2, 3, 5, 48, 80, 256, 132),    # the largest case
         (1, 7, 6, 2, 2, 5, 40),         # strong downsampling: cells with empty support
         (1, 8, 8, 8, 8, 256, 40)]       # 8 x 8 x 257 floats of cells do not fit the LDS budget: seg_plan ends at 4 x 4-pixel tiles, 2 x 2
VARIANTS = (None, "all_invalid", "nan", "inf", "far")


def make_case(i, H, variant=None):
    """X ~ N(0, 1) [B h w, K], W ~ 0.3 N(0, 1) [H C, K], b ~ N(0, 1) [H C], gt f32 [B, Hl, Wl] = min + (max - min) rand with about 10 % set
    to 0 (invalid).  variant: "all_invalid" (every label 0), or one planted label at a pixel that was valid: "nan", "inf", "far"
    (1.5 max_depth)"""
    B, h, w, Hl, Wl, C, K = CASES[i]
    g = torch.Generator().manual_seed(300 + i)
    X = torch.randn(B * h * w, K, generator=g)
    W = 0.3 * torch.randn(H * C, K, generator=g)
    b = torch.randn(H * C, generator=g)
    gt = MIN_DEPTH + (MAX_DEPTH - MIN_DEPTH) * torch.rand(B, Hl, Wl, generator=g)
    r = torch.rand(B, Hl, Wl, generator=g)
    gt[r < 0.10] = 0.0
    if variant == "all_invalid":
        gt.fill_(0.0)
    elif variant is not None:
        at = tuple(int(v) for v in (gt > 0).nonzero()[-1])  # the last valid pixel
        gt[at] = {"nan": float("nan"), "inf": float("inf"), "far": 1.5 * MAX_DEPTH}[variant]
    return X, W, b, gt
