"""Helper of the segmentation-probe tests (not a test): an fp64 torch restatement of the linear segmentation probe -- bilinear taps
and weights (ATen's upsample_bilinear2d with align_corners=False, by its formula), upsampled logits, mean per-pixel cross-entropy
over the valid pixels, the gradient with respect to the low-resolution logits as the explicit sum over pixels, the confusion
matrix, mIoU and one SGD-with-momentum step.  tests/test_segprobe_host.py pins it to torch's own CPU ops (F.interpolate,
F.cross_entropy, autograd); tests/test_segprobe_gpu.py checks the kernels (csrc/segprobe.hip) against it."""
import math

import torch

F64 = torch.float64
IGNORE = 255


def gamma(n):
    """a-priori relative bound of n fp32 roundings in a chain: n u / (1 - n u), u = 2^-24"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def taps(out, inn):
    """(i0, i1 int64 [out], l0, l1 fp64 [out]) of an axis resampled from inn to out entries: scale = inn / out,
    src = max(scale (dst + 0.5) - 0.5, 0), i0 = floor(src), i1 = i0 + (i0 < inn - 1), l1 = src - i0, l0 = 1 - l1"""
    dst = torch.arange(out, dtype=F64)
    src = ((inn / out) * (dst + 0.5) - 0.5).clamp_min(0.0)
    i0 = src.floor().long()
    i1 = i0 + (i0 < inn - 1).long()
    l1 = src - i0.to(F64)
    return i0, i1, 1.0 - l1, l1


def tap_matrix(out, inn):
    """A fp64 [out, inn]: row dst holds l0 at i0 and l1 at i1 (added where the two coincide)"""
    i0, i1, l0, l1 = taps(out, inn)
    A = torch.zeros(out, inn, dtype=F64)
    r = torch.arange(out)
    A.index_put_((r, i0), l0, accumulate=True)
    A.index_put_((r, i1), l1, accumulate=True)
    return A


def upsample(z, Hl, Wl):
    """z [B, h, w, C] -> [B, Hl, Wl, C]: value = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11)"""
    z = z.to(F64)
    y0, y1, ly0, ly1 = taps(Hl, z.shape[1])
    x0, x1, lx0, lx1 = taps(Wl, z.shape[2])
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    top = lx0 * z[:, y0][:, :, x0] + lx1 * z[:, y0][:, :, x1]
    bot = lx0 * z[:, y1][:, :, x0] + lx1 * z[:, y1][:, :, x1]
    return ly0[None, :, None, None] * top + ly1[None, :, None, None] * bot


def valid_mask(labels, C, ignore=IGNORE):
    """(valid, out_of_range) bool [B, Hl, Wl]: a label equal to ignore is skipped; a label >= C that is not ignore is skipped too
    and counted"""
    labels = labels.long()
    return (labels != ignore) & (labels < C), (labels != ignore) & (labels >= C)


def loss_and_grad(z, labels, ignore=IGNORE):
    """z [B, h, w, C] (any float dtype, taken to fp64), labels integer [B, Hl, Wl] -> dict with
    up [B, Hl, Wl, C], lse [B, Hl, Wl], loss (mean of lse - z[y] over the valid pixels; 0 without one), n_valid, out_of_range and
    G [B, h, w, C] = (1 / n_valid) sum over the valid pixels p of w_p(i, j) (softmax(p) - onehot(y_p)): the explicit sum, the
    weight of cell (i, j) in pixel p being the product of the axis weights of tap_matrix"""
    z = z.to(F64)
    B, h, w, C = z.shape
    Hl, Wl = labels.shape[1:]
    up = upsample(z, Hl, Wl)
    lse = torch.logsumexp(up, dim=-1)
    ok, oor = valid_mask(labels, C, ignore)
    n = int(ok.sum())
    y = torch.where(ok, labels.long(), torch.zeros_like(labels.long()))
    zy = up.gather(-1, y[..., None])[..., 0]
    loss = float(((lse - zy) * ok).sum() / n) if n else 0.0
    d = torch.exp(up - lse[..., None])
    d.scatter_add_(-1, y[..., None], -torch.ones_like(zy)[..., None])
    d = d * ok[..., None]
    G = torch.einsum("yi,xj,byxc->bijc", tap_matrix(Hl, h), tap_matrix(Wl, w), d) / max(n, 1)
    return dict(up=up, lse=lse, loss=loss, n_valid=n, out_of_range=int(oor.sum()), G=G, valid=ok)


def confusion(up, labels, keep=None, ignore=IGNORE):
    """int64 [C, C], row = target, column = argmax of up [B, Hl, Wl, C] (the lowest index on ties); ignored pixels skipped, and
    those outside the bool mask `keep` where one is given"""
    C = up.shape[-1]
    ok, _ = valid_mask(labels, C, ignore)
    if keep is not None:
        ok = ok & keep
    pred = up.argmax(dim=-1)
    idx = labels.long()[ok] * C + pred[ok]
    return torch.bincount(idx, minlength=C * C).view(C, C)


def miou(conf):
    """(mIoU, per-class IoU fp64 [C] with NaN for a class absent from targets and predictions, pixel accuracy) of an int64 [C, C]
    confusion matrix; the mean runs over the classes with TP + FP + FN > 0"""
    conf = conf.to(F64)
    tp = conf.diag()
    union = conf.sum(0) + conf.sum(1) - tp
    iou = torch.full_like(tp, float("nan"))
    seen = union > 0
    iou[seen] = tp[seen] / union[seen]
    return (float(iou[seen].mean()) if bool(seen.any()) else float("nan")), iou, float(tp.sum() / conf.sum())


def sgd_step(W, b, mW, mb, G, X, lr, momentum):
    """one torch.optim.SGD(momentum, dampening 0, no weight decay) step in place from G [M, C] and X [M, K] (fp64)"""
    for p, m, g in ((W, mW, G.T @ X), (b, mb, G.sum(0))):
        m.mul_(momentum).add_(g)
        p.sub_(lr * m)


def cosine_lr(base, step, max_iter):
    return base if max_iter is None else base * 0.5 * (1.0 + math.cos(math.pi * step / max_iter))


class RefSeg:
    """heads: [(key, n_blocks, lr)]; weights: key -> (W [C, n D], b [C]).  X_all [B h w, n_max D]: a head reads its trailing n D columns."""

    def __init__(self, heads, weights, D, momentum=0.9, max_iter=None, ignore=IGNORE):
        self.heads, self.D, self.momentum, self.max_iter, self.ignore = list(heads), D, momentum, max_iter, ignore
        self.n_max = max(h[1] for h in self.heads)
        self.W = {k: weights[k][0].detach().cpu().to(F64).clone() for k, *_ in self.heads}
        self.b = {k: weights[k][1].detach().cpu().to(F64).clone() for k, *_ in self.heads}
        self.mW = {k: torch.zeros_like(v) for k, v in self.W.items()}
        self.mb = {k: torch.zeros_like(v) for k, v in self.b.items()}
        self.steps = 0

    def logits(self, x_all, hw, B, key, n):
        x = x_all.detach().cpu().to(F64)[:, (self.n_max - n) * self.D:]
        return x, (x @ self.W[key].T + self.b[key]).view(B, hw[0], hw[1], -1)

    def step(self, x_all, hw, labels):
        """one optimizer step of every head; returns key -> loss (before the step)"""
        labels = labels.detach().cpu()
        out = {}
        for k, n, base in self.heads:
            x, z = self.logits(x_all, hw, labels.shape[0], k, n)
            r = loss_and_grad(z, labels, self.ignore)
            sgd_step(self.W[k], self.b[k], self.mW[k], self.mb[k], r["G"].reshape(x.shape[0], -1), x,
                     cosine_lr(base, self.steps, self.max_iter), self.momentum)
            out[k] = r["loss"]
        self.steps += 1
        return out


# (B, h, w, Hl, Wl, C, K): the smallest shapes at which each kernel can still go wrong; case i is drawn from seed 100 + i
CASES = [(1, 1, 1, 5, 7, 2, 40),         # every tap clamps
         (3, 2, 3, 32, 48, 21, 132),     # integer scale 16
         (2, 5, 4, 37, 23, 150, 260),    # non-integer, non-square
         (2, 5, 4, 3, 2, 21, 40),        # downsampling
         (1, 4, 4, 4, 4, 150, 132),      # scale 1: the identity
         (2, 3, 5, 48, 80, 150, 260),
         (1, 7, 6, 2, 2, 5, 40),         # strong downsampling: cells with empty support
         (1, 9, 9, 9, 9, 150, 40)]       # 9 x 9 x 151 floats of cells do not fit the LDS budget: seg_plan shrinks th to 4 (tw stays 32), 3 x 1 tiles


def make_case(i, H, all_ignored=False):
    """X ~ N(0, 1) [B h w, K], W ~ 0.3 N(0, 1) [H C, K], b ~ N(0, 1) [H C], labels uint8 [B, Hl, Wl] uniform in [0, C) with about
    10 % set to 255 (ignored) and about 2 % to C (out of range); all_ignored: every label 255"""
    B, h, w, Hl, Wl, C, K = CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    X = torch.randn(B * h * w, K, generator=g)
    W = 0.3 * torch.randn(H * C, K, generator=g)
    b = torch.randn(H * C, generator=g)
    labels = torch.randint(0, C, (B, Hl, Wl), generator=g)
    r = torch.rand(B, Hl, Wl, generator=g)
    labels[r < 0.10] = IGNORE
    labels[(r >= 0.10) & (r < 0.12)] = C
    if all_ignored:
        labels.fill_(IGNORE)
    return X, W, b, labels.to(torch.uint8)
