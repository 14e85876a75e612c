"""Linear monocular-depth probe on frozen patch tokens: one linear layer per head whose outputs are `n_bins` uniform bins of depth
over [min_depth, max_depth], its low-resolution logit map upsampled bilinearly to the label map, AdaBins' "linear normalisation"
(a_c = max(z_c, 0) + 0.1, depth = sum_c a_c e_c / sum_c a_c) and the scale-invariant log loss of Eigen et al. -- the "lin." depth
evaluation the DINOv2 / DINOv3 papers report beside k-NN, linear classification and linear segmentation, restated from the papers'
description.  Parity with the DINOv2 depth code or the Monocular-Depth-Estimation-Toolbox is UNPINNED, and three things differ from
those programs: they put a BatchNorm in front of the linear layer (none here); they upsample the features x 4 and resize the
predicted depth (here the logits are interpolated straight to the label size and normalised there); they train with AdamW (here it
is the probes' SGD + cosine).  The arithmetic is pinned by an fp64 restatement checked against torch's own CPU ops
(tests/depth_ref.py).

Per feature group: ONE exact-fp32 logits GEMM over all heads at the low resolution (vtp_probe_logits), ONE pixel pass that
interpolates each pixel's logits from LDS-staged cells (depth, log residual, fp64 loss statistics), ONE gather pass for the gradient
of the low-resolution logits and ONE sliced weight-gradient + SGD-momentum step (csrc/depthprobe.hip; the weight step is
SegProbe's).  Nothing of size [B, n_bins, Hl, Wl] exists and nothing is summed with atomics: a step repeats bit for bit.

    probe = DepthProbe(model, [("depth_1_lr_0_01", 1, 0.01), ("depth_4_lr_0_01", 4, 0.01)], max_iter=iters)
    losses = probe.step(images, depth)             # device f32 [heads]; depth f32 [B, Hl, Wl] in metres, 0 = no measurement
    probe.evaluate(images, depth); probe.metrics(); probe.best()
    pred = probe.predict(images, (Ho, Wo))         # f32 [heads, B, Ho, Wo]

A pixel counts iff 0 < depth <= max_depth (NaN and inf do not): crops (Eigen, Garg) are the caller's, who zeroes the pixels outside.
There is no CPU path: tensors on the CPU raise.  Training is single-process; evaluation sums its counters over a process group."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .banks import Workspace
from .denseprobe import SGD_WORKSPACE_BOUND, DenseProbe, Head  # noqa: F401 (re-exported)
from .heads import cosine_factor

METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "silog", "d1", "d2", "d3", "valid")


def metrics_from_counters(counts: torch.Tensor, sums: torch.Tensor) -> Dict[str, float]:
    """counts int64 [4] = (valid, d1, d2, d3 hits), sums fp64 [6] = sums over the valid pixels of (g, g^2, |d - gt| / gt,
    (d - gt)^2 / gt, (d - gt)^2, |g| / ln 10) with g = log d - log gt -> the metrics, in fp64 on the host"""
    n = int(counts[0])
    if n == 0:
        raise RuntimeError("nothing evaluated yet (no valid pixel)")
    s = [float(v) / n for v in sums.tolist()]
    return {"abs_rel": s[2], "sq_rel": s[3], "rmse": math.sqrt(s[4]), "rmse_log": math.sqrt(s[1]), "log10": s[5],
            "silog": 100.0 * math.sqrt(max(s[1] - s[0] * s[0], 0.0)), "d1": int(counts[1]) / n, "d2": int(counts[2]) / n,
            "d3": int(counts[3]) / n, "valid": n}


class DepthProbe(DenseProbe):
    """heads: (key, use_n_blocks, lr) tuples with unique keys, grouped and stored as denseprobe.DenseProbe describes (C = n_bins).
    cls_concat appends each block's class token to every one of its patch tokens (K = 2 D per block).  model may be None when only
    the *_features methods are used (then pass embed_dim)."""

    _COLS = "n_max Dc"
    _sgd = staticmethod(ops.depth_sgd)
    _sgd_workspace_bytes = staticmethod(ops.depth_sgd_workspace_bytes)

    def __init__(self, model, heads: Sequence[Head], min_depth: float = 0.001, max_depth: float = 10.0, n_bins: int = 256,
                 lam: float = 0.85, momentum: float = 0.9, max_iter: Optional[int] = None, group=None, *, cls_concat: bool = False,
                 embed_dim: Optional[int] = None, device=None):
        if not 2 <= int(n_bins) <= 1024:
            raise ValueError(f"n_bins must be in [2, 1024], got {n_bins}")
        if not 0.0 < float(min_depth) < float(max_depth) < math.inf:
            raise ValueError(f"need 0 < min_depth < max_depth, got {min_depth}, {max_depth}")
        super().__init__(model, heads, n_bins, momentum, max_iter, group, cls_concat, embed_dim, device)
        self.min_depth, self.max_depth, self.lam = float(min_depth), float(max_depth), float(lam)
        self._ws_pix, self._ws_aux = Workspace(self.device), Workspace(self.device)
        self._stats = torch.zeros(len(self.keys), 4, device=self.device, dtype=torch.float64)  # (n, m1, m2, L) of the last call
        self._counts = torch.zeros(len(self.keys), 4, device=self.device, dtype=torch.int64)
        self._sums = torch.zeros(len(self.keys), 6, device=self.device, dtype=torch.float64)

    def _labels(self, labels: torch.Tensor) -> torch.Tensor:
        if not labels.is_floating_point() or labels.dim() != 3 or min(labels.shape) < 1:
            raise ValueError(f"labels must be floating-point depth [B, Hl, Wl], got {labels.dtype} {tuple(labels.shape)}")
        return labels.detach().to(torch.float32).contiguous()

    def _range(self):
        return self.min_depth, self.max_depth, self.lam

    # ------------------------------------------------------------------------------------------------ training
    def step_features(self, x_all: torch.Tensor, hw, labels: torch.Tensor) -> torch.Tensor:
        """one optimizer step of every head on X_all [B h w, n_max Dc] and labels [B, Hl, Wl]; returns the per-head losses (device
        f32, order of `keys`, no host sync).  Without a valid pixel the loss and the gradient are 0 and the momentum still decays."""
        self._single_process()
        x, (h, w), y = self._inputs(x_all, hw, labels)
        B, Hl, Wl = y.shape
        M, C = B * h * w, self.C
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        f = cosine_factor(self.steps, self.max_iter)
        for g in self.groups:
            self.heads.set_lr(g, f)
            z = self._logits(g, x, M)
            grad = torch.empty(M, g.H * C, device=self.device, dtype=torch.float32)
            ws = self._ws_pix.at_least(ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, g.H, C))
            aux = self._ws_aux.at_least(ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, g.H, C, aux=True))
            stats = self._stats[g.off:g.off + g.H]
            ops.depth_pix(z, y, (h, w), g.H, C, *self._range(), aux=aux, loss=losses[g.off:g.off + g.H], stats=stats, workspace=ws)
            ops.depth_dlogits(z, (B, Hl, Wl), (h, w), g.H, C, *self._range(), aux, stats, grad)
            self._weight_step(g, grad, x[:, g.col0:g.col0 + g.K], M)
        self.steps += 1
        return losses

    # ------------------------------------------------------------------------------------------------ evaluation
    def evaluate_features(self, x_all: torch.Tensor, hw, labels: torch.Tensor) -> torch.Tensor:
        """adds this batch to the evaluation counters (depth predicted at the labels' own size, invalid pixels skipped); returns its
        per-head losses (device f32, no host sync)"""
        x, (h, w), y = self._inputs(x_all, hw, labels)
        B, Hl, Wl = y.shape
        M, C = B * h * w, self.C
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        for g in self.groups:
            ws = self._ws_pix.at_least(ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, g.H, C))
            ops.depth_pix(self._logits(g, x, M), y, (h, w), g.H, C, *self._range(), loss=losses[g.off:g.off + g.H],
                          stats=self._stats[g.off:g.off + g.H], workspace=ws, eval_counts=self._counts[g.off:g.off + g.H],
                          eval_sums=self._sums[g.off:g.off + g.H])
        return losses

    def predict(self, images: torch.Tensor, out_hw) -> torch.Tensor:
        return self.predict_features(self.features(images), self._hw(images), out_hw)

    def predict_features(self, x_all: torch.Tensor, hw, out_hw) -> torch.Tensor:
        """f32 [heads, B, Ho, Wo]: the depth of every head (order of `keys`) at out_hw = (Ho, Wo), in [min_depth, max_depth]"""
        self._on_device(features=x_all)
        h, w = int(hw[0]), int(hw[1])
        Ho, Wo = int(out_hw[0]), int(out_hw[1])
        if h < 1 or w < 1 or Ho < 1 or Wo < 1 or x_all.dim() != 2 or x_all.shape[0] % (h * w):
            raise ValueError(f"features must be [B h w, n_max Dc] and out_hw >= 1, got {tuple(x_all.shape)}, hw {hw}, out_hw {out_hw}")
        B = x_all.shape[0] // (h * w)
        x, _ = self._features(x_all, (h, w), B)
        out = torch.empty(len(self.keys), B, Ho, Wo, device=self.device, dtype=torch.float32)
        for g in self.groups:
            ops.depth_pix(self._logits(g, x, B * h * w), None, (h, w), g.H, self.C, *self._range(), out_hw=(Ho, Wo),
                          dhat=out[g.off:g.off + g.H])
        return out

    def counters(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(int64 [heads, 4], fp64 [heads, 6]) on the host, summed over the process group with one all-reduce (the counts travel as
        fp64: exact below 2^53 pixels)"""
        nh = len(self.keys)
        flat = self._group.summed(torch.cat([self._counts.to(torch.float64).reshape(-1), self._sums.reshape(-1)])).cpu()
        return flat[:4 * nh].view(nh, 4).to(torch.int64), flat[4 * nh:].view(nh, 6)

    def metrics(self) -> Dict[str, Dict[str, float]]:
        """key -> {abs_rel, sq_rel, rmse, rmse_log, log10, silog (= 100 sqrt(m2 - m1^2) over everything evaluated), d1, d2, d3, valid}"""
        counts, sums = self.counters()
        return {k: metrics_from_counters(counts[i], sums[i]) for i, k in enumerate(self.keys)}

    def best(self) -> Tuple[str, float]:
        """the head with the lowest rmse"""
        m = {k: v["rmse"] for k, v in self.metrics().items()}
        key = min(m, key=m.get)
        return key, m[key]

    def reset_eval(self) -> None:
        self._counts.zero_()
        self._sums.zero_()
