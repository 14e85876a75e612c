"""Linear segmentation probe on frozen patch tokens: one linear layer per head on the patch tokens of the last trunk blocks, its
low-resolution logit map upsampled bilinearly to the label map, per-pixel cross-entropy, mIoU -- the dense evaluation the DINOv2
and iBOT papers report beside linear probing and k-NN, restated from the papers' description.  Parity with mmsegmentation or the
DINOv2 segmentation code is UNPINNED (they train with AdamW + poly; this is LinearProbe's SGD + cosine); the arithmetic is pinned
by an fp64 restatement checked against torch's own CPU ops (tests/seg_ref.py).

Per feature group: ONE exact-fp32 logits GEMM over all heads at the low resolution (vtp_probe_logits, M = B h w rows), ONE pixel
pass that interpolates each pixel's logits from LDS-staged cells (loss, lse, confusion counts), ONE gather pass for the gradient of
the low-resolution logits and ONE sliced weight-gradient + SGD-momentum step (csrc/segprobe.hip).  Nothing of size [B, C, Hl, Wl]
exists, no float is summed with atomics: a step repeats bit for bit.

    probe = SegProbe(model, [("seg_1_lr_0_01", 1, 0.01), ("seg_4_lr_0_01", 4, 0.01)], num_classes=150, max_iter=iters)
    losses = probe.step(images, labels)            # device f32 [heads]; labels [B, Hl, Wl] integers, 255 = ignore
    probe.evaluate(images, labels); probe.miou(); probe.best()

There is no CPU path: tensors on the CPU raise.  Training is single-process; evaluation sums its counters over a process group."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .banks import Workspace
from .denseprobe import SGD_WORKSPACE_BOUND, DenseProbe, Head  # noqa: F401 (re-exported)
from .heads import cosine_factor


def miou_from_confusion(conf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """conf int64 [..., C, C] (row = target, column = prediction) -> (mIoU [...], per-class IoU [..., C], pixel accuracy [...]) in
    fp64.  A class with TP + FP + FN == 0 has IoU NaN and is left out of the mean; without any class the mean is NaN."""
    conf = conf.to(torch.float64)
    tp = conf.diagonal(dim1=-2, dim2=-1)
    union = conf.sum(-1) + conf.sum(-2) - tp
    iou = torch.where(union > 0, tp / union.clamp_min(1.0), torch.full_like(tp, float("nan")))
    seen = (union > 0).sum(-1)
    miou = torch.where(seen > 0, torch.nan_to_num(iou).sum(-1) / seen.clamp_min(1), torch.full_like(iou[..., 0], float("nan")))
    total = conf.sum((-1, -2))
    acc = torch.where(total > 0, tp.sum(-1) / total.clamp_min(1.0), torch.full_like(total, float("nan")))
    return miou, iou, acc


class SegProbe(DenseProbe):
    """heads: (key, use_n_blocks, lr) tuples with unique keys, grouped and stored as denseprobe.DenseProbe describes (C =
    num_classes).  model may be None when only step_features / evaluate_features are used (then pass embed_dim)."""

    _FEATURE_METHODS = "step_features / evaluate_features"

    def __init__(self, model, heads: Sequence[Head], num_classes: int, ignore_index: int = 255, momentum: float = 0.9,
                 max_iter: Optional[int] = None, group=None, *, embed_dim: Optional[int] = None, device=None):
        if not 1 <= int(num_classes) <= 255:
            raise ValueError(f"num_classes must be in [1, 255] (labels are bytes), got {num_classes}")
        super().__init__(model, heads, num_classes, momentum, max_iter, group, False, embed_dim, device)
        self.ignore_index = int(ignore_index)
        self._ws_ce = Workspace(self.device)
        self._call_counts = torch.zeros(2, device=self.device, dtype=torch.int32)
        self._conf = torch.zeros(len(self.keys), self.C, self.C, device=self.device, dtype=torch.int64)
        self._totals = torch.zeros(2, device=self.device, dtype=torch.int64)  # valid pixels, out-of-range labels

    def _labels(self, labels: torch.Tensor) -> torch.Tensor:
        if labels.is_floating_point() or labels.dtype == torch.bool or labels.dim() != 3 or min(labels.shape) < 1:
            raise ValueError(f"labels must be integers [B, Hl, Wl], got {labels.dtype} {tuple(labels.shape)}")
        y = labels.detach()
        if y.dtype != torch.uint8:  # on the device, no host sync: anything a byte cannot hold is no class
            y = torch.where((y < 0) | (y > 255), torch.full_like(y, 255), y).to(torch.uint8)
        return y.contiguous()

    def _ce(self, g, z, y, hw, losses, **out):
        B, Hl, Wl = y.shape
        ws = self._ws_ce.at_least(ops.seg_ce_workspace_bytes(B, *hw, Hl, Wl, g.H, self.C))
        ops.seg_ce(z, y, hw, g.H, self.C, self.ignore_index, losses[g.off:g.off + g.H], self._call_counts, ws, **out)

    # ------------------------------------------------------------------------------------------------ training
    def step_features(self, x_all: torch.Tensor, hw, labels: torch.Tensor) -> torch.Tensor:
        """one optimizer step of every head on X_all [B h w, n_max D] and labels [B, Hl, Wl] integers; returns the per-head losses
        (device f32, order of `keys`, no host sync).  Without a valid pixel the loss and the gradient are 0 and the momentum still
        decays."""
        self._single_process()
        x, (h, w), y = self._inputs(x_all, hw, labels)
        B, Hl, Wl = y.shape
        M = B * h * w
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        f = cosine_factor(self.steps, self.max_iter)
        for g in self.groups:
            self.heads.set_lr(g, f)
            z = self._logits(g, x, M)
            grad = torch.empty(M, g.H * self.C, device=self.device, dtype=torch.float32)
            lse = torch.empty(g.H, B, Hl, Wl, device=self.device, dtype=torch.float32)
            self._ce(g, z, y, (h, w), losses, lse=lse)
            ops.seg_dlogits(z, y, (h, w), g.H, self.C, self.ignore_index, lse, self._call_counts, grad)
            self._weight_step(g, grad, x[:, g.col0:g.col0 + g.K], M)
        self.steps += 1
        return losses

    # ------------------------------------------------------------------------------------------------ evaluation
    def evaluate_features(self, x_all: torch.Tensor, hw, labels: torch.Tensor) -> torch.Tensor:
        """adds this batch to the confusion matrices (logits upsampled to the labels' own size, lowest index on ties, ignored pixels
        skipped); returns its per-head mean losses (device f32, no host sync)"""
        x, (h, w), y = self._inputs(x_all, hw, labels)
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        for i, g in enumerate(self.groups):
            self._ce(g, self._logits(g, x, y.shape[0] * h * w), y, (h, w), losses, conf=self._conf[g.off:g.off + g.H],
                     totals=self._totals if i == 0 else None)
        return losses

    def counts(self) -> Dict[str, object]:
        """{"confusion": CPU int64 [heads, C, C] (row = target, column = prediction), "valid": pixels scored, "out_of_range": labels
        >= C that are not ignore_index (skipped; a non-zero count means a broken dataset)}, summed over the process group with one
        all-reduce"""
        flat = self._group.summed(torch.cat([self._conf.reshape(-1), self._totals])).cpu()
        return {"confusion": flat[:-2].view(len(self.keys), self.C, self.C), "valid": int(flat[-2]), "out_of_range": int(flat[-1])}

    def _scores(self):
        c = self.counts()
        if c["valid"] == 0:
            raise RuntimeError("nothing evaluated yet (no valid pixel)")
        return miou_from_confusion(c["confusion"])

    def miou(self) -> Dict[str, float]:
        """key -> the mean, over the classes with TP + FP + FN > 0, of TP / (TP + FP + FN), in percent"""
        return {k: 100.0 * float(v) for k, v in zip(self.keys, self._scores()[0])}

    def per_class_iou(self) -> Dict[str, torch.Tensor]:
        """key -> fp64 [C] IoU in percent; NaN for a class absent from targets and predictions alike"""
        return {k: 100.0 * v for k, v in zip(self.keys, self._scores()[1])}

    def pixel_accuracy(self) -> Dict[str, float]:
        return {k: 100.0 * float(v) for k, v in zip(self.keys, self._scores()[2])}

    def best(self) -> Tuple[str, float]:
        m = self.miou()
        key = max(m, key=m.get)
        return key, m[key]

    def reset_eval(self) -> None:
        self._conf.zero_()
        self._totals.zero_()
