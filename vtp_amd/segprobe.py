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
from .banks import Group, Workspace, eval_device
from .heads import HeadGroup, HeadStore, cosine_factor

Head = Tuple[str, int, float]  # (key, use_n_blocks, lr)
SGD_WORKSPACE_BOUND = 64 << 20  # bytes of weight-gradient slices per launch; a group whose heads need more is stepped in chunks of heads


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


class SegProbe:
    """heads: (key, use_n_blocks, lr) tuples with unique keys; heads with equal use_n_blocks form a group and are stored stacked
    (heads.HeadStore: weight [H, C, K], bias [H, C] and their momentum buffers, contiguous fp32; normal_(0, 0.01) weights and zero
    biases drawn on the host in creation order).  `keys` lists the heads group by group: the order of every per-head vector.  model
    may be None when only step_features / evaluate_features are used (then pass embed_dim)."""

    def __init__(self, model, heads: Sequence[Head], num_classes: int, ignore_index: int = 255, momentum: float = 0.9,
                 max_iter: Optional[int] = None, group=None, *, embed_dim: Optional[int] = None, device=None):
        self.device = eval_device("SegProbe", model, device)
        self.model = model
        self.D = int(embed_dim if embed_dim is not None else model.config.vision_embed_dim)
        if self.D % 4:
            raise ValueError(f"embed_dim must be a multiple of 4 (16-byte column slices), got {self.D}")
        if not 1 <= int(num_classes) <= 255:
            raise ValueError(f"num_classes must be in [1, 255] (labels are bytes), got {num_classes}")
        if max_iter is not None and max_iter < 1:
            raise ValueError("max_iter must be >= 1 (or None for constant learning rates)")
        self.C, self.ignore_index, self.momentum, self.max_iter = int(num_classes), int(ignore_index), float(momentum), max_iter
        self.group = group
        self._group = Group(group)
        self.world, self.rank = self._group.world, self._group.rank
        heads = [(str(k), int(n), float(lr)) for k, n, lr in heads]
        if not heads:
            raise ValueError("no heads")
        if len({k for k, _, _ in heads}) != len(heads):
            raise ValueError("head keys must be unique")
        self.n_max = max(n for _, n, _ in heads)
        init = {}
        for key, n, _ in heads:
            if n < 1:
                raise ValueError(f"{key}: use_n_blocks must be >= 1")
            init[key] = (torch.empty(self.C, n * self.D).normal_(mean=0.0, std=0.01), torch.zeros(self.C))
        # a group reads the last n blocks: the trailing n D columns of X_all
        self.heads = HeadStore([(key, n, n * self.D, (self.n_max - n) * self.D, lr) for key, n, lr in heads], init, self.device, max_iter)
        del init
        self.groups, self.keys = self.heads.groups, self.heads.keys
        self.steps = 0
        self.head_chunk: Optional[int] = None  # heads per weight-step launch; None: as many as SGD_WORKSPACE_BOUND allows
        self._ws_ce, self._ws_sgd = Workspace(self.device), Workspace(self.device)
        self._call_counts = torch.zeros(2, device=self.device, dtype=torch.int32)
        self._conf = torch.zeros(len(self.keys), self.C, self.C, device=self.device, dtype=torch.int64)
        self._totals = torch.zeros(2, device=self.device, dtype=torch.int64)  # valid pixels, out-of-range labels

    # ------------------------------------------------------------------------------------------------ inputs
    def features(self, images: torch.Tensor) -> torch.Tensor:
        """X_all f32 [B h w, n_max D] with (h, w) = the image size over the patch size 16: the patch tokens (no class token) of the
        last n_max blocks, each through the trunk's final norm, concatenated in ascending block order; in exact fp32 where the
        model's enable_fp32_forward covers the trunk"""
        if self.model is None:
            raise RuntimeError("SegProbe was built without a model: use step_features / evaluate_features")
        outs = self.model.get_intermediate_layers_feature(images, n=self.n_max, norm=True)
        B, T, D = outs[0].shape
        return torch.cat([o.reshape(B * T, D) for o in outs], dim=1)

    @staticmethod
    def _hw(images: torch.Tensor) -> Tuple[int, int]:
        return images.shape[-2] // 16, images.shape[-1] // 16

    def _inputs(self, x_all: torch.Tensor, hw, labels: torch.Tensor):
        for name, t in (("features", x_all), ("labels", labels)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"{name} must live on the MI355X (got a CPU tensor): there is no CPU path")
        h, w = int(hw[0]), int(hw[1])
        if labels.is_floating_point() or labels.dtype == torch.bool or labels.dim() != 3 or min(labels.shape) < 1:
            raise ValueError(f"labels must be integers [B, Hl, Wl], got {labels.dtype} {tuple(labels.shape)}")
        B = labels.shape[0]
        x = x_all.detach().to(torch.float32)
        if x.dim() != 2 or h < 1 or w < 1 or tuple(x.shape) != (B * h * w, self.n_max * self.D):
            raise ValueError(f"features must be [B h w, n_max D] = [{B * h * w}, {self.n_max * self.D}], got {tuple(x_all.shape)}")
        if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
            x = x.contiguous()
        y = labels.detach()
        if y.dtype != torch.uint8:  # on the device, no host sync: anything a byte cannot hold is no class
            y = torch.where((y < 0) | (y > 255), torch.full_like(y, 255), y).to(torch.uint8)
        return x, (h, w), y.contiguous()

    def _head_chunk(self, g: HeadGroup, M: int) -> int:
        if self.head_chunk is not None:
            return max(1, min(g.H, int(self.head_chunk)))
        per_head = ops.seg_sgd_workspace_bytes(M, self.C, g.K)
        return max(1, min(g.H, SGD_WORKSPACE_BOUND // per_head))

    # ------------------------------------------------------------------------------------------------ training
    def learning_rates(self, step: Optional[int] = None) -> Dict[str, float]:
        return self.heads.learning_rates(self.steps if step is None else step)

    def step(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self.step_features(self.features(images), self._hw(images), labels)

    def step_features(self, x_all: torch.Tensor, hw, labels: torch.Tensor) -> torch.Tensor:
        """one optimizer step of every head on X_all [B h w, n_max D] and labels [B, Hl, Wl]; returns the per-head losses (device
        f32, order of `keys`, no host sync).  Without a valid pixel the loss and the gradient are 0 and the momentum still decays."""
        if self.world > 1:
            raise NotImplementedError("Training is single-process in this pull request.")
        x, (h, w), y = self._inputs(x_all, hw, labels)
        B, Hl, Wl = y.shape
        M, C = B * h * w, self.C
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        f = cosine_factor(self.steps, self.max_iter)
        f32 = dict(device=self.device, dtype=torch.float32)
        for g in self.groups:
            N = g.H * C
            self.heads.set_lr(g, f)
            xs = x[:, g.col0:g.col0 + g.K]
            z, grad = torch.empty(M, N, **f32), torch.empty(M, N, **f32)
            lse = torch.empty(g.H, B, Hl, Wl, **f32)
            ops.probe_logits(xs, g.weight, g.bias, z, M, N, g.K)
            ws = self._ws_ce.at_least(ops.seg_ce_workspace_bytes(B, h, w, Hl, Wl, g.H, C))
            ops.seg_ce(z, y, (h, w), g.H, C, self.ignore_index, losses[g.off:g.off + g.H], self._call_counts, ws, lse=lse)
            ops.seg_dlogits(z, y, (h, w), g.H, C, self.ignore_index, lse, self._call_counts, grad)
            step = self._head_chunk(g, M)
            for lo in range(0, g.H, step):  # the chunking bounds the workspace and changes no bit of the result
                n = min(step, g.H - lo)
                ws = self._ws_sgd.at_least(ops.seg_sgd_workspace_bytes(M, n * C, g.K))
                ops.seg_sgd(g.weight[lo:lo + n], g.bias[lo:lo + n], g.m_weight[lo:lo + n], g.m_bias[lo:lo + n], grad[:, lo * C:], xs,
                            g.lr[lo:lo + n], M, n, C, g.K, self.momentum, ws)
        self.steps += 1
        return losses

    # ------------------------------------------------------------------------------------------------ evaluation
    def evaluate(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self.evaluate_features(self.features(images), self._hw(images), labels)

    def evaluate_features(self, x_all: torch.Tensor, hw, labels: torch.Tensor) -> torch.Tensor:
        """adds this batch to the confusion matrices (logits upsampled to the labels' own size, lowest index on ties, ignored pixels
        skipped); returns its per-head mean losses (device f32, no host sync)"""
        x, (h, w), y = self._inputs(x_all, hw, labels)
        B, Hl, Wl = y.shape
        M, C = B * h * w, self.C
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        for i, g in enumerate(self.groups):
            z = torch.empty(M, g.H * C, device=self.device, dtype=torch.float32)
            ops.probe_logits(x[:, g.col0:g.col0 + g.K], g.weight, g.bias, z, M, g.H * C, g.K)
            ws = self._ws_ce.at_least(ops.seg_ce_workspace_bytes(B, h, w, Hl, Wl, g.H, C))
            ops.seg_ce(z, y, (h, w), g.H, C, self.ignore_index, losses[g.off:g.off + g.H], self._call_counts, ws,
                       conf=self._conf[g.off:g.off + g.H], totals=self._totals if i == 0 else None)
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

    # ------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {**{name: t.clone() for name, t in self._named()}, "steps": torch.tensor(self.steps, dtype=torch.int64)}

    def _named(self):
        """(checkpoint key, tensor view) per head: heads.<key>.weight, heads.<key>.bias, momentum.<key>.weight, momentum.<key>.bias"""
        entries = list(self.heads.entries())
        for (k, _, w, mw), (_, _, b, mb) in zip(entries[0::2], entries[1::2]):  # a head's weight entry, then its bias entry
            yield from ((f"heads.{k}.weight", w), (f"heads.{k}.bias", b), (f"momentum.{k}.weight", mw), (f"momentum.{k}.bias", mb))

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        want = {f"{p}.{k}.{q}" for k in self.keys for p in ("heads", "momentum") for q in ("weight", "bias")} | {"steps"}
        if want != set(sd):
            raise KeyError(f"load_state_dict: missing {sorted(want - set(sd))}, unexpected {sorted(set(sd) - want)}")
        for name, dst in self._named():
            if sd[name].shape != dst.shape:
                raise ValueError(f"{name}: shape {tuple(sd[name].shape)}, expected {tuple(dst.shape)}")
            dst.copy_(sd[name])
        self.steps = int(sd["steps"])
