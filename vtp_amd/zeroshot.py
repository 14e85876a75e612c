"""Zero-shot classification (reference: tools/test_zero_shot_hf.py) with the tool's own arithmetic on the project's kernels: the
classifier is built by ONE class-mean + normalise kernel per class batch, and a batch is scored by ONE launch that forms the
logits, ranks the target of every row and adds to the top-1 / top-5 counters on the device (csrc/zeroshot.hip) -- no reshape /
mean / F.normalize / cat / matmul / topk / eq / sum on torch, and no host synchronisation before the accuracy is asked for.

    zs = ZeroShot(model)
    zs.build_classifier(tokenizer, classnames, templates)              # build_zero_shot_classifier (:342-394)
    for images, targets in loader:
        zs.update(images.cuda(), targets.cuda())                      # the loop body of evaluate (:420-440)
    top1, top5 = zs.accuracy()                                        # percent, as the tool prints them

This is the tool's precision='fp32' arithmetic for the tool's own operations (template mean, normalisation, 100 * f @ classifier,
top-k), exact fp32 on the f32-input MFMA; the model's internals run as the project's kernels run them.  The reference's launcher
script passes bf16, which puts the classifier product in bf16 as well -- that is not imitated.  Ties are broken towards the
lower class index.  There is no CPU path: tensors on the CPU raise."""
from __future__ import annotations

from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import torch

from . import ops
from .banks import Group, aligned_f32, eval_device


def caption_batches(classnames: Sequence[str], templates: Sequence[Callable[[str], str]],
                    num_classes_per_batch: int = 10) -> Iterator[Tuple[int, List[str]]]:
    """(index of the batch's first class, texts) per class batch, texts = [template(c) for c in batch for template in templates]:
    the lists, order and batching that build_zero_shot_classifier hands its tokenizer (:302-309, :376-380).  Pure host code."""
    if num_classes_per_batch < 1:
        raise ValueError("num_classes_per_batch must be >= 1")
    if not templates:
        raise ValueError("no templates")
    names = list(classnames)
    for c0 in range(0, len(names), num_classes_per_batch):
        yield c0, [template(c) for c in names[c0:c0 + num_classes_per_batch] for template in templates]


def percent(hits: int, n: int) -> float:
    """count / n * 100, the expression of the tool (:441); nothing evaluated yet is an error, not a division by zero"""
    if n <= 0:
        raise RuntimeError("accuracy(): nothing evaluated yet")
    return hits / n * 100


class ZeroShot:
    """model: a vtp_amd.VTPModel with train_clip (None when the classifier and the features are given: set_classifier /
    update_features).  scale: the factor in front of the image features (100.0 in the tool).  group: a process group whose ranks
    each evaluate their own rows; counts() sums over it."""

    def __init__(self, model, group=None, scale: float = 100.0, device=None):
        self.device = eval_device("ZeroShot", model, device)
        self.model, self.group, self.scale = model, group, float(scale)
        self._group = Group(group)
        self.Wt: Optional[torch.Tensor] = None  # f32 [C, D], one row per class
        self._counts = torch.zeros(3, device=self.device, dtype=torch.int64)  # top-1 hits, top-5 hits, rows
        self._per_class: Optional[torch.Tensor] = None  # i32 [2, C]: rows seen, top-1 hits

    # ------------------------------------------------------------------------------------------------ classifier
    def _adopt(self, wt: torch.Tensor) -> torch.Tensor:
        C, D = wt.shape
        if C < 5:
            raise ValueError(f"zero-shot top-5 needs at least 5 classes, got {C}")
        self.Wt = wt
        self._per_class = torch.zeros(2, C, device=self.device, dtype=torch.int32)
        self._counts.zero_()
        return wt.T

    def build_classifier(self, tokenizer, classnames: Sequence[str], templates: Sequence[Callable[[str], str]],
                         num_classes_per_batch: int = 10) -> torch.Tensor:
        """build_zero_shot_classifier (:342-394): per class batch every template's caption through
        get_clip_text_feature(normalize=True), then mean over the templates and F.normalize written straight into the rows of
        the persistent [C, D] classifier.  Returns the tool's [D, C] classifier as a view of it.  Resets the counters."""
        if self.model is None:
            raise RuntimeError("ZeroShot was built without a model: use set_classifier")
        if self.model.config.text_pool_type == "none":
            raise RuntimeError("build_classifier needs pooled text features: text_pool_type = 'none' returns per-token features [B, T, D]")
        C, T = len(classnames), len(templates)
        wt = None
        with torch.no_grad():
            for c0, texts in caption_batches(classnames, templates, num_classes_per_batch):
                nb = len(texts) // T
                tokens = tokenizer(texts).to(self.device)
                feat = self.model.get_clip_text_feature(tokens, normalize=True).detach().to(torch.float32).contiguous()
                if feat.dim() != 2 or feat.shape[0] != nb * T:
                    raise ValueError(f"text features must be [{nb * T}, D], got {tuple(feat.shape)}")
                D = feat.shape[1]
                if D % 4:
                    raise ValueError(f"the CLIP feature width must be a multiple of 4, got {D}")
                if wt is None:
                    wt = torch.empty(C, D, device=self.device, dtype=torch.float32)
                ops.zs_class_mean(feat, wt[c0:c0 + nb], nb, T, D, 1e-12)
        if wt is None:
            raise ValueError("no classes")
        return self._adopt(wt)

    def set_classifier(self, classifier: torch.Tensor) -> torch.Tensor:
        """adopt a [D, C] classifier made elsewhere (the tool's layout; copied into [C, D]).  Resets the counters."""
        if classifier.dim() != 2 or classifier.shape[0] % 4:
            raise ValueError(f"classifier must be [D, C] with D a multiple of 4, got {tuple(classifier.shape)}")
        return self._adopt(classifier.detach().to(device=self.device, dtype=torch.float32).T.contiguous())

    @property
    def classifier(self) -> torch.Tensor:
        if self.Wt is None:
            raise RuntimeError("no classifier yet: build_classifier or set_classifier first")
        return self.Wt.T

    # ------------------------------------------------------------------------------------------------ evaluation
    def update(self, images: torch.Tensor, targets: torch.Tensor) -> None:
        if self.model is None:
            raise RuntimeError("ZeroShot was built without a model: use update_features")
        if not images.is_cuda:
            raise ValueError("images must live on the MI355X (got a CPU tensor): there is no CPU path")
        with torch.no_grad():
            feats = self.model.get_clip_image_feature(images.to(torch.float32), normalize=True)
        self.update_features(feats, targets)

    def update_features(self, feats: torch.Tensor, targets: torch.Tensor, logits_out: Optional[torch.Tensor] = None,
                        rank_out: Optional[torch.Tensor] = None, pred_out: Optional[torch.Tensor] = None) -> None:
        """adds one batch of image features f32 [B, D] to the counters: device only, no host synchronisation.  Optional outputs
        (all on the device): logits_out f32 [B, C], rank_out i32 [B] (the number of classes ranked before the target; C for a
        target outside [0, C)), pred_out i32 [B, 5] (the five best classes)."""
        if self.Wt is None:
            raise RuntimeError("no classifier yet: build_classifier or set_classifier first")
        C, D = self.Wt.shape
        if not feats.is_cuda or not targets.is_cuda:
            raise ValueError("features and targets must live on the MI355X (got a CPU tensor): there is no CPU path")
        if feats.dim() != 2 or feats.shape[1] != D:
            raise ValueError(f"features must be [B, {D}], got {tuple(feats.shape)}")
        B = feats.shape[0]
        if targets.is_floating_point() or targets.shape != (B,):
            raise ValueError(f"targets must be {B} integer class indices, got {targets.dtype} {tuple(targets.shape)}")
        f = aligned_f32(feats)
        y = targets.detach().to(torch.int64).contiguous()
        for name, t, shape, dt in (("logits_out", logits_out, (B, C), torch.float32), ("rank_out", rank_out, (B,), torch.int32),
                                   ("pred_out", pred_out, (B, 5), torch.int32)):
            if t is None:
                continue
            if not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or t.stride(-1) != 1 or (name == "pred_out" and not t.is_contiguous()):
                raise ValueError(f"{name} must be a {dt} tensor of shape {shape} on the MI355X, rows contiguous")
        ops.zs_topk(f, self.Wt, y, self.scale, B, C, D, self._counts, self._per_class, rank_out, pred_out, logits_out)

    def counts(self) -> Tuple[int, int, int]:
        """(top-1 hits, top-5 hits, rows seen), summed over the process group with one all-reduce; one copy to the host"""
        c = self._group.summed(self._counts).cpu()
        return int(c[0]), int(c[1]), int(c[2])

    def accuracy(self) -> Tuple[float, float]:
        """(top-1, top-5) in percent: count / n * 100 as the tool (:441)"""
        c1, c5, n = self.counts()
        return percent(c1, n), percent(c5, n)

    def per_class_accuracy(self) -> torch.Tensor:
        """top-1 accuracy in percent per class (CPU f64 [C]; NaN for a class no target named)"""
        if self._per_class is None:
            raise RuntimeError("no classifier yet: build_classifier or set_classifier first")
        pc = self._group.summed(self._per_class).cpu().to(torch.float64)
        return torch.where(pc[0] > 0, pc[1] / pc[0].clamp_min(1.0) * 100.0, torch.full_like(pc[0], float("nan")))

    def reset(self) -> None:
        self._counts.zero_()
        if self._per_class is not None:
            self._per_class.zero_()
