"""Weighted k-NN classification on frozen features: the evaluation DINO and DINOv2 run on a self-supervised trunk during and after
training (k = 10, 20, 100, 200, temperature 0.07, top-1 and top-5), restated from the papers' description.  Neither code base is a
reference of this project, so parity with those programs is unpinned; the arithmetic is pinned by the fp64 restatement in
tests/knn_ref.py.

    knn = Knn(model, num_classes=1000, ks=(10, 20, 100, 200), temperature=0.07)
    for images, labels in train_loader:
        knn.add_bank(images.cuda(), labels.cuda())
    for images, targets in val_loader:
        knn.update(images.cuda(), targets.cuda())
    acc = knn.accuracy()                                               # {k: (top-1 %, top-5 %)}

Every feature row is L2-normalised on the device (F.normalize, eps 1e-12).  A batch of queries is scored by csrc/knn.hip: the
bank is walked in chunks by vtp_knn_topk, which forms the similarities in exact fp32 tile by tile, never writes the [B, N] matrix
and keeps per query the first max(ks) bank rows under (similarity descending, bank index ascending) -- a total order, so the
lists and everything after them repeat bit for bit whatever the chunk size or the batch -- and vtp_knn_vote turns the lists into
the weighted votes, the rank of every target and the integer counters.  No host synchronisation before the accuracy is asked for.

With `group`, each rank evaluates its own queries against a FULL copy of the bank (every rank adds every bank row) and the
counters are summed with one all-reduce.  A bank sharded across ranks is out of scope: 1.28 M rows x 768 x 4 B = 3.9 GB fit one
GPU many times.  There is no CPU path: tensors on the CPU raise."""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .banks import Bank, Group, Workspace, eval_device, feature_rows, spans
from .zeroshot import percent


def cls_feature(model, images: torch.Tensor) -> torch.Tensor:
    """the protocol's feature: the class token after the final norm"""
    return model.get_last_layer_feature(images)["cls_token"]


def check_ks(ks: Sequence[int]) -> Tuple[int, ...]:
    ks = tuple(int(k) for k in ks)
    if not 1 <= len(ks) <= 8:
        raise ValueError(f"ks must name 1 to 8 neighbour counts, got {len(ks)}")
    if ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks must be positive and strictly ascending, got {ks}")
    if ks[-1] > ops.KNN_MAX_K:
        raise ValueError(f"ks must not exceed {ops.KNN_MAX_K}, got {ks}")
    return ks


def neighbour_lists(q: torch.Tensor, x: torch.Tensor, k: int, ws: Workspace, query_rows: int, chunk_rows: int, splits: int,
                    sims: torch.Tensor, idx: torch.Tensor) -> None:
    """merges the bank rows x [N, D] into the neighbour lists sims f32 [B, k] / idx int64 [B, k] of the queries q [B, D], which
    start out (-inf, -1): passes of query_rows queries over chunks of chunk_rows bank rows"""
    for b0, b1 in spans(q.shape[0], query_rows):
        buf = ws.at_least(ops.knn_workspace_bytes(b1 - b0, k, splits))
        for n0, n1 in spans(x.shape[0], chunk_rows):
            ops.knn_topk(q[b0:b1], x[n0:n1], n0, k, sims[b0:b1], idx[b0:b1], buf, splits)


class Knn:
    """model: a vtp_amd.VTPModel, or None when features are given (add_bank_features / update_features).  feature_fn(model, images)
    -> [B, D] replaces the class token after the final norm.  capacity: bank rows to allocate up front (the buffer doubles when it
    is full).  chunk_rows / query_rows: bank rows per vtp_knn_topk call and queries per pass over the bank; results do not depend
    on either.  group: a process group whose ranks each evaluate their own queries; counts() sums over it."""

    def __init__(self, model, num_classes: int = 1000, ks: Sequence[int] = (10, 20, 100, 200), temperature: float = 0.07, group=None,
                 capacity: Optional[int] = None, feature_fn: Optional[Callable] = None, device=None, chunk_rows: int = 1 << 20,
                 query_rows: int = 1024):
        self.ks = check_ks(ks)
        if num_classes < 5:
            raise ValueError(f"k-NN top-5 needs at least 5 classes, got {num_classes}")
        if not temperature > 0:
            raise ValueError(f"temperature must be positive, got {temperature}")
        if chunk_rows < 1 or query_rows < 1 or (capacity is not None and capacity < 1):
            raise ValueError("chunk_rows, query_rows and capacity must be positive")
        self.device = eval_device("Knn", model, device)
        self.model, self.group = model, group
        self.num_classes, self.temperature = int(num_classes), float(temperature)
        self.feature_fn = feature_fn or cls_feature
        self.chunk_rows, self.query_rows = int(chunk_rows), int(query_rows)
        self._group = Group(group)
        self._bank = Bank(self.device, capacity, {"labels": torch.int32})  # the normalised rows and their labels
        self._frozen = False  # an update has seen the bank
        self._counts = torch.zeros(len(self.ks), 3, device=self.device, dtype=torch.int64)  # per k: top-1 hits, top-5 hits, rows
        self._ws = Workspace(self.device)

    # ------------------------------------------------------------------------------------------------ features
    def _features(self, images: torch.Tensor) -> torch.Tensor:
        if self.model is None:
            raise RuntimeError("Knn was built without a model: use add_bank_features / update_features")
        if not images.is_cuda:
            raise ValueError("images must live on the MI355X (got a CPU tensor): there is no CPU path")
        with torch.no_grad():
            return self.feature_fn(self.model, images)

    def _ints(self, t: torch.Tensor, n: int, what: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{what} must live on the MI355X (got a CPU tensor): there is no CPU path")
        if t.is_floating_point() or t.shape != (n,):
            raise ValueError(f"{what} must be {n} integer class indices, got {t.dtype} {tuple(t.shape)}")
        return t.detach()

    # ------------------------------------------------------------------------------------------------ bank
    def add_bank(self, images: torch.Tensor, labels: torch.Tensor) -> None:
        self.add_bank_features(self._features(images), labels)

    def add_bank_features(self, feats: torch.Tensor, labels: torch.Tensor) -> None:
        """appends the normalised rows of feats [n, D] and their labels [n] to the bank: device only"""
        if self._frozen:
            raise RuntimeError("the bank has been evaluated against: reset() before adding to it")
        f = feature_rows(feats, "bank features", self._bank.width, align=True)
        n, D = f.shape
        y = self._ints(labels, n, "bank labels").to(torch.int32)
        rows, lab = self._bank.reserve(n, D)
        ops.zs_class_mean(f, rows, n, 1, D, 1e-12)  # F.normalize of every row (T = 1)
        lab.copy_(y)

    size = property(lambda self: self._bank.size, doc="bank rows in use")
    capacity = property(lambda self: self._bank.capacity, doc="bank rows allocated")

    @property
    def bank(self) -> torch.Tensor:
        """the normalised bank rows in use, f32 [size, D] (a view)"""
        if not self.size:
            raise RuntimeError("the bank is empty: add_bank / add_bank_features first")
        return self._bank.rows

    @property
    def bank_labels(self) -> torch.Tensor:
        if not self.size:
            raise RuntimeError("the bank is empty: add_bank / add_bank_features first")
        return self._bank.column("labels")

    # ------------------------------------------------------------------------------------------------ evaluation
    def update(self, images: torch.Tensor, targets: torch.Tensor) -> None:
        self.update_features(self._features(images), targets)

    def update_features(self, feats: torch.Tensor, targets: torch.Tensor, sims_out: Optional[torch.Tensor] = None,
                        idx_out: Optional[torch.Tensor] = None, rank_out: Optional[torch.Tensor] = None,
                        pred_out: Optional[torch.Tensor] = None, splits: int = 0) -> None:
        """adds one batch of query features [B, D] to the counters: device only, no host synchronisation.  Optional outputs (on the
        device, contiguous), K = max(ks), nk = len(ks): sims_out f32 [B, K] and idx_out int64 [B, K] (the neighbour lists), rank_out
        int32 [B, nk] (classes ranked before the target; num_classes for a target outside [0, num_classes)), pred_out int32
        [B, nk, 5].  splits: the bank splits of vtp_knn_topk (0: its heuristic); the result does not depend on it."""
        K, nk = self.ks[-1], len(self.ks)
        if self.size < K:
            raise RuntimeError(f"the bank holds {self.size} rows, fewer than max(ks) = {K}")
        f = feature_rows(feats, "query features", self._bank.width, align=True)
        B, D = f.shape
        y = self._ints(targets, B, "targets").to(torch.int64).contiguous()
        for name, t, shape, dt in (("sims_out", sims_out, (B, K), torch.float32), ("idx_out", idx_out, (B, K), torch.int64),
                                   ("rank_out", rank_out, (B, nk), torch.int32), ("pred_out", pred_out, (B, nk, 5), torch.int32)):
            if t is not None and (not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on the MI355X")
        self._frozen = True
        q = torch.empty(B, D, device=self.device, dtype=torch.float32)
        ops.zs_class_mean(f, q, B, 1, D, 1e-12)
        sims = sims_out if sims_out is not None else torch.empty(B, K, device=self.device, dtype=torch.float32)
        idx = idx_out if idx_out is not None else torch.empty(B, K, device=self.device, dtype=torch.int64)
        sims.fill_(float("-inf"))  # (-inf, -1): an empty entry
        idx.fill_(-1)
        neighbour_lists(q, self._bank.rows, K, self._ws, self.query_rows, self.chunk_rows, splits, sims, idx)
        ops.knn_vote(sims, idx, self.bank_labels, y, self.ks, 1.0 / self.temperature, self.num_classes, self._counts, rank_out, pred_out)

    def counts(self) -> Dict[int, Tuple[int, int, int]]:
        """{k: (top-1 hits, top-5 hits, rows seen)}, summed over the process group with one all-reduce; one copy to the host"""
        c = self._group.summed(self._counts).cpu()
        return {k: (int(c[m, 0]), int(c[m, 1]), int(c[m, 2])) for m, k in enumerate(self.ks)}

    def accuracy(self) -> Dict[int, Tuple[float, float]]:
        """{k: (top-1, top-5)} in percent: count / n * 100"""
        return {k: (percent(c1, n), percent(c5, n)) for k, (c1, c5, n) in self.counts().items()}

    def reset(self) -> None:
        """clears the counters and keeps the bank, which may be added to again"""
        self._counts.zero_()
        self._frozen = False
