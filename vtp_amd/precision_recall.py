"""k-NN manifold precision / recall of generated samples (Kynkaanniemi et al. 2019; the estimate the ADM evaluation suite reports
with k = 3 beside FID and IS), restated from the paper's description.  Neither ADM's evaluator nor the authors' code is a reference
of this project, so parity with those programs is unpinned; the arithmetic is pinned by the fp64 restatement in tests/pr_ref.py.

    pr = PrecisionRecall(k=3)
    for u8 in real_batches:
        pr.add_real_features(fid.features(u8))
    for u8 in fake_batches:
        pr.add_fake_features(fid.features(u8))
    out = pr.result()                                                   # {"precision": float, "recall": float}

The radius of a row is the distance to its k-th nearest neighbour within its own set (the row itself excluded by index).  A query
is covered by a set when it lies within the radius of at least one of the set's rows.  precision = the share of generated rows
covered by the real set, recall = the share of real rows covered by the generated set.

Rows are stored as given (no normalisation).  result() recomputes everything from the two banks with csrc/precision_recall.hip:
vtp_pr_sqnorm for the norms, vtp_pr_knn_dist (each set against itself) for the radii, vtp_pr_cover for the hit counts.  The
squared distances are formed in exact fp32 tile by tile and never written; only values are selected, so the result repeats bit for
bit whatever chunk_rows or query_rows.  No host synchronisation before the covered counts are read.

With `group`, each rank adds ITS OWN rows; result() all-gathers both banks (rank-major) and every rank computes the whole result
redundantly, so every rank returns what a single process fed the rank-major concatenation returns.  There is no CPU path."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import ops
from .banks import BankSet, Group, Workspace, eval_device, spans

SETS = ("real", "fake")


def bank_rows(banks: BankSet, which: str) -> torch.Tensor:
    """this rank's rows of the real or the generated bank, f32 [size, D] (a view)"""
    if not banks[which].size:
        raise RuntimeError(f"the {which} bank is empty: add_{which}_features first")
    return banks[which].rows


def gathered_rows(banks: BankSet, group: Group) -> Dict[str, torch.Tensor]:
    """{"real", "fake"}: both banks of the whole group, rank-major (this rank's rows without a group, where an empty bank raises)"""
    if group.world == 1:
        return {s: bank_rows(banks, s) for s in SETS}
    rows, _, totals = banks.gathered(group)
    if not any(totals.values()):
        raise RuntimeError("both banks are empty on every rank: add_real_features / add_fake_features first")
    return rows


class PrecisionRecall:
    """k: neighbourhood size, 1 .. 8.  capacity: rows to allocate per bank up front (a bank doubles when it is full).  chunk_rows /
    query_rows: bank rows per kernel call and queries per pass over the bank; results do not depend on either.  group: a process
    group whose ranks each add their own rows."""

    def __init__(self, k: int = 3, group=None, device=None, capacity: Optional[int] = None, chunk_rows: int = 1 << 16,
                 query_rows: int = 1024):
        if not 1 <= int(k) <= ops.PR_MAX_K:
            raise ValueError(f"k must be 1 .. {ops.PR_MAX_K}, got {k}")
        if chunk_rows < 1 or query_rows < 1 or (capacity is not None and capacity < 1):
            raise ValueError("chunk_rows, query_rows and capacity must be positive")
        self.device = eval_device("PrecisionRecall", None, device)
        self.k, self.group = int(k), group
        self.chunk_rows, self.query_rows = int(chunk_rows), int(query_rows)
        self._group = Group(group)
        self.banks = BankSet(SETS, self.device, capacity)  # rows as given
        self._ws = Workspace(self.device)
        self.reset()

    def reset(self) -> None:
        """empties both banks and forgets the last result"""
        self.banks.clear()
        self._radii: Dict[str, torch.Tensor] = {}
        self._hits: Dict[str, torch.Tensor] = {}
        self._covered: Optional[torch.Tensor] = None  # int64 [2] on the device: covered fake rows, covered real rows

    # ------------------------------------------------------------------------------------------------ banks
    def _add(self, which: str, feats: torch.Tensor) -> None:
        self.banks.append(which, feats, f"{which} features")
        self._radii, self._hits, self._covered = {}, {}, None

    def add_real_features(self, feats: torch.Tensor) -> None:
        """appends the rows of feats [n, D] to the real bank: device only"""
        self._add("real", feats)

    def add_fake_features(self, feats: torch.Tensor) -> None:
        """appends the rows of feats [n, D] to the bank of generated samples: device only"""
        self._add("fake", feats)

    def rows(self, which: str) -> torch.Tensor:
        """this rank's rows of a bank, f32 [size, D] (a view)"""
        return bank_rows(self.banks, which)

    def gathered(self) -> Dict[str, torch.Tensor]:
        """{"real", "fake"}: both banks of the whole group, rank-major, f32 [N, D] on the device (this rank's rows without a group):
        what result() evaluates, for an evaluation that shares these banks (vtp_amd.KID)"""
        return gathered_rows(self.banks, self._group)

    # ------------------------------------------------------------------------------------------------ evaluation
    def _radii_of(self, x: torch.Tensor, xn: torch.Tensor) -> torch.Tensor:
        """the squared distance of every row of x to its k-th nearest other row"""
        n = x.shape[0]
        dist = torch.full((n, ops.PR_MAX_K), float("inf"), device=self.device, dtype=torch.float32)
        for b0, b1 in spans(n, self.query_rows):
            ws = self._ws.at_least(ops.pr_workspace_bytes(b1 - b0))
            for n0, n1 in spans(n, self.chunk_rows):
                ops.pr_knn_dist(x[b0:b1], xn[b0:b1], x[n0:n1], xn[n0:n1], dist[b0:b1], ws, query_base=b0, index_base=n0)
        return dist[:, self.k - 1].contiguous()

    def _hits_of(self, q: torch.Tensor, qn: torch.Tensor, x: torch.Tensor, xn: torch.Tensor, r2: torch.Tensor) -> torch.Tensor:
        """per row of q the number of rows of x whose ball holds it"""
        hits = torch.zeros(q.shape[0], device=self.device, dtype=torch.int32)
        for b0, b1 in spans(q.shape[0], self.query_rows):
            for n0, n1 in spans(x.shape[0], self.chunk_rows):
                ops.pr_cover(q[b0:b1], qn[b0:b1], x[n0:n1], xn[n0:n1], r2[n0:n1], hits[b0:b1])
        return hits

    def _compute(self) -> None:
        x = self.gathered()
        for s in SETS:
            if x[s].shape[0] < self.k + 1:
                raise RuntimeError(f"the {s} set holds {x[s].shape[0]} rows, fewer than k + 1 = {self.k + 1}: its radii would be infinite")
        norms = {}
        for s in SETS:
            norms[s] = torch.empty(x[s].shape[0], device=self.device, dtype=torch.float32)
            ops.pr_sqnorm(x[s], norms[s])
        self._radii = {s: self._radii_of(x[s], norms[s]) for s in SETS}
        self._hits = {"fake": self._hits_of(x["fake"], norms["fake"], x["real"], norms["real"], self._radii["real"]),
                      "real": self._hits_of(x["real"], norms["real"], x["fake"], norms["fake"], self._radii["fake"])}
        self._covered = torch.stack([(self._hits["fake"] > 0).sum(), (self._hits["real"] > 0).sum()]).to(torch.int64)

    def counts(self) -> Dict[str, Tuple[int, int]]:
        """{"precision": (generated rows covered by the real set, generated rows), "recall": (real rows covered by the generated
        set, real rows)}; computes the result if the banks changed since the last one; one copy to the host"""
        if self._covered is None:
            self._compute()
        c = self._covered.cpu()
        return {"precision": (int(c[0]), int(self._hits["fake"].shape[0])), "recall": (int(c[1]), int(self._hits["real"].shape[0]))}

    def result(self) -> Dict[str, float]:
        """{"precision": covered generated rows / generated rows, "recall": covered real rows / real rows}, recomputed from the banks"""
        self._covered = None
        return {name: covered / rows for name, (covered, rows) in self.counts().items()}

    def radii(self, which: str) -> torch.Tensor:
        """the squared radii of the real or the generated rows, f32 [N] on the device; valid after result()"""
        if which not in self._radii:
            raise RuntimeError("radii() is valid after result()")
        return self._radii[which]

    def hits(self, which: str) -> torch.Tensor:
        """int32 [N] on the device: for "fake" the hits of each generated row against the real set, for "real" the hits of each real
        row against the generated set; valid after result()"""
        if which not in self._hits:
            raise RuntimeError("hits() is valid after result()")
        return self._hits[which]
