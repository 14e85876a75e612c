"""Kernel Inception Distance (Binkowski et al. 2018): the unbiased MMD^2 of two feature sets under the polynomial kernel
k(x, y) = (gamma x.y + coef0)^degree, gamma = 1 / D, coef0 = 1, degree = 3 -- reported beside FID where the sample count is small,
because FID is biased in N and KID is not.  Restated from the paper's definition.  Neither torch-fidelity nor the authors' TF code is
a reference of this project, so parity with those programs (their subset draws above all) is unpinned; the arithmetic is pinned by
the fp64 restatement in tests/mmd_ref.py.

    kid = KID(subsets=100, subset_size=1000)
    for u8 in real_batches:
        kid.add_real_features(fid.features(u8))
    for u8 in fake_batches:
        kid.add_fake_features(fid.features(u8))
    out = kid.result()                                                  # {"kid": float, "kid_std": float}

subsets >= 1, the standard protocol: per subset, subset_size rows of each set are drawn without replacement (on the host, from
torch.Generator().manual_seed(seed): randperm(n)[:subset_size], real then fake, subset by subset; the tables are kept for the next
result() on the same row counts) and
    MMD^2_u = Sxx / (m (m - 1)) + Syy / (m (m - 1)) - 2 Sxy / m^2,      m = subset_size,
with Sxx / Syy the kernel sums over the ordered pairs i != j of the real / generated subset and Sxy the sum over all pairs of one
real and one generated row.  "kid" is the mean over the subsets, "kid_std" their population standard deviation.  The index tables go
to the device once and the subsets run as the problems of three launches of vtp_mmd_poly_part: no subset is copied.
subsets = 0, the full-set estimator: all rows of both banks, weights 1 / (m (m - 1)), 1 / (n (n - 1)), 2 / (m n); {"kid"} only.

Rows are stored as given.  The products are formed in exact fp32 tile by tile (the bits of ops.gemm_nt_f32), everything after in
fp64 in one fixed order (csrc/mmd.hip), nothing is added atomically: result() repeats bit for bit whatever chunk_rows, query_rows,
the batching of add_* or the card.  Nothing synchronises with the host before the totals are read.  With `group`, each rank adds
ITS OWN rows and every rank returns what a single process fed the rank-major concatenation returns.  There is no CPU path."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import ops
from .banks import BankSet, Group, eval_device, spans
from .precision_recall import SETS, PrecisionRecall, bank_rows, gathered_rows

PASSES = (("real", "real"), ("fake", "fake"), ("real", "fake"))  # (queries, bank) of the three sweeps: Sxx, Syy, Sxy


def subset_tables(n_real: int, n_fake: int, subsets: int, subset_size: int, seed: int) -> Dict[str, torch.Tensor]:
    """the draws of the protocol, int32 [subsets, subset_size] on the host for each set: a function of the arguments alone"""
    g = torch.Generator().manual_seed(int(seed))
    out = {s: torch.empty(subsets, subset_size, dtype=torch.int32) for s in SETS}
    for p in range(subsets):
        out["real"][p] = torch.randperm(n_real, generator=g)[:subset_size]
        out["fake"][p] = torch.randperm(n_fake, generator=g)[:subset_size]
    return out


class KID:
    """subsets / subset_size: the protocol (subsets = 0: the full-set estimator).  degree (1 .. 8), gamma (None: 1 / D), coef0: the
    kernel.  seed: of the subset draws.  banks: a PrecisionRecall whose banks (its group gather included) are read instead of rows
    of this object's own -- add_* then belong to that object.  chunk_rows (rounded up to a multiple of 128) / query_rows: bank rows
    per kernel call and queries per pass of the full-set estimator; results do not depend on either."""

    def __init__(self, subsets: int = 100, subset_size: int = 1000, degree: int = 3, gamma: Optional[float] = None, coef0: float = 1.0,
                 seed: int = 0, banks: Optional[PrecisionRecall] = None, group=None, device=None, capacity: Optional[int] = None,
                 chunk_rows: int = 1 << 16, query_rows: int = 1024):
        if int(subsets) < 0 or (int(subsets) > 0 and int(subset_size) < 2):
            raise ValueError(f"subsets must be >= 0 and subset_size >= 2, got {subsets} and {subset_size}")
        if not 1 <= int(degree) <= ops.MMD_MAX_DEGREE:
            raise ValueError(f"degree must be 1 .. {ops.MMD_MAX_DEGREE}, got {degree}")
        if chunk_rows < 1 or query_rows < 1 or (capacity is not None and capacity < 1):
            raise ValueError("chunk_rows, query_rows and capacity must be positive")
        if banks is not None and not isinstance(banks, PrecisionRecall):
            raise ValueError(f"banks must be a PrecisionRecall, got {type(banks)}")
        if banks is not None and (group is not None or capacity is not None):
            raise ValueError("group and capacity belong to the PrecisionRecall whose banks are shared")
        self.device = eval_device("KID", None, banks.device if banks is not None else device)
        self.subsets, self.subset_size, self.degree = int(subsets), int(subset_size), int(degree)
        self.gamma, self.coef0, self.seed = gamma, float(coef0), int(seed)
        self.chunk_rows = (int(chunk_rows) + ops.MMD_TILE - 1) // ops.MMD_TILE * ops.MMD_TILE
        self.query_rows = int(query_rows)
        self._shared = banks is not None
        self._group = Group(banks.group if self._shared else group)
        self.banks = banks.banks if self._shared else BankSet(SETS, self.device, capacity)  # rows as given
        self._rowsums: Dict[str, torch.Tensor] = {}
        self._tables = (None, None)  # (the arguments of the last draws, their tables on the device)

    # ------------------------------------------------------------------------------------------------ banks
    def _add(self, which: str, feats: torch.Tensor) -> None:
        if self._shared:
            raise RuntimeError("this KID reads the banks of a PrecisionRecall: add the rows there")
        self._rowsums = {}
        self.banks.append(which, feats, f"{which} features")

    def add_real_features(self, feats: torch.Tensor) -> None:
        """appends the rows of feats [n, D] to the real bank: device only"""
        self._add("real", feats)

    def add_fake_features(self, feats: torch.Tensor) -> None:
        """appends the rows of feats [n, D] to the bank of generated samples: device only"""
        self._add("fake", feats)

    def rows(self, which: str) -> torch.Tensor:
        """this rank's rows of a bank, f32 [size, D] (a view)"""
        return bank_rows(self.banks, which)

    def reset(self) -> None:
        """empties both banks (shared banks are their owner's to empty) and forgets the last result"""
        if not self._shared:
            self.banks.clear()
        self._rowsums = {}

    # ------------------------------------------------------------------------------------------------ evaluation
    def _gamma(self, D: int) -> float:
        return 1.0 / D if self.gamma is None else float(self.gamma)

    def _subset_totals(self, x: Dict[str, torch.Tensor]) -> torch.Tensor:
        """f64 [3, subsets] on the device: Sxx, Syy, Sxy of every subset, three launches with P = subsets"""
        P, m = self.subsets, self.subset_size
        key = (x["real"].shape[0], x["fake"].shape[0], P, m, self.seed)
        if self._tables[0] != key:  # the draws are a function of these alone: a result on the same row counts reuses them
            self._tables = (key, {s: t.to(self.device, non_blocking=True) for s, t in subset_tables(*key).items()})
        tab = self._tables[1]
        gamma = self._gamma(x["real"].shape[1])
        part = torch.empty(ops.mmd_workspace_bytes(m, m, P) // 8, device=self.device, dtype=torch.float64).view(P, -1, m)
        totals = torch.empty(3, P, device=self.device, dtype=torch.float64)
        for i, (qs, xs) in enumerate(PASSES):
            rowsum = torch.zeros(P, m, device=self.device, dtype=torch.float64)
            ops.mmd_poly_part(x[qs], x[xs], part, gamma, self.coef0, self.degree, query_base=0 if qs == xs else -1, index_base=0,
                              qi=tab[qs], xi=tab[xs])
            ops.mmd_fold(part, rowsum)
            ops.mmd_total(rowsum, totals[i])
        return totals

    def _full_totals(self, x: Dict[str, torch.Tensor]) -> torch.Tensor:
        """f64 [3, 1] on the device: Sxx, Syy, Sxy over all rows, in passes of query_rows queries over chunks of chunk_rows bank rows"""
        gamma = self._gamma(x["real"].shape[1])
        totals = torch.empty(3, 1, device=self.device, dtype=torch.float64)
        rows = max(x[s].shape[0] for s in SETS)
        qr, cr = min(self.query_rows, rows), min(self.chunk_rows, rows)
        ws = torch.empty(ops.mmd_workspace_bytes(qr, cr, 1) // 8, device=self.device, dtype=torch.float64)
        self._rowsums = {}
        for i, (qs, xs) in enumerate(PASSES):
            q, bank = x[qs], x[xs]
            rowsum = torch.zeros(1, q.shape[0], device=self.device, dtype=torch.float64)
            for b0, b1 in spans(q.shape[0], self.query_rows):
                for n0, n1 in spans(bank.shape[0], self.chunk_rows):
                    tiles = (n1 - n0 + ops.MMD_TILE - 1) // ops.MMD_TILE
                    part = ws[:tiles * (b1 - b0)].view(1, tiles, b1 - b0)
                    ops.mmd_poly_part(q[b0:b1], bank[n0:n1], part, gamma, self.coef0, self.degree, query_base=b0 if qs == xs else -1,
                                      index_base=n0)
                    ops.mmd_fold(part, rowsum[:, b0:b1])
            ops.mmd_total(rowsum, totals[i])
            self._rowsums[f"{qs}_{xs}"] = rowsum[0]
        return totals

    def result(self) -> Dict[str, float]:
        """{"kid": the mean of the subsets' MMD^2_u, "kid_std": their population standard deviation}, or with subsets = 0 {"kid": the
        MMD^2_u of the whole sets}; recomputed from the banks, one copy to the host"""
        x = gathered_rows(self.banks, self._group)
        nr, nf = x["real"].shape[0], x["fake"].shape[0]
        if self.subsets:
            m = self.subset_size
            if m > min(nr, nf):
                raise ValueError(f"subset_size = {m} exceeds the smaller set ({nr} real rows, {nf} generated rows)")
            t = self._subset_totals(x).cpu().tolist()
            vals = [sxx / (m * (m - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (m * m) for sxx, syy, sxy in zip(*t)]
            mean = math.fsum(vals) / len(vals)
            return {"kid": mean, "kid_std": math.sqrt(math.fsum((v - mean) ** 2 for v in vals) / len(vals))}
        if min(nr, nf) < 2:
            raise ValueError(f"the full-set estimator needs at least 2 rows per set ({nr} real rows, {nf} generated rows)")
        (sxx,), (syy,), (sxy,) = self._full_totals(x).cpu().tolist()
        return {"kid": sxx / (nr * (nr - 1)) + syy / (nf * (nf - 1)) - 2.0 * sxy / (nr * nf)}

    def row_sums(self) -> Dict[str, torch.Tensor]:
        """the row sums of the last full-set result, f64 on the device: "real_real" [m] and "fake_fake" [n] (each row's kernel sum
        over the other rows of its set) and "real_fake" [m] (each real row's sum over the generated set)"""
        if not self._rowsums:
            raise RuntimeError("row_sums() is valid after result() with subsets = 0")
        return self._rowsums
