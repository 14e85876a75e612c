"""The five numbers the ADM evaluation suite reports for generated samples -- FID, sFID, Inception Score, precision and recall --
from ONE Inception pass per image.  Neither ADM's evaluator nor its TF graph is a reference of this project, so parity with that
program is unpinned: the pieces are pinned one by one (tests/fid_ref.py, tests/is_ref.py, tests/pr_ref.py), the spatial tap's
layout follows the published graph names (InceptionFeatures.forward_taps).

    inc = InceptionFeatures("pytorch_fid")
    sd = torch.load("inception_v3.pth"); inc.load_state_dict(sd)
    ge = GenEval(inc.cuda(), fc=(sd["fc.weight"], sd["fc.bias"]), k=3, split_size=5000)
    ref = np.load("reference_statistics.npz")                      # the caller loads an ADM-style reference file
    ge.set_reference(ref["mu"], ref["sigma"], ref["mu_s"], ref["sigma_s"])
    for u8 in real_batches:                                        # optional: the real set of precision / recall
        ge.add_real(u8)
    for u8 in generated_batches:
        ge.add_generated(u8)                                       # uint8 [B, H, W, 3] on the device
    ge.results()                                                   # {"fid", "sfid", "is", "is_std", "precision", "recall"}
GenEval(..., kid=True) (or kid=dict(subsets=..., subset_size=...)) adds "kid" / "kid_std", the Kernel Inception Distance of
vtp_amd.KID on the same pool rows (tests/mmd_ref.py).

add_generated / add_real run InceptionFeatures.forward_taps once on FID's preprocessing of the byte images; the pool row feeds a
FrechetStats (FID), the InceptionScore and the PrecisionRecall bank, the flattened spatial tap a second FrechetStats (sFID, its
width fixed by the first batch: 7 h w).  results() reuses frechet_distance, InceptionScore.result and PrecisionRecall.result as
they are.  A key is present only when its inputs are (result_keys): no `fc`, no "is" / "is_std"; no real images, no "precision" /
"recall"; "fid" / "sfid" need the reference statistics of set_reference -- which win where both are there -- or real images.
There is no CPU path."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .fid import FEATURE_DIM, FID, FrechetStats, InceptionFeatures, frechet_distance
from .inception_score import InceptionScore
from .kid import KID
from .precision_recall import PrecisionRecall


def result_keys(fc: bool, reference: bool, reference_spatial: bool, real_rows: int, precision_recall: bool = True, kid: bool = False,
                kid_subsets: bool = True) -> Tuple[str, ...]:
    """the keys of GenEval.results(): fc -- a classifier was given; reference / reference_spatial -- set_reference was called with
    (mu, sigma) / also with (mu_s, sigma_s); real_rows -- rows added through add_real on this rank's group; kid -- a KID was asked
    for, kid_subsets -- with the subset protocol (the full-set estimator has no "kid_std")"""
    keys = []
    if reference or real_rows >= 2:
        keys.append("fid")
    if reference_spatial or real_rows >= 2:
        keys.append("sfid")
    if fc:
        keys += ["is", "is_std"]
    if precision_recall and real_rows >= 1:
        keys += ["precision", "recall"]
    if kid and real_rows >= 1:
        keys += ["kid", "kid_std"] if kid_subsets else ["kid"]
    return tuple(keys)


class GenEval:
    """inception: an InceptionFeatures on the device.  fc: (weight [C, 2048], bias [C]) of the classifier, or None (no Inception
    Score).  k: the neighbourhood size of precision / recall (None: no banks are kept).  split_size: rows per split of the
    Inception Score.  group: a process group whose ranks each add their own images.  kid: a dict of vtp_amd.KID arguments (True:
    its defaults; None: no KID); with k set it reads the banks of precision / recall, so the pool rows are kept once."""

    def __init__(self, inception: InceptionFeatures, fc=None, k: Optional[int] = 3, split_size: Optional[int] = 5000, group=None,
                 kid=None):
        self.inception, self.group = inception, group
        self._fid = FID(inception, group)  # its preprocessing per variant; ref = the real images, rec = the generated ones
        self.device = self._fid.device
        self._spatial: Optional[Dict[str, FrechetStats]] = None  # made by the first batch, which fixes D = 7 h w
        self.isc = None if fc is None else InceptionScore(fc[0], fc[1], split_size=split_size, device=self.device, group=group)
        self.pr = None if k is None else PrecisionRecall(k=k, group=group, device=self.device)
        self.kid = None
        if kid is not None and kid is not False:
            kw = {} if kid is True else dict(kid)
            self.kid = KID(banks=self.pr, **kw) if self.pr is not None else KID(group=group, device=self.device, **kw)
        self._ref = self._ref_s = None
        self._real_rows = 0

    @property
    def real(self) -> FrechetStats:
        return self._fid.ref

    @property
    def generated(self) -> FrechetStats:
        return self._fid.rec

    def set_reference(self, mu, sigma, mu_s=None, sigma_s=None) -> None:
        """the pool statistics mu [2048], sigma [2048, 2048] of a reference set, and optionally the spatial ones mu_s [7 h w],
        sigma_s [7 h w, 7 h w]"""
        mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
        if mu.shape != (FEATURE_DIM,) or sigma.shape != (FEATURE_DIM, FEATURE_DIM):
            raise ValueError(f"mu must be [{FEATURE_DIM}] and sigma [{FEATURE_DIM}, {FEATURE_DIM}], got {mu.shape} and {sigma.shape}")
        if (mu_s is None) != (sigma_s is None):
            raise ValueError("mu_s and sigma_s go together")
        self._ref, self._ref_s = (mu, sigma), None
        if mu_s is not None:
            mu_s, sigma_s = np.asarray(mu_s, dtype=np.float64), np.asarray(sigma_s, dtype=np.float64)
            if mu_s.ndim != 1 or sigma_s.shape != (mu_s.size, mu_s.size):
                raise ValueError(f"mu_s must be [D] and sigma_s [D, D], got {mu_s.shape} and {sigma_s.shape}")
            self._ref_s = (mu_s, sigma_s)

    def _pass(self, u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        pool, spatial = self.inception.forward_taps(self._fid._images(u8))
        spatial = spatial.view(spatial.shape[0], -1)
        if self._spatial is None:
            D = spatial.shape[1]
            self._spatial = {s: FrechetStats(D, self.device, self.group) for s in ("real", "generated")}
        return pool, spatial

    def add_real(self, u8: torch.Tensor) -> None:
        """real byte images uint8 [B, H, W, 3]: the real side of every statistic and the real set of precision / recall"""
        pool, spatial = self._pass(u8)
        self.real.update(pool)
        self._spatial["real"].update(spatial)
        if self.pr is not None:
            self.pr.add_real_features(pool)
        elif self.kid is not None:
            self.kid.add_real_features(pool)
        self._real_rows += int(pool.shape[0])

    def add_generated(self, u8: torch.Tensor) -> None:
        """generated byte images uint8 [B, H, W, 3]: one Inception pass feeds all four accumulators"""
        pool, spatial = self._pass(u8)
        self.generated.update(pool)
        self._spatial["generated"].update(spatial)
        if self.isc is not None:
            self.isc.update(pool)
        if self.pr is not None:
            self.pr.add_fake_features(pool)
        elif self.kid is not None:
            self.kid.add_fake_features(pool)

    def _real_rows_of_group(self) -> int:
        if self.group is None:
            return self._real_rows
        import torch.distributed as dist
        where = "cpu" if dist.get_backend(self.group) == "gloo" else self.device  # gloo reduces host tensors
        t = torch.tensor([self._real_rows], device=where, dtype=torch.int64)
        if dist.get_world_size(self.group) > 1:
            dist.all_reduce(t, group=self.group)
        return int(t.item())

    def results(self, method: str = "auto") -> Dict[str, float]:
        if self.generated.n < 1:
            raise RuntimeError("results(): add_generated first")
        keys = result_keys(self.isc is not None, self._ref is not None, self._ref_s is not None, self._real_rows_of_group(),
                           self.pr is not None, self.kid is not None, self.kid is not None and self.kid.subsets > 0)
        out: Dict[str, float] = {}
        if "fid" in keys:
            mu, sigma = self._ref if self._ref is not None else self.real.mean_cov()
            out["fid"] = frechet_distance(mu, sigma, *self.generated.mean_cov(), method)
        if "sfid" in keys:
            mu, sigma = self._ref_s if self._ref_s is not None else self._spatial["real"].mean_cov()
            out["sfid"] = frechet_distance(mu, sigma, *self._spatial["generated"].mean_cov(), method)
        if "is" in keys:
            r = self.isc.result()
            out["is"], out["is_std"] = r["is"], r["is_std"]
        if "precision" in keys:
            out.update(self.pr.result())
        if "kid" in keys:
            out.update(self.kid.result())
        return out

    def reset(self) -> None:
        """forgets every image; the reference statistics of set_reference stay"""
        self._fid.reset()
        for s in (self._spatial or {}).values():
            s.reset()
        if self.isc is not None:
            self.isc.reset()
        if self.pr is not None:
            self.pr.reset()
        if self.kid is not None:
            self.kid.reset()
        self._real_rows = 0
