"""Inception Score of generated samples (Salimans et al. 2016; the figure the ADM evaluation suite reports beside FID), restated
from the papers' definition.  Neither ADM's evaluator nor its TF graph is a reference of this project, so parity with that program
is unpinned; the arithmetic is pinned by the fp64 restatement in tests/is_ref.py.

    isc = InceptionScore.load_fc(torch.load("inception_v3.pth"))    # "fc.weight" [C, 2048], "fc.bias" [C]
    for u8 in fake_batches:
        isc.update(fid.features(u8))                                # the pool features InceptionFeatures returns
    out = isc.result()                                              # {"is": float, "is_std": float, "splits": int}

With p_i = softmax(logits_i), the rows cut in the order they were added into splits of split_size rows (the last may be partial;
split_size=None: one split over everything):
    KL_s = (1 / n_s) sum_i sum_c p_ic (log p_ic - log m_c),  m_c = (1 / n_s) sum_i p_ic,  IS = mean_s exp(KL_s),
and is_std the population standard deviation of exp(KL_s) over the splits.

update(): logits = vtp_gemm_nt_f32 with the bias epilogue (exact fp32, K = D), then csrc/inception_score.hip: vtp_is_rows (softmax
and h_i = sum_c p_ic (l_ic - lse_i) per row in fp64) and vtp_is_accum (H_s = sum_i h_i and S_sc = sum_i p_ic per split, rows in
order, one thread per element).  The batch goes through in chunks of max_rows rows, so the workspace is bounded; nothing
synchronises with the host, and any split of the same rows over updates leaves the same bits.  result() copies the sums to the
host once and finishes in fp64: KL_s = (H_s - sum_c S_sc log(S_sc / n_s)) / n_s (inception_score_from_sums).

The GEMM needs a class count that is a multiple of 8: the weight and bias are padded with zero rows on upload and the true C goes
to vtp_is_rows, so the padded logits never enter the softmax.

With `group`, each rank adds ITS OWN rows and fills the slots in its own row order; result() sums [n_s | state] over the ranks
(one all-reduce, after the slot count is agreed on), so a slot then holds split_size rows PER RANK.  There is no CPU path."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops

F32, F64 = torch.float32, torch.float64


def inception_score_from_sums(n, H, S) -> Tuple[float, float]:
    """(mean, population std) over the splits of exp(KL_s), KL_s = (H_s - sum_c S_sc log(S_sc / n_s)) / n_s, in fp64 on the host.
    n [s] rows per split, H [s] = sum_i sum_c p_ic (l_ic - lse_i), S [s, C] = sum_i p_ic; a term with S_sc = 0 is 0; splits
    without rows are left out"""
    n = np.atleast_1d(np.asarray(n, dtype=np.float64))
    H = np.atleast_1d(np.asarray(H, dtype=np.float64))
    S = np.asarray(S, dtype=np.float64)
    S = S.reshape(1, -1) if S.ndim == 1 else S
    if n.ndim != 1 or H.shape != n.shape or S.ndim != 2 or S.shape[0] != n.shape[0]:
        raise ValueError(f"inception_score_from_sums: n [s], H [s] and S [s, C] must agree, got {n.shape}, {H.shape}, {S.shape}")
    keep = n > 0
    if not keep.any():
        raise RuntimeError("inception_score_from_sums: no rows")
    n, H, S = n[keep], H[keep], S[keep]
    pos = S > 0
    cross = np.where(pos, S * np.log(np.where(pos, S, 1.0) / n[:, None]), 0.0).sum(axis=1)
    scores = np.exp((H - cross) / n)
    return float(scores.mean()), float(scores.std())


def pad_fc(weight: torch.Tensor, bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weight f32 [Cp, D], bias f32 [Cp]) with Cp = C rounded up to a multiple of 8, the added rows zero"""
    C, D = weight.shape
    Cp = (C + 7) // 8 * 8
    w = torch.zeros(Cp, D, dtype=F32)
    b = torch.zeros(Cp, dtype=F32)
    w[:C].copy_(weight.detach().to(F32))
    b[:C].copy_(bias.detach().to(F32))
    return w, b


class InceptionScore:
    """fc_weight [C, D], fc_bias [C]: the classifier on the pool features (C >= 2, D a multiple of 8).  split_size: rows per split
    (None: one split).  max_rows: rows per pass of update(), which bounds the workspace.  group: a process group whose ranks each
    add their own rows."""

    def __init__(self, fc_weight: torch.Tensor, fc_bias: torch.Tensor, split_size: Optional[int] = 5000, device=None, group=None,
                 max_rows: int = 1024):
        if fc_weight.dim() != 2 or fc_bias.dim() != 1 or fc_bias.shape[0] != fc_weight.shape[0]:
            raise ValueError(f"fc_weight must be [C, D] and fc_bias [C], got {tuple(fc_weight.shape)} and {tuple(fc_bias.shape)}")
        C, D = fc_weight.shape
        if C < 2 or D < 8 or D % 8:
            raise ValueError(f"need C >= 2 classes and D a positive multiple of 8, got C={C} D={D}")
        if split_size is not None and int(split_size) < 1:
            raise ValueError(f"split_size must be positive or None, got {split_size}")
        if int(max_rows) < 1:
            raise ValueError(f"max_rows must be positive, got {max_rows}")
        if not torch.cuda.is_available():
            raise RuntimeError("vtp_amd.InceptionScore runs on the MI355X kernels only (no CPU path)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("vtp_amd.InceptionScore runs on the MI355X kernels only: the device must be cuda (no CPU path)")
        self.C, self.D, self.group = int(C), int(D), group
        self.split_size = None if split_size is None else int(split_size)
        self.max_rows = int(max_rows)
        w, b = pad_fc(fc_weight.cpu(), fc_bias.cpu())
        self._w, self._b = w.to(self.device), b.to(self.device)
        self._logits = self._p = self._h = None  # workspace of update(), allocated at the first one
        self._state = torch.zeros(1, 1 + self.C, device=self.device, dtype=F64)  # [slots, H | S_0 .. S_C-1]; grows by doubling
        self.n = 0

    @classmethod
    def load_fc(cls, state_dict, **kw) -> "InceptionScore":
        """from the "fc.weight" [C, 2048] and "fc.bias" [C] of torchvision's inception_v3 (or pytorch_fid's) state dict"""
        for key in ("fc.weight", "fc.bias"):
            if key not in state_dict:
                raise KeyError(f"the state dict has no {key!r}")
        return cls(state_dict["fc.weight"], state_dict["fc.bias"], **kw)

    # ------------------------------------------------------------------------------------------------ compute
    def _check(self, feats: torch.Tensor) -> torch.Tensor:
        if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
            raise ValueError("feats must live on the MI355X (got a CPU tensor): there is no CPU path")
        if feats.dim() != 2 or feats.shape[1] != self.D or feats.shape[0] < 1:
            raise ValueError(f"feats must be [n >= 1, {self.D}], got {tuple(feats.shape)}")
        return feats.detach().to(F32).contiguous()

    def _into(self, f: torch.Tensor, out: torch.Tensor) -> None:
        ops.gemm_nt_f32(f, self._w, out, bias=self._b)

    def logits(self, feats: torch.Tensor) -> torch.Tensor:
        """f32 [B, C]: feats W^T + b, the bits of vtp_gemm_nt_f32 with the bias epilogue (a view of the padded [B, Cp] product when
        C is not a multiple of 8)"""
        f = self._check(feats)
        out = torch.empty(f.shape[0], self._w.shape[0], device=self.device, dtype=F32)
        self._into(f, out)
        return out[:, :self.C]

    def _slots_for(self, rows: int) -> None:
        need = 1 if self.split_size is None else (rows - 1) // self.split_size + 1
        have = self._state.shape[0]
        if need > have:
            grown = torch.zeros(max(need, 2 * have), 1 + self.C, device=self.device, dtype=F64)
            grown[:have].copy_(self._state)
            self._state = grown

    def update(self, feats: torch.Tensor) -> None:
        """adds the rows of feats f32 [n, D] (device only), in order"""
        f = self._check(feats)
        if self._logits is None:
            self._logits = torch.empty(self.max_rows, self._w.shape[0], device=self.device, dtype=F32)
            self._p = torch.empty(self.max_rows, self.C, device=self.device, dtype=F64)
            self._h = torch.empty(self.max_rows, device=self.device, dtype=F64)
        self._slots_for(self.n + f.shape[0])
        for b0 in range(0, f.shape[0], self.max_rows):
            m = min(self.max_rows, f.shape[0] - b0)
            lg, p, h = self._logits[:m], self._p[:m], self._h[:m]
            self._into(f[b0:b0 + m], lg)
            ops.is_rows(lg, self.C, p, h)
            ops.is_accum(p, h, self._state, self.n, self.split_size)
            self.n += m

    def _counts(self, slots: int) -> torch.Tensor:
        """rows per slot of this rank, f64 [slots]"""
        if self.split_size is None:
            return torch.tensor([float(self.n)] + [0.0] * (slots - 1), dtype=F64)
        at = torch.arange(slots, dtype=F64) * self.split_size
        return (self.n - at).clamp(0, self.split_size)

    def _gathered(self) -> torch.Tensor:
        """[n_s | H_s | S_s] per slot, summed over the group, on the host (one copy)"""
        slots = self._state.shape[0]
        if self.group is None:
            return torch.cat([self._counts(slots)[:, None], self._state.cpu()], 1)
        import torch.distributed as dist
        many = dist.get_world_size(self.group) > 1
        where = "cpu" if dist.get_backend(self.group) == "gloo" else self.device  # gloo reduces host tensors
        if many:  # the ranks may have grown their states differently: agree on the slot count first
            most = torch.tensor([slots], device=where, dtype=torch.int64)
            dist.all_reduce(most, op=dist.ReduceOp.MAX, group=self.group)
            slots = int(most.item())
        t = torch.zeros(slots, 2 + self.C, device=where, dtype=F64)
        t[:, 0] = self._counts(slots)
        t[:self._state.shape[0], 1:] = self._state.to(where)
        if many:
            dist.all_reduce(t, group=self.group)
        return t.cpu()

    def result(self) -> Dict[str, float]:
        """{"is": mean_s exp(KL_s), "is_std": the population standard deviation of exp(KL_s) over the splits, "splits": their number}"""
        t = self._gathered().numpy()
        if t[:, 0].sum() < 1:
            raise RuntimeError("result(): no rows were added")
        mean, std = inception_score_from_sums(t[:, 0], t[:, 1], t[:, 2:])
        return {"is": mean, "is_std": std, "splits": int((t[:, 0] > 0).sum())}

    def reset(self) -> None:
        self._state.zero_()
        self.n = 0

    def state_dict(self) -> dict:
        return {"n": self.n, "split_size": self.split_size, "state": self._state.clone()}

    def load_state_dict(self, sd: dict) -> None:
        if sd["split_size"] != self.split_size or sd["state"].shape[1] != 1 + self.C:
            raise ValueError(f"the state was taken with split_size={sd['split_size']} and {sd['state'].shape[1] - 1} classes, this object has "
                             f"split_size={self.split_size} and {self.C}")
        self._state = sd["state"].to(self.device, F64).clone()
        self.n = int(sd["n"])
