"""The head store LinearProbe and SegProbe share: linear heads sorted into groups that read the same columns of the input matrix,
each group stored stacked, with the SGD momentum buffers, the per-head learning rates and the cosine schedule beside them.  Which
heads exist, which group a head belongs to and how its weights are drawn is the caller's; nothing here draws a number.
Plain torch: it works on CPU tensors as well."""
from __future__ import annotations

import math
from typing import Dict, Hashable, Iterator, List, Optional, Sequence, Tuple

import torch

HeadSpec = Tuple[str, Hashable, int, int, float]  # (key, group id, K, col0, base lr)


def cosine_factor(step: int, max_iter: Optional[int]) -> float:
    """CosineAnnealingLR(max_iter, eta_min=0) in closed form (fp64): the rate of optimizer step `step` (0-based) over its base"""
    return 1.0 if max_iter is None else 0.5 * (1.0 + math.cos(math.pi * step / max_iter))


class HeadGroup:
    """the H heads that share one input, the contiguous column slice [col0, col0 + K) of X_all: weight [H, C, K], bias [H, C], their
    momentum buffers m_weight / m_bias and lr [H], contiguous fp32; `off` is the group's first position in the store's `keys`"""

    def __init__(self, gid: Hashable, K: int, col0: int):
        self.id, self.K, self.col0 = gid, int(K), int(col0)
        self.keys: List[str] = []
        self.base_lr: List[float] = []


class HeadStore:
    """heads: (key, group id, K, col0, base lr) with unique keys; init: key -> (weight [C, K], bias [C]) host tensors.  Groups stand in
    the order their ids first appear and `keys` lists the heads group by group: the order of every per-head vector."""

    def __init__(self, heads: Sequence[HeadSpec], init: Dict[str, Tuple[torch.Tensor, torch.Tensor]], device,
                 max_iter: Optional[int] = None):
        self.max_iter = max_iter
        self.groups: List[HeadGroup] = []
        for key, gid, K, col0, lr in heads:
            g = next((g for g in self.groups if g.id == gid), None)
            if g is None:
                g = HeadGroup(gid, K, col0)
                self.groups.append(g)
            g.keys.append(key)
            g.base_lr.append(float(lr))
        self.keys: List[str] = []
        f32 = dict(device=device, dtype=torch.float32)
        for g in self.groups:
            g.H, g.off = len(g.keys), len(self.keys)
            self.keys += g.keys
            g.weight = torch.stack([init[k][0] for k in g.keys]).to(**f32).contiguous()
            g.bias = torch.stack([init[k][1] for k in g.keys]).to(**f32).contiguous()
            g.m_weight, g.m_bias = torch.zeros_like(g.weight), torch.zeros_like(g.bias)
            g.lr = torch.zeros(g.H, **f32)

    def learning_rates(self, step: int) -> Dict[str, float]:
        """key -> the rate of optimizer step `step` (fp64)"""
        f = cosine_factor(step, self.max_iter)
        return {k: lr * f for g in self.groups for k, lr in zip(g.keys, g.base_lr)}

    def set_lr(self, g: HeadGroup, factor: float) -> None:
        """g.lr = base rate * factor, the fp64 product rounded to fp32"""
        g.lr.copy_(torch.tensor([lr * factor for lr in g.base_lr], dtype=torch.float64).to(torch.float32))

    def entries(self) -> Iterator[Tuple[str, str, torch.Tensor, torch.Tensor]]:
        """(key, "weight" | "bias", parameter view, momentum view) of every head in the order of `keys`, weight before bias"""
        for g in self.groups:
            for i, k in enumerate(g.keys):
                yield k, "weight", g.weight[i], g.m_weight[i]
                yield k, "bias", g.bias[i], g.m_bias[i]
