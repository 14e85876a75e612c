"""Linear probing on frozen trunk features (reference: tools/test_linear_probing_hf.py) with every classifier of the sweep on the
project's kernels: per feature group ONE exact-fp32 logits GEMM over all heads, ONE cross-entropy kernel and ONE fused
weight-gradient + SGD-momentum kernel (csrc/probe.hip) -- no nn.Linear, no autograd, no torch.optim.

    probe = LinearProbe.from_sweep(model, max_iter=epochs * epoch_length)      # setup_linear_classifiers + SGD + CosineAnnealingLR
    losses = probe.step(images, labels)                                        # device f32 [heads]; the tool prints their sum
    probe.evaluate(images, labels); probe.accuracies(); probe.best()

There is no CPU path: tensors on the CPU raise."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .banks import Group, eval_device
from .heads import HeadGroup, HeadStore, cosine_factor

DEFAULT_LEARNING_RATES = (1e-5, 2e-5, 5e-5, 1e-4, 2e-4, 5e-4, 1e-3, 2e-3, 5e-3, 1e-2, 2e-2, 5e-2, 0.1)  # the tool's sweep (:61-64)
Head = Tuple[str, int, bool, float]  # (key, use_n_blocks, use_avgpool, lr)


def sweep_heads(n_last_blocks_list: Sequence[int] = (1, 4), learning_rates: Sequence[float] = DEFAULT_LEARNING_RATES,
                batch_size: int = 128, world: int = 1) -> List[Head]:
    """setup_linear_classifiers (:221-254) as a head list, in creation order and BEFORE key collisions are resolved: the learning
    rate is scaled by batch_size * world / 256 (scale_lr, :216-218), use_avgpool is always True, and the key prints the scaled
    rate with five decimals -- so two small rates can share a key (1e-5 and 2e-5 at batch 128 on one GPU both print 0_00001)."""
    heads = []
    for n in n_last_blocks_list:
        for avgpool in (True,):
            for base in learning_rates:
                lr = base * (batch_size * world) / 256.0
                heads.append((f"classifier_{n}_blocks_avgpool_{avgpool}_lr_{lr:.5f}".replace(".", "_"), int(n), avgpool, lr))
    return heads


def resolve_heads(heads: Sequence[Head]) -> List[Head]:
    """nn.ModuleDict semantics on a key collision: the later head takes the place (position included) of the earlier one, which the
    reference then neither trains nor evaluates"""
    by_key: Dict[str, Head] = {}
    for h in heads:
        by_key[h[0]] = (h[0], int(h[1]), bool(h[2]), float(h[3]))
    return list(by_key.values())


def init_heads(heads: Sequence[Head], embed_dim: int, num_classes: int) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """host initialisation in creation order, consuming the generator exactly as LinearClassifier.__init__ (:155-162) does --
    nn.Linear's own init first, then weight.normal_(0, 0.01) and a zero bias -- for EVERY head, a replaced one included, so that
    the kept heads equal the reference's under the same torch.manual_seed.  Returns key -> (weight [C, in], bias [C]) of the
    heads that survive."""
    out = {}
    for key, n, avgpool, _ in heads:
        lin = torch.nn.Linear((n + (1 if avgpool else 0)) * embed_dim, num_classes)
        lin.weight.data.normal_(mean=0.0, std=0.01)
        out[key] = (lin.weight.data, torch.zeros(num_classes))
    return out


class LinearProbe:
    """heads: (key, use_n_blocks, use_avgpool, lr) tuples; heads with equal (use_n_blocks, use_avgpool) form a feature group and
    are stored stacked (heads.HeadStore: weight [H, C, in], bias [H, C] and their momentum buffers, contiguous fp32).  `keys` lists
    the heads group by group, which is the order of every per-head vector (losses, counts); for a sweep it is the reference's order.
    model may be None when only step_features / evaluate_features are used (then pass embed_dim)."""

    def __init__(self, model, heads: Sequence[Head], num_classes: int, momentum: float = 0.9, max_iter: Optional[int] = None,
                 group=None, *, embed_dim: Optional[int] = None, device=None):
        self.device = eval_device("LinearProbe", model, device)
        self.model = model
        self.D = int(embed_dim if embed_dim is not None else model.config.vision_embed_dim)
        if self.D % 4:
            raise ValueError(f"embed_dim must be a multiple of 4 (16-byte column slices), got {self.D}")
        if max_iter is not None and max_iter < 1:
            raise ValueError("max_iter must be >= 1 (or None for constant learning rates)")
        self.C, self.momentum, self.max_iter, self.group = int(num_classes), float(momentum), max_iter, group
        self._group = Group(group)
        self.world, self.rank = self._group.world, self._group.rank
        heads = list(heads)
        kept = resolve_heads(heads)
        if not kept:
            raise ValueError("no heads")
        init = init_heads(heads, self.D, self.C)
        self.n_max = max(h[1] for h in kept)
        for key, n, _, _ in kept:
            if n < 1:
                raise ValueError(f"{key}: use_n_blocks must be >= 1")
        # a group reads the class tokens of its last n blocks and, with avgpool, the pooled patch tokens behind them
        self.heads = HeadStore([(key, (n, avgpool), (n + (1 if avgpool else 0)) * self.D, (self.n_max - n) * self.D, lr)
                                for key, n, avgpool, lr in kept], init, self.device, max_iter)
        del init
        self.groups, self.keys = self.heads.groups, self.heads.keys
        for g in self.groups:
            g.buf = {}
        self.steps = 0
        self._correct = torch.zeros(len(self.keys), device=self.device, dtype=torch.int32)
        self._total = 0

    @classmethod
    def from_sweep(cls, model, n_last_blocks_list: Sequence[int] = (1, 4), learning_rates: Sequence[float] = DEFAULT_LEARNING_RATES,
                   batch_size: int = 128, num_classes: int = 1000, world: int = 1, **kw):
        """the tool's setup_linear_classifiers + optimizer parameter groups (:221-254, :487)"""
        return cls(model, sweep_heads(n_last_blocks_list, learning_rates, batch_size, world), num_classes, **kw)

    # ------------------------------------------------------------------------------------------------ inputs
    def features(self, images: torch.Tensor):
        if self.model is None:
            raise RuntimeError("LinearProbe was built without a model: use step_features / evaluate_features")
        return self.model.get_intermediate_layers_feature(images, n=self.n_max, return_class_token=True)

    def input_matrix(self, features) -> torch.Tensor:
        """X_all f32 [B, (n_max + 1) D] = [cls of block -n_max ... cls of block -1 | mean of the last block's patch tokens]: the
        input of every group (create_linear_input, :137-152) is a contiguous column slice of it.  A ready matrix passes through."""
        if torch.is_tensor(features):
            x = features
        else:
            last = list(features)[-self.n_max:]
            if len(last) != self.n_max:
                raise ValueError(f"need the outputs of the last {self.n_max} blocks, got {len(features)}")
            x = torch.cat([c for _, c in last] + [torch.mean(last[-1][0], dim=1)], dim=-1)
        if not x.is_cuda:
            raise ValueError("features must live on the MI355X (got a CPU tensor): there is no CPU path")
        x = x.detach().to(torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != (self.n_max + 1) * self.D:
            raise ValueError(f"input matrix must be [B, {(self.n_max + 1) * self.D}], got {tuple(x.shape)}")
        return x

    def _labels(self, labels: torch.Tensor, B: int) -> torch.Tensor:
        if not labels.is_cuda:
            raise ValueError("labels must live on the MI355X (got a CPU tensor)")
        if labels.is_floating_point() or labels.shape != (B,):
            raise ValueError(f"labels must be {B} integer class indices, got {labels.dtype} {tuple(labels.shape)}")
        return labels.detach().to(torch.int64).contiguous()

    def _bufs(self, g: HeadGroup, B: int):
        if B not in g.buf:
            f32 = dict(device=self.device, dtype=torch.float32)
            g.buf = {B: (torch.empty(B, g.H * self.C, **f32), torch.empty(B, g.H * self.C, **f32),
                         torch.empty(B * self.world, g.H * self.C, **f32) if self.world > 1 else None)}
        return g.buf[B]

    # ------------------------------------------------------------------------------------------------ training
    def learning_rates(self, step: Optional[int] = None) -> Dict[str, float]:
        return self.heads.learning_rates(self.steps if step is None else step)

    def step(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self.step_features(self.features(images), labels)

    def step_features(self, features, labels: torch.Tensor) -> torch.Tensor:
        """one optimizer step of every head (train_one_epoch's loop body, :282-291); returns the per-head losses (device f32, order
        of `keys`, no host sync).  With a process group: features / labels are this rank's rows, the losses the global means."""
        x = self.input_matrix(features)
        B = x.shape[0]
        y = self._labels(labels, B)
        x_all = x
        if self.world > 1:  # DDP's gradient mean, without a dW to reduce: every rank runs the same full-batch update
            x_all = torch.empty(B * self.world, x.shape[1], device=self.device, dtype=torch.float32)
            self._group.all_gather_rows(x_all, x)
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        f = cosine_factor(self.steps, self.max_iter)
        for g in self.groups:
            N = g.H * self.C
            logits, dlogits, dl_all = self._bufs(g, B)
            self.heads.set_lr(g, f)
            xs = x[:, g.col0:g.col0 + g.K]
            ops.probe_logits(xs, g.weight, g.bias, logits, B, N, g.K)
            ops.probe_ce(logits, y, B, g.H, self.C, 1.0 / (B * self.world), losses[g.off:g.off + g.H], None, dlogits)
            if self.world > 1:
                self._group.all_gather_rows(dl_all, dlogits)
                dlogits = dl_all
            ops.probe_sgd(g.weight, g.bias, g.m_weight, g.m_bias, dlogits, x_all[:, g.col0:g.col0 + g.K], g.lr, B * self.world, g.H,
                          self.C, g.K, self.momentum)
        if self.world > 1:
            self._group.dist.all_reduce(losses, group=self.group)
        self.steps += 1
        return losses

    # ------------------------------------------------------------------------------------------------ evaluation
    def evaluate(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self.evaluate_features(self.features(images), labels)

    def evaluate_features(self, features, labels: torch.Tensor) -> torch.Tensor:
        """adds this batch to the top-1 counts (evaluate, :303-330); returns its per-head mean losses (device f32)"""
        x = self.input_matrix(features)
        B = x.shape[0]
        y = self._labels(labels, B)
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        for g in self.groups:
            logits = self._bufs(g, B)[0]
            ops.probe_logits(x[:, g.col0:g.col0 + g.K], g.weight, g.bias, logits, B, g.H * self.C, g.K)
            ops.probe_ce(logits, y, B, g.H, self.C, 1.0 / B, losses[g.off:g.off + g.H], self._correct[g.off:g.off + g.H], None)
        self._total += B
        return losses

    def counts(self) -> Tuple[torch.Tensor, int]:
        """(correct per head as a CPU int64 tensor, rows seen), summed over the process group with one all-reduce"""
        c = torch.cat([self._correct.to(torch.int64), torch.tensor([self._total], device=self.device, dtype=torch.int64)])
        c = self._group.summed(c).cpu()
        return c[:-1], int(c[-1])

    def accuracies(self) -> Dict[str, float]:
        """key -> top-1 accuracy in percent (:332-345)"""
        correct, total = self.counts()
        if total == 0:
            raise RuntimeError("accuracies(): nothing evaluated yet")
        return {k: 100.0 * int(c) / total for k, c in zip(self.keys, correct)}

    def best(self) -> Tuple[str, float]:
        acc = self.accuracies()
        key = max(acc, key=acc.get)
        return key, acc[key]

    def reset_eval(self):
        self._correct.zero_()
        self._total = 0

    # ------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """the reference's AllClassifiers layout (classifiers_dict.<key>.linear.weight | bias); momentum buffers and the step count
        under the prefix `probe.`"""
        sd = {f"classifiers_dict.{k}.linear.{p}": param.clone() for k, p, param, _ in self.heads.entries()}
        sd.update({f"probe.momentum.{k}.{p}": mom.clone() for k, p, _, mom in self.heads.entries()})
        sd["probe.steps"] = torch.tensor(self.steps, dtype=torch.int64)
        return sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        """accepts a checkpoint of the reference's AllClassifiers (also saved through DDP: leading `module.`); without `probe.*`
        entries the momentum buffers are zeroed and the step count restarts"""
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        want = {f"classifiers_dict.{k}.linear.{p}" for k in self.keys for p in ("weight", "bias")}
        have = {k for k in sd if k.startswith("classifiers_dict.")}
        if want != have:
            raise KeyError(f"load_state_dict: missing {sorted(want - have)}, unexpected {sorted(have - want)}")
        for k, p, param, mom in self.heads.entries():
            src = sd[f"classifiers_dict.{k}.linear.{p}"]
            if src.shape != param.shape:
                raise ValueError(f"{k}.linear.{p}: shape {tuple(src.shape)}, expected {tuple(param.shape)}")
            param.copy_(src)
            m = sd.get(f"probe.momentum.{k}.{p}")
            if m is None:
                mom.zero_()
            else:
                mom.copy_(m)
        self.steps = int(sd["probe.steps"]) if "probe.steps" in sd else 0
