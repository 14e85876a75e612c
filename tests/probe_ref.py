"""Helper of the linear-probe tests (not a test): an fp64 torch restatement of one step of the probe sweep -- a linear layer per head,
mean cross-entropy, SGD with momentum (dampening 0, no weight decay), cosine annealing in closed form -- and of the rule that names
the heads of a sweep and resolves equal names.  tests/test_probe_host.py checks it against the real tool where the reference tree
is present; tests/test_probe_gpu.py checks the kernels against it."""
import math

import torch

F64 = torch.float64


def sweep(n_blocks_list, learning_rates, batch_size, world):
    """[(key, n_blocks, avgpool, scaled lr)] of a sweep after equal keys are resolved: dict semantics, the later head replaces the
    earlier one in the earlier one's position"""
    heads = {}
    for n in n_blocks_list:
        for base in learning_rates:
            lr = base * batch_size * world / 256.0
            key = "classifier_%d_blocks_avgpool_True_lr_%s" % (n, ("%.5f" % lr).replace(".", "_"))
            heads[key] = (key, n, True, lr)
    return list(heads.values())


def cosine_lr(base, step, max_iter):
    """learning rate of optimizer step `step` (0-based) under cosine annealing to 0 over max_iter steps; None = constant"""
    return base if max_iter is None else base * 0.5 * (1.0 + math.cos(math.pi * step / max_iter))


def head_input(x_all, n_max, D, n, avgpool):
    """columns of X_all = [cls of block -n_max .. cls of block -1 | mean patch token of the last block] that a head reads"""
    c0 = (n_max - n) * D
    return x_all[:, c0:c0 + (n + (1 if avgpool else 0)) * D]


def x_all_of(features, n_max):
    """X_all from the trunk's ((patch tokens, cls token), ...) outputs"""
    last = list(features)[-n_max:]
    return torch.cat([c for _, c in last] + [last[-1][0].mean(dim=1)], dim=-1)


class RefProbe:
    """heads: [(key, n_blocks, avgpool, lr)] with unique keys; weights: key -> (W [C, in], b [C])"""

    def __init__(self, heads, weights, D, momentum=0.9, max_iter=None, dtype=F64):
        self.heads, self.D, self.momentum, self.max_iter, self.dtype = list(heads), D, momentum, max_iter, dtype
        self.n_max = max(h[1] for h in self.heads)
        self.W = {k: weights[k][0].detach().cpu().to(dtype).clone() for k, *_ in self.heads}
        self.b = {k: weights[k][1].detach().cpu().to(dtype).clone() for k, *_ in self.heads}
        self.mW = {k: torch.zeros_like(v) for k, v in self.W.items()}
        self.mb = {k: torch.zeros_like(v) for k, v in self.b.items()}
        self.steps = 0

    def logits(self, x_all):
        x_all = x_all.detach().cpu().to(self.dtype)
        return {k: head_input(x_all, self.n_max, self.D, n, ap) @ self.W[k].T + self.b[k] for k, n, ap, _ in self.heads}

    @staticmethod
    def _ce(z, y):
        logp = torch.log_softmax(z, dim=1)
        return -logp[torch.arange(z.shape[0]), y].mean(), logp

    def step(self, x_all, labels):
        """one optimizer step of every head; returns key -> loss (before the step)"""
        x_all, y = x_all.detach().cpu().to(self.dtype), labels.detach().cpu().long()
        B = x_all.shape[0]
        losses = {}
        for k, n, ap, base in self.heads:
            x = head_input(x_all, self.n_max, self.D, n, ap)
            loss, logp = self._ce(x @ self.W[k].T + self.b[k], y)
            dz = logp.exp()
            dz[torch.arange(B), y] -= 1.0
            dz /= B
            lr = cosine_lr(base, self.steps, self.max_iter)
            for p, m, g in ((self.W[k], self.mW[k], dz.T @ x), (self.b[k], self.mb[k], dz.sum(0))):
                m.mul_(self.momentum).add_(g)
                p.sub_(lr * m)
            losses[k] = float(loss)
        self.steps += 1
        return losses

    def evaluate(self, x_all, labels):
        """key -> number of rows whose first maximum is the label"""
        y = labels.detach().cpu().long()
        return {k: int((z.argmax(dim=1) == y).sum()) for k, z in self.logits(x_all).items()}


def gamma(n):
    """a-priori relative bound of n fp32 roundings in a chain: n u / (1 - n u), u = 2^-24"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)
