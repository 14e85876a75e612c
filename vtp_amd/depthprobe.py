"""Linear monocular-depth probe on frozen patch tokens: one linear layer per head whose outputs are `n_bins` uniform bins of depth
over [min_depth, max_depth], its low-resolution logit map upsampled bilinearly to the label map, AdaBins' "linear normalisation"
(a_c = max(z_c, 0) + 0.1, depth = sum_c a_c e_c / sum_c a_c) and the scale-invariant log loss of Eigen et al. -- the "lin." depth
evaluation the DINOv2 / DINOv3 papers report beside k-NN, linear classification and linear segmentation, restated from the papers'
description.  Parity with the DINOv2 depth code or the Monocular-Depth-Estimation-Toolbox is UNPINNED, and three things differ from
those programs: they put a BatchNorm in front of the linear layer (none here); they upsample the features x 4 and resize the
predicted depth (here the logits are interpolated straight to the label size and normalised there); they train with AdamW (here it
is the probes' SGD + cosine).  The arithmetic is pinned by an fp64 restatement checked against torch's own CPU ops
(tests/depth_ref.py).

Per feature group: ONE exact-fp32 logits GEMM over all heads at the low resolution (vtp_probe_logits), ONE pixel pass that
interpolates each pixel's logits from LDS-staged cells (depth, log residual, fp64 loss statistics), ONE gather pass for the gradient
of the low-resolution logits and ONE sliced weight-gradient + SGD-momentum step (csrc/depthprobe.hip; the weight step is
SegProbe's).  Nothing of size [B, n_bins, Hl, Wl] exists and nothing is summed with atomics: a step repeats bit for bit.

    probe = DepthProbe(model, [("depth_1_lr_0_01", 1, 0.01), ("depth_4_lr_0_01", 4, 0.01)], max_iter=iters)
    losses = probe.step(images, depth)             # device f32 [heads]; depth f32 [B, Hl, Wl] in metres, 0 = no measurement
    probe.evaluate(images, depth); probe.metrics(); probe.best()
    pred = probe.predict(images, (Ho, Wo))         # f32 [heads, B, Ho, Wo]

A pixel counts iff 0 < depth <= max_depth (NaN and inf do not): crops (Eigen, Garg) are the caller's, who zeroes the pixels outside.
There is no CPU path: tensors on the CPU raise.  Training is single-process; evaluation sums its counters over a process group."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .banks import Group, Workspace, eval_device
from .heads import HeadGroup, HeadStore, cosine_factor

Head = Tuple[str, int, float]  # (key, use_n_blocks, lr)
SGD_WORKSPACE_BOUND = 64 << 20  # bytes of weight-gradient slices per launch; a group whose heads need more is stepped in chunks of heads
METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "silog", "d1", "d2", "d3", "valid")


def metrics_from_counters(counts: torch.Tensor, sums: torch.Tensor) -> Dict[str, float]:
    """counts int64 [4] = (valid, d1, d2, d3 hits), sums fp64 [6] = sums over the valid pixels of (g, g^2, |d - gt| / gt,
    (d - gt)^2 / gt, (d - gt)^2, |g| / ln 10) with g = log d - log gt -> the metrics, in fp64 on the host"""
    n = int(counts[0])
    if n == 0:
        raise RuntimeError("nothing evaluated yet (no valid pixel)")
    s = [float(v) / n for v in sums.tolist()]
    return {"abs_rel": s[2], "sq_rel": s[3], "rmse": math.sqrt(s[4]), "rmse_log": math.sqrt(s[1]), "log10": s[5],
            "silog": 100.0 * math.sqrt(max(s[1] - s[0] * s[0], 0.0)), "d1": int(counts[1]) / n, "d2": int(counts[2]) / n,
            "d3": int(counts[3]) / n, "valid": n}


class DepthProbe:
    """heads: (key, use_n_blocks, lr) tuples with unique keys; heads with equal use_n_blocks form a group and are stored stacked
    (heads.HeadStore: weight [H, n_bins, K], bias [H, n_bins] and their momentum buffers, contiguous fp32; normal_(0, 0.01) weights and
    zero biases drawn on the host in creation order).  `keys` lists the heads group by group: the order of every per-head vector.
    cls_concat appends each block's class token to every one of its patch tokens (K = 2 D per block).  model may be None when only
    the *_features methods are used (then pass embed_dim)."""

    def __init__(self, model, heads: Sequence[Head], min_depth: float = 0.001, max_depth: float = 10.0, n_bins: int = 256,
                 lam: float = 0.85, momentum: float = 0.9, max_iter: Optional[int] = None, group=None, *, cls_concat: bool = False,
                 embed_dim: Optional[int] = None, device=None):
        self.device = eval_device("DepthProbe", model, device)
        self.model = model
        self.D = int(embed_dim if embed_dim is not None else model.config.vision_embed_dim)
        if self.D % 4:
            raise ValueError(f"embed_dim must be a multiple of 4 (16-byte column slices), got {self.D}")
        if not 2 <= int(n_bins) <= 1024:
            raise ValueError(f"n_bins must be in [2, 1024], got {n_bins}")
        if not 0.0 < float(min_depth) < float(max_depth) < math.inf:
            raise ValueError(f"need 0 < min_depth < max_depth, got {min_depth}, {max_depth}")
        if max_iter is not None and max_iter < 1:
            raise ValueError("max_iter must be >= 1 (or None for constant learning rates)")
        self.C, self.min_depth, self.max_depth, self.lam = int(n_bins), float(min_depth), float(max_depth), float(lam)
        self.momentum, self.max_iter, self.cls_concat = float(momentum), max_iter, bool(cls_concat)
        self.Dc = 2 * self.D if self.cls_concat else self.D
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
            init[key] = (torch.empty(self.C, n * self.Dc).normal_(mean=0.0, std=0.01), torch.zeros(self.C))
        # a group reads the last n blocks: the trailing n Dc columns of X_all
        self.heads = HeadStore([(key, n, n * self.Dc, (self.n_max - n) * self.Dc, lr) for key, n, lr in heads], init, self.device, max_iter)
        del init
        self.groups, self.keys = self.heads.groups, self.heads.keys
        self.steps = 0
        self.head_chunk: Optional[int] = None  # heads per weight-step launch; None: as many as SGD_WORKSPACE_BOUND allows
        self._ws_pix, self._ws_aux, self._ws_sgd = Workspace(self.device), Workspace(self.device), Workspace(self.device)
        self._stats = torch.zeros(len(self.keys), 4, device=self.device, dtype=torch.float64)  # (n, m1, m2, L) of the last call
        self._counts = torch.zeros(len(self.keys), 4, device=self.device, dtype=torch.int64)
        self._sums = torch.zeros(len(self.keys), 6, device=self.device, dtype=torch.float64)

    # ------------------------------------------------------------------------------------------------ inputs
    def features(self, images: torch.Tensor) -> torch.Tensor:
        """X_all f32 [B h w, n_max Dc] with (h, w) = the image size over the patch size 16: the patch tokens of the last n_max
        blocks, each through the trunk's final norm, in ascending block order; with cls_concat every patch token is followed by its
        block's class token (patch then cls, Dc = 2 D)"""
        if self.model is None:
            raise RuntimeError("DepthProbe was built without a model: use the *_features methods")
        outs = self.model.get_intermediate_layers_feature(images, n=self.n_max, norm=True, return_class_token=self.cls_concat)
        cols = []
        for o in outs:
            patch, cls_t = o if self.cls_concat else (o, None)
            B, T, D = patch.shape
            cols.append(patch.reshape(B * T, D))
            if cls_t is not None:
                cols.append(cls_t[:, None, :].expand(B, T, D).reshape(B * T, D))
        return torch.cat(cols, dim=1)

    @staticmethod
    def _hw(images: torch.Tensor) -> Tuple[int, int]:
        return images.shape[-2] // 16, images.shape[-1] // 16

    def _features(self, x_all: torch.Tensor, hw, B: int):
        h, w = int(hw[0]), int(hw[1])
        x = x_all.detach().to(torch.float32)
        if x.dim() != 2 or h < 1 or w < 1 or tuple(x.shape) != (B * h * w, self.n_max * self.Dc):
            raise ValueError(f"features must be [B h w, n_max Dc] = [{B * h * w}, {self.n_max * self.Dc}], got {tuple(x_all.shape)}")
        if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
            x = x.contiguous()
        return x, (h, w)

    def _inputs(self, x_all: torch.Tensor, hw, labels: torch.Tensor):
        for name, t in (("features", x_all), ("labels", labels)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"{name} must live on the MI355X (got a CPU tensor): there is no CPU path")
        if not labels.is_floating_point() or labels.dim() != 3 or min(labels.shape) < 1:
            raise ValueError(f"labels must be floating-point depth [B, Hl, Wl], got {labels.dtype} {tuple(labels.shape)}")
        x, hw = self._features(x_all, hw, labels.shape[0])
        return x, hw, labels.detach().to(torch.float32).contiguous()

    def _head_chunk(self, g: HeadGroup, M: int) -> int:
        if self.head_chunk is not None:
            return max(1, min(g.H, int(self.head_chunk)))
        per_head = ops.depth_sgd_workspace_bytes(M, self.C, g.K)
        return max(1, min(g.H, SGD_WORKSPACE_BOUND // per_head))

    def _logits(self, g: HeadGroup, x: torch.Tensor, M: int) -> torch.Tensor:
        z = torch.empty(M, g.H * self.C, device=self.device, dtype=torch.float32)
        ops.probe_logits(x[:, g.col0:g.col0 + g.K], g.weight, g.bias, z, M, g.H * self.C, g.K)
        return z

    def _range(self):
        return self.min_depth, self.max_depth, self.lam

    # ------------------------------------------------------------------------------------------------ training
    def learning_rates(self, step: Optional[int] = None) -> Dict[str, float]:
        return self.heads.learning_rates(self.steps if step is None else step)

    def step(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self.step_features(self.features(images), self._hw(images), labels)

    def step_features(self, x_all: torch.Tensor, hw, labels: torch.Tensor) -> torch.Tensor:
        """one optimizer step of every head on X_all [B h w, n_max Dc] and labels [B, Hl, Wl]; returns the per-head losses (device
        f32, order of `keys`, no host sync).  Without a valid pixel the loss and the gradient are 0 and the momentum still decays."""
        if self.world > 1:
            raise NotImplementedError("Training is single-process in this pull request.")
        x, (h, w), y = self._inputs(x_all, hw, labels)
        B, Hl, Wl = y.shape
        M, C = B * h * w, self.C
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        f = cosine_factor(self.steps, self.max_iter)
        for g in self.groups:
            self.heads.set_lr(g, f)
            xs = x[:, g.col0:g.col0 + g.K]
            z = self._logits(g, x, M)
            grad = torch.empty(M, g.H * C, device=self.device, dtype=torch.float32)
            ws = self._ws_pix.at_least(ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, g.H, C))
            aux = self._ws_aux.at_least(ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, g.H, C, aux=True))
            stats = self._stats[g.off:g.off + g.H]
            ops.depth_pix(z, y, (h, w), g.H, C, *self._range(), aux=aux, loss=losses[g.off:g.off + g.H], stats=stats, workspace=ws)
            ops.depth_dlogits(z, (B, Hl, Wl), (h, w), g.H, C, *self._range(), aux, stats, grad)
            step = self._head_chunk(g, M)
            for lo in range(0, g.H, step):  # the chunking bounds the workspace and changes no bit of the result
                n = min(step, g.H - lo)
                ws = self._ws_sgd.at_least(ops.depth_sgd_workspace_bytes(M, n * C, g.K))
                ops.depth_sgd(g.weight[lo:lo + n], g.bias[lo:lo + n], g.m_weight[lo:lo + n], g.m_bias[lo:lo + n], grad[:, lo * C:], xs,
                              g.lr[lo:lo + n], M, n, C, g.K, self.momentum, ws)
        self.steps += 1
        return losses

    # ------------------------------------------------------------------------------------------------ evaluation
    def evaluate(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self.evaluate_features(self.features(images), self._hw(images), labels)

    def evaluate_features(self, x_all: torch.Tensor, hw, labels: torch.Tensor) -> torch.Tensor:
        """adds this batch to the evaluation counters (depth predicted at the labels' own size, invalid pixels skipped); returns its
        per-head losses (device f32, no host sync)"""
        x, (h, w), y = self._inputs(x_all, hw, labels)
        B, Hl, Wl = y.shape
        M, C = B * h * w, self.C
        losses = torch.zeros(len(self.keys), device=self.device, dtype=torch.float32)
        for g in self.groups:
            ws = self._ws_pix.at_least(ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, g.H, C))
            ops.depth_pix(self._logits(g, x, M), y, (h, w), g.H, C, *self._range(), loss=losses[g.off:g.off + g.H],
                          stats=self._stats[g.off:g.off + g.H], workspace=ws, eval_counts=self._counts[g.off:g.off + g.H],
                          eval_sums=self._sums[g.off:g.off + g.H])
        return losses

    def predict(self, images: torch.Tensor, out_hw) -> torch.Tensor:
        return self.predict_features(self.features(images), self._hw(images), out_hw)

    def predict_features(self, x_all: torch.Tensor, hw, out_hw) -> torch.Tensor:
        """f32 [heads, B, Ho, Wo]: the depth of every head (order of `keys`) at out_hw = (Ho, Wo), in [min_depth, max_depth]"""
        if not isinstance(x_all, torch.Tensor) or not x_all.is_cuda:
            raise ValueError("features must live on the MI355X (got a CPU tensor): there is no CPU path")
        h, w = int(hw[0]), int(hw[1])
        Ho, Wo = int(out_hw[0]), int(out_hw[1])
        if h < 1 or w < 1 or Ho < 1 or Wo < 1 or x_all.dim() != 2 or x_all.shape[0] % (h * w):
            raise ValueError(f"features must be [B h w, n_max Dc] and out_hw >= 1, got {tuple(x_all.shape)}, hw {hw}, out_hw {out_hw}")
        B = x_all.shape[0] // (h * w)
        x, _ = self._features(x_all, (h, w), B)
        out = torch.empty(len(self.keys), B, Ho, Wo, device=self.device, dtype=torch.float32)
        for g in self.groups:
            ops.depth_pix(self._logits(g, x, B * h * w), None, (h, w), g.H, self.C, *self._range(), out_hw=(Ho, Wo),
                          dhat=out[g.off:g.off + g.H])
        return out

    def counters(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(int64 [heads, 4], fp64 [heads, 6]) on the host, summed over the process group with one all-reduce (the counts travel as
        fp64: exact below 2^53 pixels)"""
        nh = len(self.keys)
        flat = self._group.summed(torch.cat([self._counts.to(torch.float64).reshape(-1), self._sums.reshape(-1)])).cpu()
        return flat[:4 * nh].view(nh, 4).to(torch.int64), flat[4 * nh:].view(nh, 6)

    def metrics(self) -> Dict[str, Dict[str, float]]:
        """key -> {abs_rel, sq_rel, rmse, rmse_log, log10, silog (= 100 sqrt(m2 - m1^2) over everything evaluated), d1, d2, d3, valid}"""
        counts, sums = self.counters()
        return {k: metrics_from_counters(counts[i], sums[i]) for i, k in enumerate(self.keys)}

    def best(self) -> Tuple[str, float]:
        """the head with the lowest rmse"""
        m = {k: v["rmse"] for k, v in self.metrics().items()}
        key = min(m, key=m.get)
        return key, m[key]

    def reset_eval(self) -> None:
        self._counts.zero_()
        self._sums.zero_()

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
