"""What the dense probes (segprobe.SegProbe, depthprobe.DepthProbe) share: linear heads on the patch-token map of the last trunk
blocks, stored stacked per feature group (heads.HeadStore), the feature matrix and its checks, the exact-fp32 logits GEMM at the low
resolution, the sliced weight-gradient + SGD-momentum step in chunks of heads, the cosine schedule and the checkpoint.  A subclass
adds its labels, the pixel and cell passes between the logits and the weight step, and its counters and metrics."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .banks import Group, Workspace, eval_device
from .heads import HeadGroup, HeadStore

Head = Tuple[str, int, float]  # (key, use_n_blocks, lr)
SGD_WORKSPACE_BOUND = 64 << 20  # bytes of weight-gradient slices per launch; a group whose heads need more is stepped in chunks of heads


class DenseProbe:
    """heads: (key, use_n_blocks, lr) tuples with unique keys; heads with equal use_n_blocks form a group and are stored stacked
    (heads.HeadStore: weight [H, C, K], bias [H, C] and their momentum buffers, contiguous fp32; normal_(0, 0.01) weights and zero
    biases drawn on the host in creation order).  `keys` lists the heads group by group: the order of every per-head vector."""

    _COLS = "n_max D"  # the columns of X_all, as the messages name them
    _FEATURE_METHODS = "the *_features methods"
    _sgd = staticmethod(ops.seg_sgd)  # the weight step's entry point: its bound on C is the subclass's
    _sgd_workspace_bytes = staticmethod(ops.seg_sgd_workspace_bytes)

    def __init__(self, model, heads: Sequence[Head], n_out: int, momentum: float, max_iter: Optional[int], group, cls_concat: bool,
                 embed_dim: Optional[int], device):
        self.device = eval_device(type(self).__name__, model, device)
        self.model = model
        self.D = int(embed_dim if embed_dim is not None else model.config.vision_embed_dim)
        if self.D % 4:
            raise ValueError(f"embed_dim must be a multiple of 4 (16-byte column slices), got {self.D}")
        if max_iter is not None and max_iter < 1:
            raise ValueError("max_iter must be >= 1 (or None for constant learning rates)")
        self.C, self.momentum, self.max_iter, self.cls_concat = int(n_out), float(momentum), max_iter, bool(cls_concat)
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
        self._ws_sgd = Workspace(self.device)

    # ------------------------------------------------------------------------------------------------ inputs
    def features(self, images: torch.Tensor) -> torch.Tensor:
        """X_all f32 [B h w, n_max Dc] with (h, w) = the image size over the patch size 16: the patch tokens (no class token) of the
        last n_max blocks, each through the trunk's final norm, in ascending block order; with cls_concat every patch token is
        followed by its block's class token (patch then cls, Dc = 2 D); in exact fp32 where the model's enable_fp32_forward covers
        the trunk"""
        if self.model is None:
            raise RuntimeError(f"{type(self).__name__} was built without a model: use {self._FEATURE_METHODS}")
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

    @staticmethod
    def _on_device(**tensors) -> None:
        for name, t in tensors.items():
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"{name} must live on the MI355X (got a CPU tensor): there is no CPU path")

    def _features(self, x_all: torch.Tensor, hw, B: int):
        h, w = int(hw[0]), int(hw[1])
        x = x_all.detach().to(torch.float32)
        if x.dim() != 2 or h < 1 or w < 1 or tuple(x.shape) != (B * h * w, self.n_max * self.Dc):
            raise ValueError(f"features must be [B h w, {self._COLS}] = [{B * h * w}, {self.n_max * self.Dc}], got {tuple(x_all.shape)}")
        if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
            x = x.contiguous()
        return x, (h, w)

    def _labels(self, labels: torch.Tensor) -> torch.Tensor:
        """the subclass's: refuses labels that are not its kind of [B, Hl, Wl] map, returns them as the kernels read them"""
        raise NotImplementedError

    def _inputs(self, x_all: torch.Tensor, hw, labels: torch.Tensor):
        self._on_device(features=x_all, labels=labels)
        y = self._labels(labels)
        x, hw = self._features(x_all, hw, y.shape[0])
        return x, hw, y

    # ------------------------------------------------------------------------------------------------ training
    def _head_chunk(self, g: HeadGroup, M: int) -> int:
        if self.head_chunk is not None:
            return max(1, min(g.H, int(self.head_chunk)))
        per_head = self._sgd_workspace_bytes(M, self.C, g.K)
        return max(1, min(g.H, SGD_WORKSPACE_BOUND // per_head))

    def _logits(self, g: HeadGroup, x: torch.Tensor, M: int) -> torch.Tensor:
        z = torch.empty(M, g.H * self.C, device=self.device, dtype=torch.float32)
        ops.probe_logits(x[:, g.col0:g.col0 + g.K], g.weight, g.bias, z, M, g.H * self.C, g.K)
        return z

    def _weight_step(self, g: HeadGroup, grad: torch.Tensor, xs: torch.Tensor, M: int) -> None:
        C, step = self.C, self._head_chunk(g, M)
        for lo in range(0, g.H, step):  # the chunking bounds the workspace and changes no bit of the result
            n = min(step, g.H - lo)
            ws = self._ws_sgd.at_least(self._sgd_workspace_bytes(M, n * C, g.K))
            self._sgd(g.weight[lo:lo + n], g.bias[lo:lo + n], g.m_weight[lo:lo + n], g.m_bias[lo:lo + n], grad[:, lo * C:], xs,
                      g.lr[lo:lo + n], M, n, C, g.K, self.momentum, ws)

    def _single_process(self) -> None:
        if self.world > 1:
            raise NotImplementedError("Training is single-process in this pull request.")

    def learning_rates(self, step: Optional[int] = None) -> Dict[str, float]:
        return self.heads.learning_rates(self.steps if step is None else step)

    def step(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self.step_features(self.features(images), self._hw(images), labels)

    def evaluate(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return self.evaluate_features(self.features(images), self._hw(images), labels)

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
