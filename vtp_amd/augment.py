"""SSL crops on the device: the DINO multi-crop augmentation (DINOv2's DataAugmentationDINO, with the arithmetic of torchvision's
float-tensor path) from a batch of decoded byte images to the normalised fp32 crops `collate_ssl_batch` / `trainer.prepare_ssl`
take -- two launches per output size (csrc/augment.hip), no host synchronisation.

    aug = MultiCrop.dino_default(global_size=256, local_size=96, n_local=8, seed=0, rank=rank)
    for u8 in loader:                        # uint8 [B, Hs, Ws, 3], RGB, decoded and resized to one staging size by the loader
        g, l = aug(u8)                       # f32 [2 B, 3, 256, 256], f32 [8 B, 3, 96, 96], view-major (crop v * B + b from image b)
        ssl = trainer.prepare_ssl(g, l, masks)

Per crop, in fp32 on x = u8 / 255: resized crop (crop the box, then antialiased bicubic to S x S, clamp) -> flip -> colour jitter
(brightness, contrast, saturation, hue in a random order) -> grayscale -> 9 x 9 Gaussian blur -> solarize -> normalise.  Nothing
is rounded to 8 bits between the stages (the PIL pipeline does that at every stage): bit parity with PIL is not a goal.  The
random parameters are drawn on the host (`draw`: a numpy Generator seeded with [seed, rank], the rules of torchvision's
RandomResizedCrop.get_params and ColorJitter.get_params) into one table row per crop; `apply` uploads the tables and runs the
kernels.  There is no CPU path: without the HIP library or a GPU `apply` raises."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

from .tokenizer import NORMALIZE_IMAGENET

ROW = 16                                              # floats per table row (include/vtp_hip.h)
FLIP, JITTER, GRAY, SOLARIZE = 1, 2, 4, 8             # bits of the flags slot
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3    # operation ids of the order slots; -1: none
MAX_RATIO = 8                                         # largest box / size per axis the kernels resample
_PerView = Union[float, Tuple[float, ...]]


def encode_row(box, flip=False, order=None, factors=(1.0, 1.0, 1.0, 0.0), gray=False, sigma=0.0, solarize=False) -> np.ndarray:
    """one table row.  box = (y0, x0, h, w); order = the jitter's operations in the order they run (any arrangement of distinct
    ids out of 0..3, up to four; None = no jitter); factors = (brightness, contrast, saturation, hue); sigma <= 0 = no blur"""
    r = np.zeros(ROW, dtype=np.float32)
    r[0:4] = box
    r[5:9] = -1
    flags = FLIP * bool(flip) + GRAY * bool(gray) + SOLARIZE * bool(solarize)
    if order is not None:
        order = [int(o) for o in order]
        if len(order) > 4 or len(set(order)) != len(order) or any(o not in (0, 1, 2, 3) for o in order):
            raise ValueError(f"order must hold distinct operation ids out of 0..3, got {order}")
        flags += JITTER
        r[5:5 + len(order)] = order
    r[4] = flags
    r[9:13] = factors
    r[13] = sigma
    return r


def decode_row(row) -> dict:
    """the inverse of encode_row"""
    row = np.asarray(row, dtype=np.float32)
    flags = int(row[4])
    order = [int(o) for o in row[5:9] if o >= 0] if flags & JITTER else None
    return {"box": tuple(int(v) for v in row[0:4]), "flip": bool(flags & FLIP), "order": order,
            "factors": tuple(float(v) for v in row[9:13]), "gray": bool(flags & GRAY), "sigma": float(row[13]),
            "solarize": bool(flags & SOLARIZE)}


@dataclass
class ViewPolicy:
    """`views` crops of `size` x `size` per image.  p_blur / p_solarize: one probability, or one per view."""
    size: int
    views: int
    scale: Tuple[float, float]
    ratio: Tuple[float, float] = (3 / 4, 4 / 3)
    p_flip: float = 0.5
    p_jitter: float = 0.0
    brightness: float = 0.0
    contrast: float = 0.0
    saturation: float = 0.0
    hue: float = 0.0
    p_gray: float = 0.0
    p_blur: _PerView = 0.0
    sigma: Tuple[float, float] = (0.1, 2.0)
    p_solarize: _PerView = 0.0

    def per_view(self, p: _PerView, v: int) -> float:
        if isinstance(p, (tuple, list)):
            if len(p) != self.views:
                raise ValueError(f"a per-view probability needs {self.views} entries, got {len(p)}")
            return float(p[v])
        return float(p)


def _box(rng: np.random.Generator, Hs: int, Ws: int, scale, ratio) -> Tuple[int, int, int, int]:
    """RandomResizedCrop.get_params: ten tries of area x log-uniform aspect, then the centre crop with the ratio clamped"""
    area = Hs * Ws
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * rng.uniform(scale[0], scale[1])
        aspect = math.exp(rng.uniform(lo, hi))
        w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < w <= Ws and 0 < h <= Hs:
            return int(rng.integers(0, Hs - h + 1)), int(rng.integers(0, Ws - w + 1)), h, w
    in_ratio = Ws / Hs
    if in_ratio < min(ratio):
        w = Ws
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = Hs
        w = int(round(h * max(ratio)))
    else:
        w, h = Ws, Hs
    return (Hs - h) // 2, (Ws - w) // 2, h, w


def check_table(table: np.ndarray, n_rows: int, size: int, Hs: int, Ws: int) -> None:
    """ValueError for a table the kernels would have to bend: wrong shape, a box outside the image, box / size above 8"""
    if size < 5:
        raise ValueError(f"the crop size must be at least 5 (the blur reflects by 4), got {size}")
    if not isinstance(table, np.ndarray) or table.dtype != np.float32 or table.shape != (n_rows, ROW):
        raise ValueError(f"a table must be a float32 array [{n_rows}, {ROW}], got {getattr(table, 'dtype', None)} "
                         f"{getattr(table, 'shape', None)}")
    y0, x0, h, w = (table[:, i].astype(np.int64) for i in range(4))
    if not (np.array_equal(table[:, :4], np.stack((y0, x0, h, w), 1).astype(np.float32)) and (h >= 1).all() and (w >= 1).all()
            and (y0 >= 0).all() and (x0 >= 0).all() and (y0 + h <= Hs).all() and (x0 + w <= Ws).all()):
        raise ValueError(f"a box lies outside the {Hs} x {Ws} image (or is empty, or not integral)")
    if (h > MAX_RATIO * size).any() or (w > MAX_RATIO * size).any():
        raise ValueError(f"a box is more than {MAX_RATIO} times the crop size {size} per axis: resize the staging images first")
    if not np.isfinite(table).all():
        raise ValueError("a table holds a value that is not finite")


class MultiCrop:
    """policies: one ViewPolicy per output tensor.  seed, rank: the stream of random parameters is numpy's default generator
    seeded with [seed, rank].  mean / std: the normalisation (default: ImageNet, the tokenizer's)."""

    def __init__(self, policies: Sequence[ViewPolicy], seed: int = 0, rank: int = 0, mean=None, std=None, device=None):
        self.policies = list(policies)
        if not self.policies:
            raise ValueError("MultiCrop needs at least one ViewPolicy")
        for p in self.policies:
            if p.size < 5:
                raise ValueError(f"the crop size must be at least 5 (the blur reflects by 4), got {p.size}")
            if p.views < 1:
                raise ValueError("a ViewPolicy needs at least one view")
            for v in range(p.views):
                p.per_view(p.p_blur, v), p.per_view(p.p_solarize, v)
        self.seed, self.rank = int(seed), int(rank)
        self.rng = np.random.default_rng([self.seed, self.rank])
        self.mean = tuple(NORMALIZE_IMAGENET["mean"] if mean is None else mean)
        self.std = tuple(NORMALIZE_IMAGENET["std"] if std is None else std)
        self.device = device
        self._ws = {}

    @classmethod
    def dino_default(cls, global_size: int = 256, local_size: int = 96, n_local: int = 8, seed: int = 0, rank: int = 0, **kw):
        """DINOv2's settings: two global crops (scale 0.32..1; blur always / 0.1; solarize 0.2 on the second) and n_local local
        crops (scale 0.05..0.32; blur 0.5); flip 0.5, jitter 0.8 with (0.4, 0.4, 0.2, 0.1), grayscale 0.2 on all of them"""
        common = dict(p_flip=0.5, p_jitter=0.8, brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1, p_gray=0.2)
        pol = [ViewPolicy(size=global_size, views=2, scale=(0.32, 1.0), p_blur=(1.0, 0.1), p_solarize=(0.0, 0.2), **common)]
        if n_local > 0:
            pol.append(ViewPolicy(size=local_size, views=n_local, scale=(0.05, 0.32), p_blur=0.5, **common))
        return cls(pol, seed=seed, rank=rank, **kw)

    @classmethod
    def plain(cls, size: int, scale: Tuple[float, float] = (0.08, 1.0), seed: int = 0, rank: int = 0, **kw):
        """crop + flip + normalise only: the view of the reconstruction / CLIP images"""
        return cls([ViewPolicy(size=size, views=1, scale=scale)], seed=seed, rank=rank, **kw)

    # ---- the random parameters (host) -----------------------------------------------------------------------------------
    def _draw_row(self, p: ViewPolicy, v: int, Hs: int, Ws: int) -> np.ndarray:
        rng = self.rng
        box = _box(rng, Hs, Ws, p.scale, p.ratio)
        flip = rng.random() < p.p_flip
        order, factors = None, (1.0, 1.0, 1.0, 0.0)
        if rng.random() < p.p_jitter:  # ColorJitter.get_params: a random order, uniform factors
            order = rng.permutation(4)
            factors = (rng.uniform(max(0.0, 1 - p.brightness), 1 + p.brightness), rng.uniform(max(0.0, 1 - p.contrast), 1 + p.contrast),
                       rng.uniform(max(0.0, 1 - p.saturation), 1 + p.saturation), rng.uniform(-p.hue, p.hue))
        gray = rng.random() < p.p_gray
        sigma = rng.uniform(p.sigma[0], p.sigma[1]) if rng.random() < p.per_view(p.p_blur, v) else 0.0
        solarize = rng.random() < p.per_view(p.p_solarize, v)
        return encode_row(box, flip, order, factors, gray, sigma, solarize)

    def draw(self, B: int, Hs: int, Ws: int) -> List[np.ndarray]:
        """the parameter tables of one batch, one float32 [views * B, 16] per policy, rows view-major"""
        if B < 1 or Hs < 1 or Ws < 1:
            raise ValueError(f"draw needs B, Hs, Ws >= 1, got {B}, {Hs}, {Ws}")
        return [np.stack([self._draw_row(p, v, Hs, Ws) for v in range(p.views) for _ in range(B)]) for p in self.policies]

    def state_dict(self) -> dict:
        return {"seed": self.seed, "rank": self.rank, "bit_generator": self.rng.bit_generator.state}

    def load_state_dict(self, sd: dict) -> None:
        self.seed, self.rank = int(sd["seed"]), int(sd["rank"])
        self.rng = np.random.default_rng([self.seed, self.rank])
        self.rng.bit_generator.state = sd["bit_generator"]

    # ---- the kernels ------------------------------------------------------------------------------------------------------
    def apply(self, u8: torch.Tensor, tables: Sequence[np.ndarray]) -> List[torch.Tensor]:
        """u8: uint8 [B, Hs, Ws, 3] on the host (uploaded through a pinned buffer) or on the device; tables: what draw returned
        (or rows built with encode_row).  Returns one f32 [views * B, 3, size, size] per policy.  Everything is checked on the
        host before anything is uploaded or launched."""
        if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8:
            raise ValueError(f"the images must be a uint8 tensor, got {getattr(u8, 'dtype', type(u8))}")
        if u8.dim() != 4 or u8.shape[3] != 3 or u8.shape[0] < 1 or u8.shape[1] < 1 or u8.shape[2] < 1:
            raise ValueError(f"the images must be [B, Hs, Ws, 3], got {tuple(u8.shape)}")
        B, Hs, Ws, _ = u8.shape
        if Ws % 4:
            raise ValueError(f"the staging width must be a multiple of 4 (Ws % 4 == 0), got {Ws}")
        if len(tables) != len(self.policies):
            raise ValueError(f"{len(self.policies)} policies need {len(self.policies)} tables, got {len(tables)}")
        for p, t in zip(self.policies, tables):
            check_table(t, p.views * B, p.size, Hs, Ws)
        if not torch.cuda.is_available():
            raise RuntimeError("vtp_amd.MultiCrop runs on the MI355X kernels only (no CPU path)")
        from . import ops
        if u8.is_cuda:
            dev = u8.device
        else:
            dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError("vtp_amd.MultiCrop runs on the MI355X kernels only: the device must be cuda (no CPU path)")
        src = u8.contiguous() if u8.is_cuda else u8.contiguous().pin_memory().to(dev, non_blocking=True)
        outs = []
        for p, t in zip(self.policies, tables):
            N, S = p.views * B, p.size
            key = (str(dev), N, S)
            scratch = self._ws.get(key)
            if scratch is None:
                scratch = self._ws[key] = torch.empty(ops.augment_scratch_size(N, S), device=dev, dtype=torch.float32)
            table = torch.from_numpy(np.ascontiguousarray(t)).pin_memory().to(dev, non_blocking=True)
            out = torch.empty(N, 3, S, S, device=dev, dtype=torch.float32)
            ops.augment_crops(src, table, out, self.mean, self.std, scratch)
            outs.append(out)
        return outs

    def __call__(self, u8: torch.Tensor) -> List[torch.Tensor]:
        if not isinstance(u8, torch.Tensor) or u8.dim() != 4:
            raise ValueError("the images must be a uint8 tensor [B, Hs, Ws, 3]")
        return self.apply(u8, self.draw(int(u8.shape[0]), int(u8.shape[1]), int(u8.shape[2])))
