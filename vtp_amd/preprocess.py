"""The tools' PIL resize and crop on the device, bit for bit: decoded byte images of any sizes -> the normalised fp32 batch the
eval classes and the tokenizer take (csrc/preprocess.hip: one launch per pass over the whole ragged batch, no host
synchronisation).

    pp = Preprocess.probe_eval(resize=256, crop=224)         # Resize(short side, BICUBIC) + CenterCrop   (linear probing, eval)
    pp = Preprocess.probe_train(crop=224, seed=0, rank=0)    # RandomResizedCrop(BICUBIC) + flip 0.5      (linear probing, train)
    pp = Preprocess.zero_shot(image_size=256)                # Resize((S, S)), PIL's BILINEAR             (zero-shot tool)
    pp = Preprocess.center_crop(image_size=256, flip=False)  # center_crop_arr (ADM)                      (reconstruction, tokenizer)
    pp = Preprocess.resize((h, w), "bicubic")                # one plain Image.resize
    x = pp(images)                        # images: a sequence of uint8 [H_i, W_i, 3] arrays / CPU tensors, sizes may all differ
    x, u8 = pp(images, return_u8=True)    # f32 [B, 3, h, w] on the device (+ uint8 [B, h, w, 3] on the device)

PIL resamples 8-bit images in integer arithmetic and rounds to 8 bits after every pass, so the result can be, and is, matched
exactly: coefficients in float64 on the host exactly as Resample.c forms them, rounded to 22-bit fixed point (`coeffs`, cached
per (in, in0, in1, out, filter)); per pixel and channel acc = 2^21 + sum K[j] src[xmin + j] in int32 and clamp(acc >> 22, 0, 255)
on the device.  Image.resize runs the horizontal pass first, then the vertical one, and skips a pass whose size is unchanged.

`plan(sizes)` turns the image sizes into one Plan per image (host only: crops, resizes, the flip); `pack(images, plans)` checks
everything, lays the passes out as job rows and packs the source bytes; `apply(images, plans)` uploads and launches.  A crop is a
change of view (offset, size, pitch) and costs nothing; the last vertical pass resamples only the final crop window, applies the
flip and writes ToTensor + Normalize in the expression of vtp_u8_to_images.  JPEG decoding stays on the host.

The two torchvision size rules (Resize(int) and CenterCrop) are restated from torchvision's source.  torchvision pads a centre
crop that is larger than the resized image; here that is a ValueError.  There is no CPU path: without the HIP library or a GPU
`apply` raises RuntimeError."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .augment import _box
from .tokenizer import NORMALIZE_IMAGENET

BOX, BILINEAR, BICUBIC = 0, 1, 2
FILTER_NAMES = {"box": BOX, "bilinear": BILINEAR, "bicubic": BICUBIC}
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, BICUBIC: 2.0}
IDENTITY = 3                                          # the one-tap table K = 2^22: (2^21 + p 2^22) >> 22 == p
BITS = 22                                             # PIL's PRECISION_BITS for 8 bits per channel
JOB = 16                                              # int64 slots per job row (include/vtp_hip.h)
J_SRC, J_DST, J_OH, J_OW, J_SY, J_SX, J_TS, J_BND, J_COEF, J_KSIZE, J_SUB, J_FLAGS, J_BLOCK = range(13)
F_SCRATCH, F_AXIS_Y, F_FLIP = 1, 2, 4                 # bits of the flags slot
THREADS = 256                                         # output pixels per block


# ---- coefficient tables (host, float64 as Resample.c) ---------------------------------------------------------------------------
def _filter(filt: int, x: np.ndarray) -> np.ndarray:
    if filt == BOX:
        return ((x > -0.5) & (x <= 0.5)).astype(np.float64)
    x = np.abs(x)
    if filt == BILINEAR:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


_TABLES = {}


def coeffs(size_in: int, in0: float, in1: float, out: int, filt: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """precompute_coeffs + normalize_coeffs_8bpc of one pass -> xmin int32 [out], n int32 [out], K int32 [out, ksize] (zero
    beyond n).  filt = IDENTITY: the one-tap table of an axis that is not resampled."""
    key = (int(size_in), float(in0), float(in1), int(out), int(filt))
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    if size_in < 1 or out < 1 or not (0 <= in0 < in1 <= size_in):
        raise ValueError(f"a pass needs size_in, out >= 1 and 0 <= in0 < in1 <= size_in, got {key}")
    if filt == IDENTITY:
        if out != size_in:
            raise ValueError("the identity table does not change the size")
        tab = (np.arange(out, dtype=np.int32), np.ones(out, np.int32), np.full((out, 1), 1 << BITS, np.int32))
        _TABLES[key] = tab
        return tab
    scale = (in1 - in0) / out
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmin, n, K = np.zeros(out, np.int32), np.zeros(out, np.int32), np.zeros((out, ksize), np.int32)
    for xx in range(out):
        c = in0 + (xx + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        cnt = min(int(c + support + 0.5), size_in) - lo
        k = _filter(filt, (np.arange(lo, lo + cnt, dtype=np.int64).astype(np.float64) - c + 0.5) * ss)
        ww = 0.0
        for v in k.tolist():  # summed left to right, as the C loop does (np.sum adds pairwise)
            ww += v
        if ww != 0.0:
            k = k / ww
        K[xx, :cnt] = np.where(k < 0, k * (1 << BITS) - 0.5, k * (1 << BITS) + 0.5).astype(np.int32)  # C's (int): truncation
        xmin[xx], n[xx] = lo, cnt
    tab = (xmin, n, K)
    _TABLES[key] = tab
    return tab


# ---- plans (host, pure Python) --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Plan:
    """What happens to one H x W image: ops in order, each ("resize", filter, h, w) or ("crop", y0, x0, h, w), then the flip."""
    H: int
    W: int
    ops: Tuple[tuple, ...]
    flip: bool = False

    def sizes(self) -> List[Tuple[int, int]]:
        """(h, w) after each op; ValueError for an op that does not fit"""
        h, w, out = self.H, self.W, []
        for op in self.ops:
            if op[0] == "resize":
                _, filt, oh, ow = op
                if filt not in (BOX, BILINEAR, BICUBIC) or oh < 1 or ow < 1:
                    raise ValueError(f"bad resize {op}")
                h, w = int(oh), int(ow)
            elif op[0] == "crop":
                _, y0, x0, ch, cw = op
                if ch < 1 or cw < 1 or y0 < 0 or x0 < 0 or y0 + ch > h or x0 + cw > w:
                    raise ValueError(f"the crop {op[1:]} (y0, x0, h, w) does not lie inside the {h} x {w} image")
                h, w = int(ch), int(cw)
            else:
                raise ValueError(f"unknown op {op}")
            out.append((h, w))
        return out

    def out_size(self) -> Tuple[int, int]:
        s = self.sizes()
        return s[-1] if s else (self.H, self.W)

    def halvings(self) -> int:
        return sum(1 for op in self.ops if op[0] == "resize" and op[1] == BOX)


def _hw(H, W):
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"an image needs H, W >= 1, got {H} x {W}")
    return H, W


def plan_center_crop(H: int, W: int, S: int, flip: bool = False) -> Plan:
    """center_crop_arr (ADM): halve with BOX while the short side >= 2 S, BICUBIC so that the short side is S, centre crop"""
    H, W = _hw(H, W)
    h, w, ops = H, W, []
    while min(w, h) >= 2 * S:
        h, w = h // 2, w // 2
        ops.append(("resize", BOX, h, w))
    s = S / min(w, h)
    h, w = round(h * s), round(w * s)  # Python's round: half to even, as the tool
    if h < S or w < S:
        raise ValueError(f"center_crop: the {H} x {W} image resizes to {h} x {w}, smaller than the crop {S}")
    ops.append(("resize", BICUBIC, h, w))
    ops.append(("crop", (h - S) // 2, (w - S) // 2, S, S))
    return Plan(H, W, tuple(ops), bool(flip))


def plan_probe_eval(H: int, W: int, resize: int, crop: int) -> Plan:
    """torchvision Resize(resize, BICUBIC) of a PIL image (short side -> resize, long side -> int(resize * long / short)) and
    CenterCrop(crop) (top = int(round((h - crop) / 2.0)), left likewise).  A crop larger than the resized image: ValueError."""
    H, W = _hw(H, W)
    if W <= H:
        w, h = resize, int(resize * H / W)
    else:
        h, w = resize, int(resize * W / H)
    if crop > h or crop > w:
        raise ValueError(f"probe_eval: the crop {crop} is larger than the resized image {h} x {w} (torchvision pads; not supported)")
    top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
    return Plan(H, W, (("resize", BICUBIC, h, w), ("crop", top, left, crop, crop)))


def plan_zero_shot(H: int, W: int, S: int) -> Plan:
    H, W = _hw(H, W)
    return Plan(H, W, (("resize", BILINEAR, S, S),))


def plan_resized_crop(H: int, W: int, box, S: int, flip: bool = False) -> Plan:
    """F.resized_crop of a PIL image: crop the box (y0, x0, h, w), BICUBIC to S x S (the box is the whole image: no tap lies
    outside it), flip"""
    H, W = _hw(H, W)
    y0, x0, h, w = (int(v) for v in box)
    return Plan(H, W, (("crop", y0, x0, h, w), ("resize", BICUBIC, S, S)), bool(flip))


def plan_resize(H: int, W: int, size, filt: int) -> Plan:
    H, W = _hw(H, W)
    return Plan(H, W, (("resize", filt, int(size[0]), int(size[1])),))


# ---- packing: plans -> job rows, tables, source bytes (host) ----------------------------------------------------------------------
@dataclass
class Packed:
    """One batch ready for the kernels, all on the host: src uint8 [src_len] (pinned when a GPU is there), jobs int64 [n, 16],
    tab int32 (bounds pairs and coefficients), launches int32 [L, 3] = (first job, jobs, blocks) with the fused ending last"""
    src: torch.Tensor
    jobs: np.ndarray
    tab: np.ndarray
    launches: np.ndarray
    scratch_len: int
    B: int
    out_h: int
    out_w: int


class _Tables:
    """the tables one batch uses, concatenated: (min, n) pairs and K rows as one int32 array"""

    def __init__(self):
        self.parts, self.len, self.at = [], 0, {}

    def add(self, size_in, out, filt):
        key = (size_in, out, filt)
        if key not in self.at:
            xmin, n, K = coeffs(size_in, 0, size_in, out, filt)
            bnd = np.stack((xmin, n), 1).reshape(-1)
            self.at[key] = (self.len, self.len + bnd.size, K.shape[1], xmin, n)
            self.parts += [bnd, K.reshape(-1)]
            self.len += bnd.size + K.size
        return self.at[key]

    def array(self):
        return np.ascontiguousarray(np.concatenate(self.parts).astype(np.int32)) if self.parts else np.zeros(0, np.int32)


def _blocks(oh, ow):
    return (oh * ow + THREADS - 1) // THREADS


def build_jobs(plans: Sequence[Plan], offsets: Sequence[int]):
    """the passes of every plan as job rows -> (jobs int64 [n, 16], tab int32, launches int32 [L, 3], scratch_len).  Image i's
    bytes start at offsets[i] of the source buffer.  Launch l holds at most one job per image, and an image's passes sit in the
    last launches, so that every image's fused ending is in the final one."""
    tabs = _Tables()
    per_image, scratch = [], 0
    for plan, off in zip(plans, offsets):
        plan.sizes()
        in_scratch, h, w, pitch = 0, plan.H, plan.W, plan.W * 3
        rows = []
        resizes = [k for k, op in enumerate(plan.ops) if op[0] == "resize"]
        last = resizes[-1] if resizes else len(plan.ops)
        ops = list(plan.ops) if resizes else list(plan.ops) + [("resize", BICUBIC, *plan.out_size())]
        for k, op in enumerate(ops[:last]):
            if op[0] == "crop":
                _, y0, x0, h, w = op
                off += y0 * pitch + x0 * 3
                continue
            _, filt, oh, ow = op
            if ow != w:  # horizontal: one table entry per output column, taps 3 bytes apart
                b, c, ks, _, _ = tabs.add(w, ow, filt)
                rows.append([off, scratch, h, ow, pitch, 0, 3, b, c, ks, 0, in_scratch, 0])
                off, in_scratch, w, pitch = scratch, F_SCRATCH, ow, ow * 3
                scratch += h * ow * 3
            if oh != h:  # vertical: one table entry per output row, taps one pitch apart
                b, c, ks, _, _ = tabs.add(h, oh, filt)
                rows.append([off, scratch, oh, w, 0, 3, pitch, b, c, ks, 0, in_scratch | F_AXIS_Y, 0])
                off, in_scratch, h = scratch, F_SCRATCH, oh
                scratch += oh * w * 3
        # the last resize with the crops behind it: only the window [top, top + fh) x [left, left + fw) of its output is formed
        _, filt, oh, ow = ops[last]
        top, left, fh, fw = 0, 0, oh, ow
        for op in ops[last + 1:]:
            top, left, fh, fw = top + op[1], left + op[2], op[3], op[4]
        vb, vc, vks, vmin, vn = tabs.add(h, oh, filt if oh != h else IDENTITY)
        r0, r1 = int(vmin[top]), int((vmin[top:top + fh] + vn[top:top + fh]).max())  # the source rows the window reads
        if ow != w:
            b, c, ks, _, _ = tabs.add(w, ow, filt)
            rows.append([off + r0 * pitch, scratch, r1 - r0, fw, pitch, 0, 3, b + 2 * left, c + ks * left, ks, 0, in_scratch, 0])
            off, in_scratch, pitch, sub = scratch, F_SCRATCH, fw * 3, r0
            scratch += (r1 - r0) * fw * 3
        else:
            off, sub = off + left * 3, 0
        final = [off, len(per_image), fh, fw, 0, 3, pitch, vb + 2 * top, vc + vks * top, vks, sub,
                 in_scratch | F_AXIS_Y | (F_FLIP if plan.flip else 0), 0]
        per_image.append((rows, final))
    depth = max(len(r) for r, _ in per_image)
    jobs, launches = [], []
    for l in range(depth + 1):
        first, blocks = len(jobs), 0
        for rows, final in per_image:
            k = l - (depth - len(rows))
            if l == depth:
                row = final
            elif k >= 0:
                row = rows[k]
            else:
                continue
            row = row + [0] * (JOB - len(row))
            row[J_BLOCK] = blocks
            blocks += _blocks(row[J_OH], row[J_OW])
            jobs.append(row)
        launches.append((first, len(jobs) - first, blocks))
    return np.asarray(jobs, dtype=np.int64).reshape(-1, JOB), tabs.array(), np.asarray(launches, dtype=np.int32).reshape(-1, 3), scratch


def check_jobs(jobs: np.ndarray, tab: np.ndarray, launches: np.ndarray, src_len: int, scratch_len: int, B: int, out_h: int,
               out_w: int) -> None:
    """ValueError for a table the kernels would have to bend: every byte a job reads or writes and every table entry it looks up
    must lie inside its buffer, the block numbering must be the one the kernels search, the last launch one ending per image"""
    if (not isinstance(jobs, np.ndarray) or jobs.dtype != np.int64 or jobs.ndim != 2 or jobs.shape[1] != JOB or len(jobs) < 1
            or not isinstance(tab, np.ndarray) or tab.dtype != np.int32 or tab.ndim != 1
            or not isinstance(launches, np.ndarray) or launches.dtype != np.int32 or launches.ndim != 2 or launches.shape[1] != 3
            or len(launches) < 1):
        raise ValueError("jobs must be int64 [n, 16], tab int32 [m], launches int32 [L, 3]")
    at = 0
    for l, (first, count, blocks) in enumerate(launches.tolist()):
        fin = l == len(launches) - 1
        if first != at or count < 1 or (fin and count != B):
            raise ValueError(f"launch {l}: jobs [{first}, {first + count}) do not follow the launch before (or: not one ending per image)")
        at += count
        if at > len(jobs):
            raise ValueError(f"launch {l} names jobs beyond the table")
        nb = 0
        for i in range(first, first + count):
            src, dst, oh, ow, sy, sx, ts, bnd, coef, ks, sub, flags, blk = jobs[i, :13].tolist()
            if oh < 1 or ow < 1 or oh * ow >= 2 ** 31 or blk != nb or ks < 1 or min(sy, sx, ts) < 0 or flags & ~7:
                raise ValueError(f"job {i}: bad size, block number, strides or flags")
            nb += _blocks(oh, ow)
            cnt = oh if flags & F_AXIS_Y else ow
            if bnd < 0 or coef < 0 or bnd + 2 * cnt > len(tab) or coef + cnt * ks > len(tab):
                raise ValueError(f"job {i}: its table lies outside the table buffer")
            lo, n = tab[bnd:bnd + 2 * cnt:2].astype(np.int64) - sub, tab[bnd + 1:bnd + 2 * cnt:2].astype(np.int64)
            if (n < 1).any() or (n > ks).any() or (lo < 0).any():
                raise ValueError(f"job {i}: a tap count outside [1, {ks}] or a tap in front of its source")
            end = src + (oh - 1) * sy + (ow - 1) * sx + int((lo + n - 1).max()) * ts + 3
            size = scratch_len if flags & F_SCRATCH else src_len
            if src < 0 or end > size:
                raise ValueError(f"job {i}: reads bytes [{src}, {end}) of a buffer of {size}")
            if fin:
                if dst != i - first or (oh, ow) != (out_h, out_w):
                    raise ValueError(f"job {i}: the ending of image {i - first} must write image {i - first} at {out_h} x {out_w}, "
                                     f"got image {dst} at {oh} x {ow}")
            else:
                if flags & F_FLIP or dst < 0 or dst + oh * ow * 3 > scratch_len:
                    raise ValueError(f"job {i}: writes bytes [{dst}, {dst + oh * ow * 3}) of a scratch of {scratch_len}")
                if flags & F_SCRATCH and src < dst + oh * ow * 3 and dst < end:
                    raise ValueError(f"job {i}: reads what it writes")
        if nb != blocks or blocks >= 2 ** 31:
            raise ValueError(f"launch {l}: {blocks} blocks, its jobs need {nb}")
    if at != len(jobs):
        raise ValueError("jobs behind the last launch")


def _as_u8(img, i) -> np.ndarray:
    if isinstance(img, torch.Tensor):
        if img.is_cuda:
            raise ValueError(f"image {i}: the decoded images are CPU tensors or numpy arrays")
        img = img.numpy() if img.dtype == torch.uint8 else img
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8:
        raise ValueError(f"image {i}: must be uint8, got {getattr(img, 'dtype', type(img))}")
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"image {i}: must be [H, W, 3] with H, W >= 1, got {tuple(img.shape)}")
    return img


class Preprocess:
    """kind: "center_crop" | "probe_eval" | "probe_train" | "zero_shot" | "resize" (use the classmethods).  The output is
    f32 [B, 3, out_h, out_w].  mean / std: the normalisation (default: ImageNet, the tokenizer's)."""

    def __init__(self, kind: str, out_size: Tuple[int, int], *, resize_to: Optional[int] = None, filt: int = BICUBIC, flip: bool = False,
                 scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), seed: int = 0, rank: int = 0, mean=None, std=None,
                 device=None):
        if kind not in ("center_crop", "probe_eval", "probe_train", "zero_shot", "resize"):
            raise ValueError(f"unknown kind {kind!r}")
        self.kind = kind
        self.out_h, self.out_w = int(out_size[0]), int(out_size[1])
        if self.out_h < 1 or self.out_w < 1:
            raise ValueError(f"the output size must be at least 1 x 1, got {out_size}")
        self.resize_to, self.filt, self.flip = resize_to, int(filt), bool(flip)
        self.scale, self.ratio = tuple(scale), tuple(ratio)
        self.seed, self.rank = int(seed), int(rank)
        self.rng = np.random.default_rng([self.seed, self.rank])
        self.mean = tuple(NORMALIZE_IMAGENET["mean"] if mean is None else mean)
        self.std = tuple(NORMALIZE_IMAGENET["std"] if std is None else std)
        if len(self.mean) != 3 or len(self.std) != 3 or any(float(s) == 0.0 for s in self.std):
            raise ValueError("mean and std need three values, std none of them zero")
        self.device = device
        self._scratch = {}

    @classmethod
    def probe_eval(cls, resize: int = 256, crop: int = 224, **kw):
        """Resize(resize, BICUBIC) + CenterCrop(crop): the evaluation transform of the linear-probing tool"""
        if resize < 1 or crop < 1:
            raise ValueError("resize, crop >= 1")
        return cls("probe_eval", (crop, crop), resize_to=int(resize), **kw)

    @classmethod
    def probe_train(cls, crop: int = 224, seed: int = 0, rank: int = 0, **kw):
        """RandomResizedCrop(crop, BICUBIC) + RandomHorizontalFlip: the training transform of the linear-probing tool"""
        return cls("probe_train", (crop, crop), seed=seed, rank=rank, **kw)

    @classmethod
    def zero_shot(cls, image_size: int = 256, **kw):
        """Resize((S, S)) with torchvision's default interpolation, PIL's BILINEAR: the transform of the zero-shot tool"""
        return cls("zero_shot", (image_size, image_size), filt=BILINEAR, **kw)

    @classmethod
    def center_crop(cls, image_size: int = 256, flip: bool = False, **kw):
        """center_crop_arr (ADM) (+ the p = 1 flip of the latents_flip pass): reconstruction tool, tokenizer"""
        return cls("center_crop", (image_size, image_size), flip=flip, **kw)

    @classmethod
    def resize(cls, size: Tuple[int, int], filter="bicubic", **kw):
        """one Image.resize((w, h), filter) to size = (h, w)"""
        filt = FILTER_NAMES[filter] if isinstance(filter, str) else int(filter)
        if filt not in (BOX, BILINEAR, BICUBIC):
            raise ValueError(f"unknown filter {filter!r}")
        return cls("resize", tuple(size), filt=filt, **kw)

    # ---- host ---------------------------------------------------------------------------------------------------------------------
    def plan(self, sizes: Sequence[Tuple[int, int]]) -> List[Plan]:
        """one Plan per image from its (H, W).  probe_train draws here: the box by RandomResizedCrop.get_params, then one
        rng.random() < 0.5 for the flip, image by image."""
        plans = []
        for H, W in sizes:
            H, W = _hw(H, W)
            if self.kind == "center_crop":
                plans.append(plan_center_crop(H, W, self.out_h, self.flip))
            elif self.kind == "probe_eval":
                plans.append(plan_probe_eval(H, W, self.resize_to, self.out_h))
            elif self.kind == "zero_shot":
                plans.append(plan_zero_shot(H, W, self.out_h))
            elif self.kind == "resize":
                plans.append(plan_resize(H, W, (self.out_h, self.out_w), self.filt))
            else:
                box = _box(self.rng, H, W, self.scale, self.ratio)
                plans.append(plan_resized_crop(H, W, box, self.out_h, self.rng.random() < 0.5))
        return plans

    def state_dict(self) -> dict:
        return {"seed": self.seed, "rank": self.rank, "bit_generator": self.rng.bit_generator.state}

    def load_state_dict(self, sd: dict) -> None:
        self.seed, self.rank = int(sd["seed"]), int(sd["rank"])
        self.rng = np.random.default_rng([self.seed, self.rank])
        self.rng.bit_generator.state = sd["bit_generator"]

    def pack(self, images: Sequence, plans: Sequence[Plan], pin: bool = False) -> Packed:
        """check the images and plans (ValueError) and lay the batch out for the kernels; nothing here touches the GPU"""
        images = list(images)
        plans = list(plans)
        if not images:
            raise ValueError("the batch is empty")
        if len(plans) != len(images):
            raise ValueError(f"{len(images)} images need {len(images)} plans, got {len(plans)}")
        arrs = [_as_u8(img, i) for i, img in enumerate(images)]
        offsets, total = [], 0
        for i, (a, p) in enumerate(zip(arrs, plans)):
            if not isinstance(p, Plan) or (p.H, p.W) != a.shape[:2]:
                raise ValueError(f"image {i} is {a.shape[0]} x {a.shape[1]}, its plan is for {getattr(p, 'H', '?')} x {getattr(p, 'W', '?')}")
            if p.out_size() != (self.out_h, self.out_w):
                raise ValueError(f"image {i}: its plan ends at {p.out_size()}, the output is {self.out_h} x {self.out_w}")
            offsets.append(total)
            total += a.size
        jobs, tab, launches, scratch_len = build_jobs(plans, offsets)
        check_jobs(jobs, tab, launches, total, scratch_len, len(arrs), self.out_h, self.out_w)
        src = torch.empty(total, dtype=torch.uint8, pin_memory=pin)
        buf = src.numpy()
        for a, o in zip(arrs, offsets):
            buf[o:o + a.size] = a.reshape(-1)
        return Packed(src, jobs, tab, launches, scratch_len, len(arrs), self.out_h, self.out_w)

    # ---- the kernels --------------------------------------------------------------------------------------------------------------
    def apply(self, images: Sequence, plans: Sequence[Plan], return_u8: bool = False):
        """-> f32 [B, 3, out_h, out_w] on the device (and uint8 [B, out_h, out_w, 3] with return_u8).  Everything is checked on the
        host before anything is uploaded or launched; two uploads (the bytes, the tables), one launch per pass, no host
        synchronisation."""
        gpu = torch.cuda.is_available()
        pk = self.pack(images, plans, pin=gpu)
        if not gpu:
            raise RuntimeError("vtp_amd.Preprocess runs on the MI355X kernels only (no CPU path)")
        dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError("vtp_amd.Preprocess runs on the MI355X kernels only: the device must be cuda (no CPU path)")
        from . import ops
        with torch.cuda.device(dev):
            key = str(dev)
            scratch = self._scratch.get(key)
            if scratch is None or scratch.numel() < pk.scratch_len:
                scratch = self._scratch[key] = torch.empty(max(pk.scratch_len, 1), device=dev, dtype=torch.uint8)
            meta = torch.empty(pk.jobs.size + (pk.tab.size + 1) // 2, dtype=torch.int64, pin_memory=True)
            meta[:pk.jobs.size] = torch.from_numpy(pk.jobs.reshape(-1))
            meta[pk.jobs.size:].view(torch.int32)[:pk.tab.size] = torch.from_numpy(pk.tab)
            src = pk.src.to(dev, non_blocking=True)
            meta = meta.to(dev, non_blocking=True)
            out = torch.empty(pk.B, 3, pk.out_h, pk.out_w, device=dev, dtype=torch.float32)
            u8 = torch.empty(pk.B, pk.out_h, pk.out_w, 3, device=dev, dtype=torch.uint8) if return_u8 else None
            ops.preprocess(src, scratch, meta[:pk.jobs.size], meta[pk.jobs.size:].view(torch.int32), pk.launches, out, u8, self.mean,
                           self.std)
        return (out, u8) if return_u8 else out

    def __call__(self, images: Sequence, return_u8: bool = False):
        images = list(images)
        sizes = [tuple(_as_u8(img, i).shape[:2]) for i, img in enumerate(images)]
        return self.apply(images, self.plan(sizes), return_u8=return_u8)
