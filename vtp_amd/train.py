"""Data-parallel training step for the VTP hot path on MI355X.

The reference ships the model side of training only (VTP.forward(forward_type=...), vtp/models/vtp.py:323-338): no
loss, optimizer or DDP wrapper.  This module is that missing driver, MI355X-first:

  * one process per GPU, full replica, minibatch sharded by rank (the reference's only strategy is DP);
  * forward/backward are hand-scheduled kernel sequences (vtp_amd.engine), gradients land in ONE flat fp32 buffer;
  * gradient all-reduce = a few large contiguous RCCL buckets launched *during* backward (the c10d NCCL/RCCL backend
    runs them on its own HIP stream; they overlap the remaining backward kernels) and waited on before the optimizer;
    xGMI is point-to-point, so few large messages beat many small ones;
  * the contrastive head exchanges L2-normalised image/text features with one all-gather each and returns the
    cross-rank feature gradients with one reduce-scatter each (OpenCLIP local_loss + gather_with_grad semantics);
  * the whole step is captured once and replayed -- as ONE hipGraph without collectives, as a short chain of segments with the
    collectives between them otherwise; side work is issued behind the main stream's next kernel so that the main chain replays on
    one hardware queue (engine.Overlap.defer); hyper-parameters live in device memory so the replay sees per-step values;
  * one fused AdamW launch per contiguous parameter range + one batched bf16-weight refresh launch.

Objectives (OUR spec -- the reference defines no loss; parity unpinned):
  rec  = mean |decode(encode(x)) - x|                       (L1)
  clip = 0.5 * (CE(s I T^T) + CE(s T I^T)), s = exp(logit_scale), computed on the SAME trunk forward as `rec`
         (drop rates are 0 and the input is the same image, so trunk(image) is identical for both objectives and the
         shared forward/backward is mathematically the sum of the two separate passes).
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops
from .engine import BF, F32, OVERLAP


class GradBucketer:
    """Bucketed asynchronous all-reduce over contiguous ranges of a flat gradient buffer.

    Pure torch.distributed (works with gloo on CPU for tests, nccl==RCCL on MI355X)."""

    def __init__(self, flat_g: torch.Tensor, group=None, shard: bool = False, grad_dtype: torch.dtype = torch.float32,
                 force: bool = False):
        import torch.distributed as dist
        self.dist = dist
        self.flat_g = flat_g
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if self.world > 1 else 0
        # `force`: issue every collective even in a one-rank group (they are identities there) -- puts the RCCL code path on
        # hardware on a one-GPU box (tests/test_rccl_gpu.py)
        self.active = self.world > 1 or (bool(force) and dist.is_available() and dist.is_initialized())
        self.works = []
        self.reduced_elems = 0
        # sharded mode (reduce-scatter + rank-sharded AdamW + parameter all-gather): every bucket [lo, hi) is cut into
        # `world` equal chunks (8-element aligned, the last one zero-padded); rank r owns chunk r of every bucket
        self.shard = bool(shard) and self.active
        self.grad_dtype = grad_dtype
        self.shards: dict = {}      # (lo, hi) -> ShardRec
        self.comm_bytes = 0

    class ShardRec:
        __slots__ = ("lo", "hi", "chunk", "a", "b", "send", "g_out", "g32", "p_send", "p_recv")

    def _rec(self, lo: int, hi: int):
        rec = self.shards.get((lo, hi))
        if rec is None:
            rec = self.ShardRec()
            n, W, dev = hi - lo, self.world, self.flat_g.device
            rec.lo, rec.hi = lo, hi
            rec.chunk = (n + W * 8 - 1) // (W * 8) * 8
            rec.a = min(lo + self.rank * rec.chunk, hi)
            rec.b = min(rec.a + rec.chunk, hi)
            rec.send = torch.zeros(rec.chunk * W, dtype=self.grad_dtype, device=dev)   # padded copy / cast of the gradients
            rec.g_out = torch.zeros(rec.chunk, dtype=self.grad_dtype, device=dev)      # this rank's reduced chunk
            rec.g32 = rec.g_out if self.grad_dtype == torch.float32 else torch.zeros(rec.chunk, dtype=torch.float32, device=dev)
            rec.p_send = torch.zeros(rec.chunk, dtype=torch.float32, device=dev)
            rec.p_recv = torch.zeros(rec.chunk * W, dtype=torch.float32, device=dev)
            self.shards[(lo, hi)] = rec
        return rec

    def native(self) -> bool:
        return self.dist.get_backend(self.group) == "nccl"

    def reduce_scatter_range(self, lo: int, hi: int):
        """Launch (async) the sum-reduce-scatter of flat_g[lo:hi]: rank r receives chunk r in rec.g_out."""
        rec = self._rec(lo, hi)
        n = hi - lo
        # fp32 bucket that divides into `world` whole chunks (no padding) on RCCL: reduce-scatter straight out of the flat gradient
        # buffer -- no staging copy (nothing writes this range again before the optimizer: its gradients are complete)
        direct = self.grad_dtype == torch.float32 and n == rec.chunk * self.world and self.native()
        if direct:
            src = self.flat_g[lo:hi]
        elif self.grad_dtype == torch.float32:
            rec.send[:n].copy_(self.flat_g[lo:hi])
            src = rec.send
        else:
            ops.cast_f32_bf16(self.flat_g[lo:hi], rec.send, n)
            src = rec.send
        if self.native():
            w = self.dist.reduce_scatter_tensor(rec.g_out, src, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
            self.works.append((w, None))
        else:  # gloo has no reduce-scatter (and no bf16 on device tensors): all-reduce in fp32, keep the own chunk
            tmp = rec.send.float()
            w = self.dist.all_reduce(tmp, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
            self.works.append((w, lambda: rec.g_out.copy_(tmp[self.rank * rec.chunk:(self.rank + 1) * rec.chunk])))
        self.reduced_elems += n
        self.comm_bytes += n * rec.send.element_size()

    def reduce_range(self, lo: int, hi: int):
        """Launch (async) sum-all-reduce of flat_g[lo:hi]."""
        if not self.active or hi <= lo:
            return
        if self.shard:
            return self.reduce_scatter_range(lo, hi)
        w = self.dist.all_reduce(self.flat_g[lo:hi], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
        self.works.append((w, None))
        self.reduced_elems += hi - lo
        self.comm_bytes += (hi - lo) * 4

    def wait(self, works=None):
        """wait for the given (work, after) pairs, or for everything launched since the last wait"""
        mine = works is None
        for w, after in (self.works if mine else works):
            w.wait()
            if after is not None:
                after()
        if mine:
            self.works = []

    def all_gather_params(self, flat_p: torch.Tensor, recs):
        """Every rank contributes its (freshly updated) chunk of each bucket; afterwards rec.p_recv holds the whole bucket."""
        works = []
        for rec in recs:
            if self.native():
                works.append((self.dist.all_gather_into_tensor(rec.p_recv, rec.p_send, group=self.group, async_op=True), None))
            else:
                rec.p_recv.zero_()
                rec.p_recv[self.rank * rec.chunk:(self.rank + 1) * rec.chunk].copy_(rec.p_send)
                works.append((self.dist.all_reduce(rec.p_recv, group=self.group, async_op=True), None))
            self.comm_bytes += rec.p_recv.numel() * 4
        for w, _ in works:
            w.wait()


class HostStager:
    """Per-step host -> device upload of small index / mask arrays WITHOUT stalling the host: the arrays of one batch are packed
    into a slot of a PINNED host ring and sent with ONE non-blocking copy.  (A plain `torch.as_tensor(numpy_array, device=...)`
    copies from pageable memory, and PyTorch synchronises the stream for that: the host would wait for the whole previous step
    before it can prepare the next one -- measured 45 ms of a 54 ms step spent inside prepare_ssl.)

    Lifetimes: only the pinned HOST slots are recycled (a slot is rewritten after the copy that read it has executed: its
    event).  The DEVICE side of every upload is a fresh allocation from torch's caching allocator that the returned tensors own
    -- a loader may prepare any number of batches ahead and a caller may keep an `ssl` dict across later prepare_ssl calls
    (the earlier version handed out views of a 4-slot device ring, which the 5th upload overwrote in place)."""

    def __init__(self, device, slots: int = 4):
        self.device, self.n, self.i = device, slots, 0
        self.host = [None] * slots
        self.events = [None] * slots
        self.wait_s = 0.0  # host seconds spent waiting for a slot's previous upload (back-pressure: the host runs AHEAD of the GPU)

    def upload(self, arrays: dict) -> dict:
        import numpy as np
        plan, off = [], 0
        for k, a in arrays.items():
            a = np.ascontiguousarray(a)
            plan.append((k, a, off))
            off += (a.nbytes + 15) // 16 * 16
        total = max(off, 16)
        slot = self.i
        self.i = (self.i + 1) % self.n
        if self.events[slot] is not None:
            import time
            t0 = time.perf_counter()
            self.events[slot].synchronize()
            self.wait_s += time.perf_counter() - t0
        if self.host[slot] is None or self.host[slot].numel() < total:
            self.host[slot] = torch.empty(max(total * 2, 1 << 16), dtype=torch.uint8).pin_memory()
        h = self.host[slot]
        hn = h.numpy()
        for k, a, o in plan:
            hn[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
        d = torch.empty(total, dtype=torch.uint8, device=self.device)  # owned by the tensors returned below
        d.copy_(h[:total], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[slot] = ev
        out = {}
        for k, a, o in plan:
            t = d[o:o + a.nbytes]
            out[k] = t.view(_NP2TORCH[a.dtype.name]).view(a.shape)
        # the packed device buffer itself and where each array sits in it: a consumer that keeps STATIC copies of the arrays (the
        # hipGraph driver) refreshes all of them with one device copy when the layouts agree
        out["_packed"] = (d, tuple((k, o, a.nbytes, a.dtype.name, tuple(a.shape)) for k, a, o in plan))
        return out


_NP2TORCH = {"int32": torch.int32, "float32": torch.float32, "uint8": torch.uint8, "int64": torch.int64}


def merge_ranges(ranges: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
    out: List[Tuple[int, int]] = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def uncovered(lo: int, hi: int, covered: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """the parts of [lo, hi) that none of the (merged, sorted) `covered` ranges contains"""
    out, x = [], lo
    for a, b in covered:
        if b <= x or a >= hi:
            continue
        if a > x:
            out.append((x, a))
        x = max(x, b)
    if x < hi:
        out.append((x, hi))
    return out


def param_ranges(offsets, prefixes: Sequence[str]) -> List[Tuple[int, int]]:
    """Contiguous [lo,hi) ranges (4-element aligned) of the flat buffers covering every parameter whose name starts
    with one of `prefixes`."""
    r = []
    for name, (o, k) in offsets.items():
        if any(name.startswith(p) for p in prefixes):
            r.append((o, o + (k + 3) // 4 * 4))
    return merge_ranges(r)


def lane_pieces(ranges: Sequence[Tuple[int, int]], pairs: Sequence[Tuple[int, int, int]]) -> List[Tuple[int, int, Optional[int]]]:
    """Cut the flat ranges of a gradient bucket at the borders of the EMA-tracked parameter groups.  pairs = [(teacher_lo, student_lo,
    student_hi)]: the teacher's copy of student element x in [student_lo, student_hi) is element teacher_lo + (x - student_lo).  Returns
    [(lo, hi, teacher_lo_of_the_piece | None)]: every piece lies inside one group (fused AdamW + EMA) or outside all of them."""
    pieces = []
    for lo, hi in ranges:
        cuts = sorted({lo, hi} | {x for _, slo, shi in pairs for x in (slo, shi) if lo < x < hi})
        for a, b in zip(cuts, cuts[1:]):
            tl = next((tlo + (a - slo) for tlo, slo, shi in pairs if slo <= a and b <= shi), None)
            pieces.append((a, b, tl))
    return pieces


NO_DECAY_NAMES = ("logit_scale", "logit_bias", "cls_token", "mask_token", "positional_embedding", "storage_tokens")


def default_no_decay(name: str, shape: tuple) -> bool:
    return len(shape) < 2 or name.rsplit(".", 1)[-1] in NO_DECAY_NAMES


def _max_norm_value(value) -> float:
    """VTPTrainer(max_grad_norm=...): a number > 0 (float("inf") allowed)"""
    try:
        f = float(value)
    except (TypeError, ValueError):
        f = None
    if f is None or isinstance(value, bool) or not f > 0:
        raise ValueError(f"max_grad_norm must be None or a number > 0 (float('inf') allowed), got {value!r}")
    return f


def _skip_nonfinite_value(value, max_grad_norm) -> bool:
    """VTPTrainer(skip_nonfinite=...): a bool; True needs the clipping machinery (the norm is known before any bucket is updated)"""
    if not isinstance(value, bool):
        raise ValueError(f"skip_nonfinite must be True or False, got {value!r}")
    if value and max_grad_norm is None:
        raise ValueError("skip_nonfinite=True needs max_grad_norm to be a number: the decision is taken on the global gradient norm "
                         "(max_grad_norm=float('inf') measures it without clipping)")
    return value


MAX_PARAM_GROUPS = 128  # one table row per (group, decay-exempt) pair, 256 rows at most (csrc/elementwise.hip)


def _group_scale(group: dict, key: str) -> float:
    value = group.get(key, 1.0)
    try:
        f = float(value)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(value, bool) or not (math.isfinite(f) and f >= 0):
        raise ValueError(f"param group {group.get('name')!r}: {key} must be a finite number >= 0, got {value!r}")
    return f


def resolve_param_groups(param_groups, shapes: dict, no_decay=None):
    """VTPTrainer(param_groups=...) on the host.  param_groups: [{"name", "match": tuple of name prefixes | callable (name, shape) ->
    bool, "lr_scale" = 1.0, "wd_scale" = 1.0}]; shapes: parameter name -> shape (the keys of store.offsets); no_decay: None or a
    predicate (name, shape) -> bool.  The first matching group takes a parameter; what no group matches falls into an implicit last
    group "default" with scales (1, 1).  Returns (groups, rows): `groups` the list the trainer exposes (dicts {"name", "lr_scale",
    "wd_scale"}, in table order), `rows` parameter name -> table row = 2 * group index + (1 if the parameter is exempt from decay)."""
    user = []
    for g in param_groups:
        if not isinstance(g, dict) or "name" not in g or "match" not in g:
            raise ValueError(f"a param group is a dict with 'name' and 'match', got {g!r}")
        unknown = set(g) - {"name", "match", "lr_scale", "wd_scale"}
        if unknown:
            raise ValueError(f"param group {g['name']!r}: unknown keys {sorted(unknown)}")
        match = g["match"]
        if isinstance(match, str):
            match = (match,)
        if not callable(match):
            match = tuple(match)
            if not match or not all(isinstance(x, str) for x in match):
                raise ValueError(f"param group {g['name']!r}: match must be a tuple of name prefixes or a callable (name, shape) -> bool")
        user.append(({"name": str(g["name"]), "lr_scale": _group_scale(g, "lr_scale"), "wd_scale": _group_scale(g, "wd_scale")}, match))
    names = [g["name"] for g, _ in user]
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise ValueError(f"duplicate param group names: {dup}")
    if len(user) > MAX_PARAM_GROUPS:
        raise ValueError(f"{len(user)} param groups: at most {MAX_PARAM_GROUPS} are supported")
    rows, hit, rest = {}, [False] * len(user), False
    for name, shape in shapes.items():
        shape = tuple(shape)
        gi = next((i for i, (_, match) in enumerate(user)
                   if (match(name, shape) if callable(match) else name.startswith(match))), len(user))
        if gi < len(user):
            hit[gi] = True
        else:
            rest = True
        rows[name] = 2 * gi + (1 if no_decay is not None and no_decay(name, shape) else 0)
    empty = [g["name"] for (g, _), h in zip(user, hit) if not h]
    if empty:
        raise ValueError(f"param groups that match no parameter: {empty}")
    groups = [g for g, _ in user]
    if rest:
        if "default" in names:
            raise ValueError("duplicate param group names: ['default'] (the implicit group of the unmatched parameters)")
        if len(groups) == MAX_PARAM_GROUPS:
            raise ValueError(f"{MAX_PARAM_GROUPS} param groups and unmatched parameters: the implicit 'default' group would be one too many")
        groups.append({"name": "default", "lr_scale": 1.0, "wd_scale": 1.0})
    return groups, rows


def group_table(groups) -> List[float]:
    """the device table of this step: rows {lr_scale, wd_scale}, two per group -- row 2i for its decayed parameters, row 2i + 1 for
    those that no_decay exempts (wd_scale 0 whatever the group says)"""
    vals = []
    for g in groups:
        ls, ws = _group_scale(g, "lr_scale"), _group_scale(g, "wd_scale")
        vals += [ls, ws, ls, 0.0]
    return vals


_LAYER0 = ("cls_token", "mask_token", "storage_tokens", "register_tokens", "pos_embed", "positional_embedding", "rope_embed.")


def layerwise_lr_decay(names, depth: int, decay: float, patch_embed_lr_mult: float = 1.0, prefix: str = "trunk."):
    """DINOv2's layer-wise learning-rate decay as a param_groups list.  Of the parameters under `prefix`, patch_embed.*, the cls /
    mask / storage tokens and positional tables have layer id 0, blocks.i.* have i + 1, everything else (the final norm) depth + 1;
    lr_scale = decay ** (depth + 1 - layer id), times patch_embed_lr_mult for patch_embed.*.  Parameters outside `prefix` are left
    to the default group; parameters with equal scales share a group."""
    import re
    by_scale: dict = {}
    for name in names:
        if not name.startswith(prefix):
            continue
        local = name[len(prefix):]
        blk = re.match(r"blocks\.(\d+)\.", local)
        patch = local.startswith("patch_embed.")
        if patch or local.startswith(_LAYER0):
            layer = 0
        elif blk:
            layer = int(blk.group(1)) + 1
        else:
            layer = depth + 1
        scale = decay ** (depth + 1 - layer)
        if patch:
            scale *= patch_embed_lr_mult
        label = f"layer{layer}" + (".patch_embed" if patch else "")
        labels, members = by_scale.setdefault(scale, ([], set()))
        if label not in labels:
            labels.append(label)
        members.add(name)
    return [{"name": prefix + "+".join(labels), "match": (lambda name, shape, members=frozenset(members): name in members),
             "lr_scale": scale, "wd_scale": 1.0} for scale, (labels, members) in by_scale.items()]


CLIP_PREFIXES = ("visual_proj.", "text_transformer.", "token_embedding.", "positional_embedding", "ln_final.",
                 "text_projection", "logit_scale", "logit_bias")


class VTPTrainer:
    """Trainer for the reconstruction (+ optional contrastive) objectives: BASELINE config 2 and the rec + clip parts of
    config 3.  `step(images)` = rec only; `step(images, text)` = rec + clip."""

    def __init__(self, model, lr: float = 1e-4, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 0.05,
                 group=None, bucket_blocks: int = 3, use_graphs: bool = False, clip_weight: float = 1.0,
                 rec_weight: float = 1.0, dino_weight: float = 1.0, ibot_weight: float = 1.0, student_temp: float = 0.1,
                 teacher_temp: float = 0.07, center_momentum: float = 0.9, teacher_momentum: float = 0.994,
                 lpips=None, perceptual_weight: float = 0.0, drop_rate: float = 0.0, decoder_drop_rate: float = 0.0,
                 clip_drop_rate: Optional[float] = None, ssl_drop_rate: Optional[float] = None, rec_drop_rate: Optional[float] = None,
                 drop_seed: int = 0, centering: str = "softmax", koleo_weight: float = 0.0, sk_iterations: int = 3,
                 shard_optimizer: Optional[bool] = None, grad_dtype: str = "fp32", no_decay="default",
                 force_collectives: bool = False, max_grad_norm: Optional[float] = None, param_groups=None,
                 skip_nonfinite: bool = False):
        """lpips: a vtp_amd.LPIPS module (frozen, weights loaded by the caller) -- with perceptual_weight > 0 the
        reconstruction objective is rec_weight * L1 + perceptual_weight * mean_b LPIPS(decoded_b, image_b).
        max_grad_norm: global gradient-norm clipping in front of AdamW (torch.nn.utils.clip_grad_norm_, norm_type 2); the step's
        pre-clip norm and coefficient land in self.grad_norm / self.grad_clip_coef (device tensors).  None: no clipping.
        param_groups: per-group learning-rate / weight-decay scales (resolve_param_groups; layerwise_lr_decay builds DINOv2's list):
        group g runs AdamW with lr * lr_scale and weight_decay * wd_scale.  self.param_groups lists them; its scales are read at
        every step() (a scheduler may mutate them; no re-capture).  None: one lr / weight decay for every parameter.
        skip_nonfinite: a step whose global gradient norm is inf or NaN runs to completion but updates nothing (parameters, moments,
        bf16 copies, EMA teacher and Adam's step count keep their values); decided on the device, no host sync.  Needs max_grad_norm
        (float("inf"): no clipping).  self.step_skipped / self.skipped_steps (device int32 [1]) report the last step / the total.
        With it on, self.betas must keep the constructor's values (step() raises otherwise)."""
        self._skip = _skip_nonfinite_value(skip_nonfinite, max_grad_norm)
        self.model = model
        # stochastic depth (block.py:207-289): the student trunk's rate per objective (clip_drop_rate / ssl_drop_rate / rec_drop_rate,
        # vtp.py:205-207; `drop_rate` sets all three) and the pixel decoder's drop_path_rate.  The objectives are items of ONE list
        # forward, each with its own rate and its own image subsets; rec and clip share an item only when they see the same tensor
        # at the same rate (step(..., reconstruction_image=...))
        self.drop_rate, self.decoder_drop_rate = float(drop_rate), float(decoder_drop_rate)
        self.clip_drop_rate = self.drop_rate if clip_drop_rate is None else float(clip_drop_rate)
        self.ssl_drop_rate = self.drop_rate if ssl_drop_rate is None else float(ssl_drop_rate)
        self.rec_drop_rate = self.drop_rate if rec_drop_rate is None else float(rec_drop_rate)
        self._drop_gen = torch.Generator().manual_seed(int(drop_seed))
        # SSL loss variants (DINOv2 conventions): teacher-target centring "softmax" (EMA centre) or
        # "sinkhorn_knopp"; KoLeo regulariser on the student's global cls tokens (per view) with weight koleo_weight
        if centering not in ("softmax", "sinkhorn_knopp"):
            raise ValueError(f"centering must be 'softmax' or 'sinkhorn_knopp', got {centering!r}")
        self.centering, self.koleo_weight, self.sk_iterations = centering, float(koleo_weight), int(sk_iterations)
        self.koleo_loss_sum = None
        self.lpips, self.perceptual_weight = lpips, float(perceptual_weight)
        if self.perceptual_weight > 0 and lpips is None:
            raise ValueError("perceptual_weight > 0 needs an LPIPS module")
        self.lpips_val = None  # per-image LPIPS of the last step (device f32 [B])
        self._text_stream = None
        self.store = model._engine()
        self.trunk, self.decoder = model._trunk, model._decoder
        self.text, self.clip = model._text, model._clip
        if self.decoder is None:
            raise RuntimeError("VTPTrainer needs train_reconstruction=True")
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self._skip_betas = (float(betas[0]), float(betas[1]))  # the guarded finalize bakes them into its launch: fixed at construction
        self.clip_weight, self.rec_weight = clip_weight, rec_weight
        self.dino_weight, self.ibot_weight = dino_weight, ibot_weight
        self.student_temp, self.teacher_temp = student_temp, teacher_temp
        self.center_momentum, self.teacher_momentum = center_momentum, teacher_momentum
        self.ssl_head = getattr(model, "_head", None)  # vtp_amd.VTP only
        st = self.store
        self.ranges_rec = param_ranges(st.offsets, ("trunk.", "pixel_decoder."))
        self.ranges_all = param_ranges(st.offsets, ("trunk.", "pixel_decoder.") + CLIP_PREFIXES)
        self.ranges_ssl = param_ranges(st.offsets, ("dino_head.",))
        if self.ssl_head is not None:
            K = self.ssl_head.K
            self.center_dino = torch.zeros(K, dtype=F32, device=st.device)
            self.center_ibot = torch.zeros(K, dtype=F32, device=st.device)
            self.center_stats = torch.zeros(2 * K + 8, dtype=F32, device=st.device)  # [sum_dino | sum_ibot | n_masked, pad]
            self.ssl_loss_sum = torch.zeros(1, dtype=F32, device=st.device)
            self.koleo_loss_sum = torch.zeros(1, dtype=F32, device=st.device)
        self._ssl_static = {}
        self._stager = None  # pinned staging ring for the per-step SSL index arrays (prepare_ssl)
        self.ssl_bucket = int(os.environ.get("VTP_SSL_BUCKET", "512"))  # masked-token rows are padded to a multiple of this
        self.m = torch.zeros_like(st.flat_p)
        self.v = torch.zeros_like(st.flat_p)
        # weight-decay exemptions (the usual AdamW recipe of OpenCLIP / DINOv2 training loops; the reference ships no optimizer):
        # no_decay = "default" (biases, norm / LayerScale gains, tokens, positional embeddings, logit scale / bias -- every
        # parameter with ndim < 2 or one of the named tensors), None (decay everything) or a predicate (name, shape) -> bool.
        # One flag per float4 of the flat buffer (parameters are padded to 4 elements).
        if no_decay == "default":
            no_decay = default_no_decay
        self.nodecay4 = None
        if no_decay is not None:
            flags = torch.zeros(st.numel // 4, dtype=torch.uint8)
            for name, (o, k) in st.offsets.items():
                if no_decay(name, tuple(st.params[name].shape)):
                    flags[o // 4:(o + (k + 3) // 4 * 4) // 4] = 1
            self.nodecay4 = flags.to(st.device)
        # per-group lr / weight-decay scales: one table row index per float4 where nodecay4 holds one flag, and a device table of
        # {lr_scale, wd_scale} rows that _set_hyper refreshes every step (two rows per group: decayed / exempt -- no_decay composes)
        self.param_groups = self.group_tab = self._group4 = self._group_ring = None
        if param_groups is not None:
            shapes = {name: tuple(st.params[name].shape) for name in st.offsets}
            self.param_groups, rows = resolve_param_groups(param_groups, shapes, no_decay)
            idx = torch.zeros(st.numel // 4, dtype=torch.uint8)
            for name, (o, k) in st.offsets.items():
                idx[o // 4:(o + (k + 3) // 4 * 4) // 4] = rows[name]
            self._group4 = idx.to(st.device)
            self.group_tab = torch.tensor(group_table(self.param_groups), dtype=F32, device=st.device).view(-1, 2)
        self.step_no = 0
        self.loss_sum = torch.zeros(1, dtype=F32, device=st.device)       # L1 numerator
        self.clip_loss_sum = torch.zeros(1, dtype=F32, device=st.device)  # contrastive loss (already a mean)
        # data-parallel gradient exchange: "all-reduce + replicated AdamW" (default) or, with shard_optimizer (env
        # VTP_SHARD_OPT=1), "reduce-scatter + AdamW on this rank's 1/world of every bucket + parameter all-gather"; grad_dtype
        # "bf16" halves the reduce-scatter volume (sharded mode only; the local fp32 gradients are rounded once before the sum)
        if shard_optimizer is None:
            shard_optimizer = os.environ.get("VTP_SHARD_OPT", "0") == "1"
        if grad_dtype not in ("fp32", "bf16"):
            raise ValueError(f"grad_dtype must be 'fp32' or 'bf16', got {grad_dtype!r}")
        if grad_dtype == "bf16" and not shard_optimizer:
            raise ValueError("grad_dtype='bf16' needs shard_optimizer=True (the all-reduce path reduces the flat fp32 buffer in place)")
        self.bucketer = GradBucketer(st.flat_g, group, shard=shard_optimizer, grad_dtype=BF if grad_dtype == "bf16" else F32,
                                     force=force_collectives)
        self.shard_optimizer = self.bucketer.shard
        self._shard_layout = None  # bucket boundaries of the first sharded step (chunk ownership of the Adam moments)
        # OPTIMIZER LANE (round 5; VTP_OPT_OVERLAP=0 restores the serial leg): as soon as the gradients of a bucket are final (and,
        # with several ranks, reduced) its fused AdamW + EMA-teacher update and the refresh of ITS bf16 weight copies run on a side
        # stream beside the backward of the remaining layers, instead of one AdamW + one EMA + one refresh launch over everything
        # after the last backward kernel (2.6 ms of a 46.7 ms step, serial).  The step-start gradient zeroing likewise runs on a side
        # stream under the forward pass.  Replicated-AdamW mode only (the rank-sharded optimizer keeps its own leg).
        self.overlap_opt = (not self.shard_optimizer) and os.environ.get("VTP_OPT_OVERLAP", "1") not in ("0", "false", "off")
        self._opt_stream = self._zero_stream = None
        self._opt_plans = {}
        self._opt_busy = self._zero_busy = False
        # the SSL head's loss + backward on its own stream beside the decoder forward (one GPU / no collectives; VTP_HEAD_OVERLAP=0: in line)
        self.head_overlap = os.environ.get("VTP_HEAD_OVERLAP", "1") not in ("0", "false", "off")
        self._head_stream, self._head_keys = None, []
        self._works_prev = []  # (work, after) pairs of the previous bucket event's reductions (_handle)
        self.collectives = self.bucketer.active  # world > 1, or a one-rank group with force_collectives
        if self.collectives:
            # RCCL's channels hold CUs while the backward runs: the persistent GEMMs draw their tiles instead of owning static lists
            # (csrc/gemm8p.hip DYN; tools/cu_thief.py: a chain of the step's GEMMs beside 32 held CUs x1.02 instead of x1.18)
            from . import _lib
            _lib.load().vtp_set_gemm_dynamic(1)
        self.time_comm = False       # bench: record HIP events around every point where the main stream waits for RCCL
        self._comm_events = []
        self.world, self.rank, self.group = self.bucketer.world, self.bucketer.rank, group
        for eng in self._aug_engines():  # train-time RoPE augmentations: one stream per (seed, rank, engine), as the reference's per-rank RNG
            eng.rope_aug.reseed(drop_seed, self.rank)
        self._graph_aug = {}  # graph key -> [(engine, record keys its captured segments read)]
        self.bucket_blocks = bucket_blocks
        self._bucket_plan = self._plan_buckets()
        # hyper-parameters live in device memory so that captured hipGraphs replay with per-step values
        self.hyper = torch.zeros(16, dtype=F32, device=st.device)  # [lr b1 b2 eps wd bc1 sqrt(bc2) 1/world | 1/teacher_temp ema_m ...]
        self.momentum_dev = self.hyper[9:10]  # EMA teacher momentum of this step
        # GLOBAL GRADIENT-NORM CLIPPING (max_grad_norm; torch.nn.utils.clip_grad_norm_, norm_type 2) over exactly the gradient AdamW
        # reads: every range the step's AdamW updates gets fp64 sum-of-squares partials (one per chunk, csrc/gradnorm.hip) in a static
        # partials buffer, in the step's fixed launch order; one finalize launch adds them in a fixed order, writes grad_norm /
        # grad_clip_coef and folds the coefficient into the gradient multiplier hyper[7] that the AdamW kernels read.  No float
        # atomics: replicas that hold the same reduced gradients compute the same coefficient bit for bit.  max_norm lives in hyper[10]
        # (a change between steps needs no re-capture).  With the optimizer lane, a bucket's lane work shrinks to its partials: its
        # AdamW + EMA + weight refresh wait for the last bucket, in the optimizer leg.
        self._clip = max_grad_norm is not None
        self._max_grad_norm = _max_norm_value(max_grad_norm) if self._clip else None
        self.grad_norm = self.grad_clip_coef = self._clip_partials = self._clip_sum = None
        self._clip_ranges, self._clip_cursor, self._clip_keys = {}, 0, []
        if self._clip:
            self.grad_norm = torch.zeros(1, dtype=F32, device=st.device)       # pre-clip total norm of the last step
            self.grad_clip_coef = torch.zeros(1, dtype=F32, device=st.device)  # its clip coefficient (1 = not clipped)
            # every range of a step is disjoint from the others and lies inside the flat buffer, and each is a union of parameters
            cap = ops.sumsq_partials_count(st.numel) + len(st.offsets)
            self._clip_partials = torch.zeros(cap, dtype=torch.float64, device=st.device)
            self._clip_sum = torch.zeros(1, dtype=torch.float64, device=st.device)  # sharded optimizer: this rank's sum, all-reduced
        # SKIPPING A STEP WHOSE GRADIENT NORM IS NOT FINITE (skip_nonfinite): the clip finalize decides on the device (the step is a
        # replayed hipGraph: the host cannot look at the norm without a sync) and every update kernel of the step reads the decision,
        # skip_now, and stores nothing when it is set.  Adam's step count lives in the same device block -- a skipped step must not
        # advance it, and the host does not know which steps were skipped: the finalize overwrites the host-computed bias
        # corrections hyper[5:7] (_set_hyper) from it, in front of the step's first AdamW launch.  self.step_no stays the number of
        # ATTEMPTED steps.  Out of scope: the SSL centres follow the teacher's outputs, which do not depend on this step's gradients,
        # and the loss accumulators of a bad step read NaN -- the signal a user wants.
        self._skip_state = self.step_skipped = self.skipped_steps = None
        if self._skip:
            self._skip_state = torch.zeros(4, dtype=torch.int32, device=st.device)  # {applied_steps, skipped_steps, skip_now, -}
            self.skipped_steps = self._skip_state[1:2]  # steps skipped since construction / load_state_dict
            self.step_skipped = self._skip_state[2:3]   # 1 after a skipped step, else 0
        self._hyper_ring = None
        self.use_graphs = use_graphs
        self._graphs = {}
        # Without collectives nothing has to run BETWEEN graph segments: the whole step is captured as ONE hipGraph, the optimizer lane
        # left forked across the bucket events and joined once, in front of the optimizer leg (VTP_SINGLE_GRAPH=0: one segment per
        # bucket event, as with collectives).  Round 5 measured this at +-0 -- with the side branches captured in front of the main
        # stream's kernels, which put every block's closing norm backward on the weight-gradient branch's queue (engine.Overlap.defer);
        # with the main chain on one queue the segment boundaries are what is left between blocks: 44.72 -> 44.38 ms, same box
        self.single_graph = (not self.collectives) and os.environ.get("VTP_SINGLE_GRAPH", "1") in ("1", "true", "on")
        if self.text is not None and model.config.text_pool_type == "none":
            self._clip_unsupported = "the contrastive objective needs pooled text features (text_pool_type argmax | first | last)"
        elif self.text is not None and model.config.vision_clip_feat == "pooled" and model.config.vision_embed_dim > 1024:
            # the final-norm backward that takes the pooled feature's gradient (vtp_norm_bwd_pvec) has rows up to 1024 wide
            self._clip_unsupported = (f"vision_clip_feat='pooled' needs vision_embed_dim <= 1024 on the fused step "
                                      f"(got {model.config.vision_embed_dim}); the autograd path (model(...); loss.backward()) has no limit")
        else:
            self._clip_unsupported = None
        self.sync_replicas()

    @property
    def max_grad_norm(self) -> Optional[float]:
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        """a new clipping threshold takes effect from the next step (device memory: no re-capture); clipping itself is decided at
        construction (its buffers and launches are part of the captured step)"""
        if (value is None) != (self._max_grad_norm is None):
            raise ValueError("max_grad_norm: clipping cannot be switched on or off after construction; build the trainer with "
                             "max_grad_norm=None or with a number")
        self._max_grad_norm = None if value is None else _max_norm_value(value)

    @property
    def skip_nonfinite(self) -> bool:
        """decided at construction, like clipping: the guard is part of the captured step"""
        return self._skip

    def sync_replicas(self):
        """Data-parallel replicas must start from identical state (what DDP's constructor does with its parameter / buffer
        broadcast): rank 0's fp32 masters (student AND EMA teacher), Adam moments and SSL centres go to every rank."""
        if not self.collectives:
            return
        dist, st = self.bucketer.dist, self.store
        bufs = [st.flat_p, self.m, self.v]
        if self._skip:
            bufs.append(self._skip_state)
        if self.ssl_head is not None:
            bufs += [self.center_dino, self.center_ibot]
        for b in bufs:
            dist.broadcast(b, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)
        st.prep()
        self.model._pver = self.model._param_version()

    # gradient buckets in backward-completion order
    def _plan_buckets(self):
        off = self.store.offsets

        def rng(*prefixes):
            return param_ranges(off, prefixes)

        plan = {"dec_tail": rng("pixel_decoder.norm.", "pixel_decoder.proj_out."),
                "dec_head": rng("pixel_decoder.proj_in."),
                "trunk_tail": rng("trunk.norm.", "trunk.feature_bottleneck."),
                "trunk_head": rng("trunk.cls_token", "trunk.mask_token", "trunk.patch_embed."),
                "text_tail": rng("ln_final.", "text_projection"),
                "text_head": rng("token_embedding.", "positional_embedding"),
                "clip_head": rng("visual_proj.", "logit_scale", "logit_bias"), "dino_head": rng("dino_head.")}
        towers = [("dec", "pixel_decoder.blocks.", self.decoder.depth), ("trunk", "trunk.blocks.", self.trunk.depth)]
        if self.text is not None:
            towers.append(("text", "text_transformer.resblocks.", self.text.depth))
        for key, prefix, depth in towers:
            for i in range(depth):
                plan[f"{key}.{i}"] = rng(f"{prefix}{i}.")
        return plan

    def _reduce(self, keys: Sequence[str]):
        if not self.collectives or not keys:
            return
        rs = merge_ranges([r for k in keys for r in self._bucket_plan[k]])
        for lo, hi in rs:
            self.bucketer.reduce_range(lo, hi)

    # ------------------------------------------------------------------------------------------------------------
    # The step is written ONCE as a generator.  It yields either
    #   * a list of bucket keys: the gradients of those parameter groups are complete -> the driver launches their RCCL
    #     all-reduce (eager) / ends a hipGraph segment there and launches the all-reduce between segments; or
    #   * a callable: a collective that must run between segments (feature all-gather / reduce-scatter).
    # ------------------------------------------------------------------------------------------------------------
    def _tower_backward(self, tower: str, gen, depth: int):
        nb = self.bucket_blocks
        result = None
        try:
            while True:
                ev = next(gen)
                if ev == "tail":
                    yield [f"{tower}_tail"]
                elif ev[0] == "block" and ev[1] % nb == 0:
                    i = ev[1]
                    yield [f"{tower}.{j}" for j in range(i, min(i + nb, depth))]
        except StopIteration as stop:
            result = stop.value
        return result

    def _ssl_gen(self, P, lead_images=None):
        """SSL leg of the step: teacher forward, ONE student list forward (lead images of the rec / clip objectives +
        masked global crops + local crops), DINO + iBOT loss, head backward, and the scatter of the head's input gradient
        into the trunk's d_xnf rows.  The trunk backward itself is run once by the caller, over all items.  Returns the
        ssl_forward() dict."""
        from .vtp import ssl_forward
        out = ssl_forward(self.model, P["global"], P["local"], P["masks"], P["plan"], P["dev"], train=True, lead_images=lead_images,
                          tail_rows="student_tail_src" in P["dev"])
        self._zero_join()  # the gradient buffer was zeroed under the forward passes; the head backward below is its first writer
        if not (self.head_overlap and not self.collectives and OVERLAP.enabled):
            yield from self._ssl_tail(out, P)
            return out
        # HEAD STREAM (no collectives: the tail below yields nothing but its bucket key): teacher softmax / centring, DINO + iBOT
        # cross-entropy, the head backward and the scatter into d_xnf -- 1.2 ms of mostly HBM-bound kernels, one at a time -- run on
        # their own stream beside the decoder forward / text tower / CLIP loss (MFMA-bound, few tiles); joined in front of the trunk
        # backward, where the head's bucket is announced (_step_body).  The head's weight gradients stay in line on that stream (a fork
        # from an already forked stream breaks hipStreamEndCapture on ROCm 7.2); d_xnf is cleared HERE, on the main stream, because the
        # CLIP head writes its cls rows into it while the head stream is still busy.
        main = torch.cuda.current_stream()
        self.trunk.d_xnf_buffer(out["ctx"]).zero_()
        if self._head_stream is None:
            self._head_stream = torch.cuda.Stream()
        self._head_stream.wait_stream(main)
        with torch.cuda.stream(self._head_stream), OVERLAP.lane(2):
            was, OVERLAP.enabled = OVERLAP.enabled, False
            try:
                for ev in self._ssl_tail(out, P, zero_dxnf=False):
                    if callable(ev):
                        raise RuntimeError("head stream: the SSL tail asked for a collective")
                    self._head_keys += ev
            finally:
                OVERLAP.enabled = was
        return out

    def _ssl_tail(self, out, P, zero_dxnf: bool = True):
        """teacher targets, DINO + iBOT loss, head backward, scatter of the head's input gradient into the trunk's d_xnf rows (the
        part of the SSL leg behind the forward passes); yields the collectives of the centring / Sinkhorn and the head's bucket key"""
        model, st, head = self.model, self.store, self.ssl_head
        dist = self.bucketer.dist
        K, D = head.K, self.trunk.D
        Tt, Ts, Tm, B2, nl = out["Tt"], out["Ts"], out["Tm"], out["B2"], out["nl"]
        ws = out["ws"]
        t_logits, s_logits = out["teacher_logits"], out["student_logits"]
        probs = ws.get("probs", (Tt, K), BF)
        if self.centering == "sinkhorn_knopp":
            yield from self._sinkhorn_targets(ws, t_logits, probs, P, B2, Tm, K)
        else:
            inv_tt = self.hyper[8:9]  # 1 / teacher_temp of THIS step (device memory: the usual warm-up schedule replays correctly)
            ops.softmax_center(t_logits, self.center_dino, inv_tt, probs, B2, K)
            ops.softmax_center(t_logits[B2:], self.center_ibot, inv_tt, probs[B2:], Tm, K)
            # centre statistics of this batch (teacher outputs), summed over ranks, then EMA
            stats = self.center_stats
            stats.zero_()
            ops.colsum_bf16(t_logits, K, stats, B2, K)
            # masked-patch rows: the first n_masked of the Tm padded rows, n_masked read from device memory (graph-replay safe)
            ops.colsum_bf16_rows(t_logits[B2:], K, stats[K:], P["dev"]["n_masked_i"], Tm, K)
            stats[2 * K:2 * K + 1].copy_(P["dev"]["n_masked_f"])

            def apply_centers():
                ops.center_ema(self.center_dino, stats, 1.0 / (B2 * self.world), self.center_momentum, K)
                ops.center_ema(self.center_ibot, stats[K:], 0.0, self.center_momentum, K, count=stats[2 * K:])
            if self.collectives:
                # the centres are next needed by the NEXT step's teacher softmax: the all-reduce is launched asynchronously on RCCL's
                # stream, waited for together with the gradient buckets, and the EMA runs in the optimizer leg -- off the critical path
                yield lambda: self.bucketer.works.append((dist.all_reduce(stats, group=self.group, async_op=True), None))
                self._deferred.append(apply_centers)
            else:
                apply_centers()
        d_logits = ws.get("d_logits", (Ts, K), BF)
        ops.dino_ce(s_logits, probs, P["dev"]["t0"], P["dev"]["t1"], P["dev"]["w"], 1.0 / self.student_temp, self.ssl_loss_sum,
                    d_logits, Ts, K)
        dX = head.backward(d_logits, out["head_ctx"])
        if self.koleo_weight > 0:  # KoLeo on the student's global cls tokens = rows [nl, nl + B2) of the head input, per view
            self._koleo(ws, out["Hs"], dX, nl, B2, head.Din)
        yield ["dino_head"]
        from .vtp import ssl_head_input_bwd
        dX = ssl_head_input_bwd(model, out, dX)  # (through the bottleneck when the heads read the latents)
        ctx = out["ctx"]
        d_xnf = self.trunk.d_xnf_buffer(ctx)
        if zero_dxnf:
            d_xnf.zero_()
        if out["tail"] is not None:
            # tail rows: d_xnf holds the lead items' rows and then the head's own, in the head's order -- a copy (padding rows: zeros)
            ops.gather_token_rows(dX, P["dev"]["student_tail_keep"], d_xnf[out["tail"]:], Ts, D)
            return
        seg_g, seg_l = ctx.segs[-2], ctx.segs[-1]
        ops.scatter_token_rows(dX, P["dev"]["student_local_src"], d_xnf[seg_l.row0:], nl, D)
        ops.scatter_token_rows(dX[nl:], P["dev"]["student_global_src"], d_xnf[seg_g.row0:], Ts - nl, D)

    def _sinkhorn_targets(self, ws, t_logits, probs, P, B2, Tm, K):
        """Sinkhorn-Knopp teacher targets (DINOv2 sinkhorn_knopp_teacher) for the cls rows and for the masked-patch rows.  Under
        data parallelism the per-prototype sums, the running maximum and the sample count are all-reduced between the phases
        (the normalisation runs over the GLOBAL batch), exactly where DINOv2 calls dist.all_reduce."""
        dist = self.bucketer.dist
        it = self.sk_iterations
        inv_t = 1.0 / self.teacher_temp
        for tag, lg, pr, T, cnt_dev, rows_dev, count in (("cls", t_logits, probs, B2, None, None, float(B2 * self.world)),
                                                         ("patch", t_logits[B2:], probs[B2:], Tm, P["dev"]["n_masked_f"],
                                                          P["dev"]["n_masked_i"], 0.0)):
            u, v = ws.get(f"sk.u.{tag}", (T,), F32), ws.get(f"sk.v.{tag}", (K,), F32)
            scr = ws.get(f"sk.s.{tag}", (8 + K + T,), F32)
            if not self.collectives:
                ops.sinkhorn_knopp(lg, inv_t, pr, u, v, scr, T, K, count, it, -1, cnt_dev, rows_dev)
                continue
            if cnt_dev is not None:  # global masked-token count
                gcnt = ws.get("sk.cnt", (1,), F32)
                gcnt.copy_(cnt_dev)
                yield lambda gcnt=gcnt: dist.all_reduce(gcnt, group=self.group)
                cnt_dev = gcnt
            ops.sinkhorn_knopp(lg, inv_t, pr, u, v, scr, T, K, count, 0, 0, cnt_dev, rows_dev)
            yield lambda scr=scr: dist.all_reduce(scr[:1], op=dist.ReduceOp.MAX, group=self.group)
            for i in range(it):
                ops.sinkhorn_knopp(lg, inv_t, pr, u, v, scr, T, K, count, i, 1, cnt_dev, rows_dev)
                yield lambda scr=scr: dist.all_reduce(scr[8:8 + K], group=self.group)
                ops.sinkhorn_knopp(lg, inv_t, pr, u, v, scr, T, K, count, i, 2, cnt_dev, rows_dev)
            ops.sinkhorn_knopp(lg, inv_t, pr, u, v, scr, T, K, count, it, 3, cnt_dev, rows_dev)

    def _koleo(self, ws, Xs, dX, nl, B2, D):
        """koleo_weight * sum over the two views of KoLeoLoss(student global cls tokens): adds its gradient to the head-input
        gradient rows of those tokens (dX bf16) -- the tokens are the final-norm trunk outputs, so it flows on into the trunk."""
        B = B2 // 2
        self.koleo_loss_sum.zero_()
        x32 = ws.get("kl.x", (B2, D), F32)
        x32.copy_(Xs[nl:nl + B2])
        xn, inv = ws.get("kl.xn", (B2, D), F32), ws.get("kl.inv", (B2,), F32)
        ops.l2norm_fwd(x32, xn, inv, B2, D, 1e-8)
        d_xn = ws.get("kl.dxn", (B2, D), F32)
        d_xn.zero_()
        nn = ws.get("kl.nn", (B2,), torch.int32)
        for v in range(2):
            ops.koleo(xn[v * B:], nn[v * B:], d_xn[v * B:], self.koleo_loss_sum, B, D, self.koleo_weight / B)
        dx = ws.get("kl.dx", (B2, D), F32)
        ops.l2norm_bwd(d_xn, xn, inv, dx, B2, D)
        dxb = ws.get("kl.dxb", (B2, D), BF)
        dxb.copy_(dx)
        dX[nl:nl + B2].add_(dxb)

    def prepare_ssl(self, global_crops: torch.Tensor, local_crops: torch.Tensor, masks, pad_to: Optional[int] = None,
                    upperbound: Optional[int] = None) -> dict:
        """Host-side preparation of one SSL batch (index plan + small H2D copies of the index tensors; no device sync).
        global_crops f32 [2B,3,R,R] (view-major), local_crops f32 [n_local*B,3,r,r], masks bool [2B, (R/16)^2].
        The masked-token buffers are padded to a multiple of `pad_to` rows (default self.ssl_bucket = 512; the reference pads
        to the collate's fixed `upperbound`, vtp.py:432-439 -- pass upperbound=ssl_dict["upperbound"] for exactly that): the
        step's hipGraph is keyed by the padded size only, the true count travels in device memory."""
        from .ssl_engine import build_ssl_indices
        from .vtp import plan_to_device
        import numpy as np
        B = global_crops.shape[0] // 2
        hw = (global_crops.shape[-2] // 16) * (global_crops.shape[-1] // 16)
        hw_l = (local_crops.shape[-2] // 16) * (local_crops.shape[-1] // 16)
        n_local = local_crops.shape[0] // B
        m = masks.detach().cpu().numpy().astype(bool) if torch.is_tensor(masks) else np.asarray(masks, bool)
        plan = build_ssl_indices(m, B, hw, n_local, hw_l, self.dino_weight, self.ibot_weight,
                                 pad_to=int(pad_to or self.ssl_bucket), upperbound=upperbound)
        # one pinned, non-blocking upload for every per-step array (index plan + masks): the host never waits for the GPU here
        if self._stager is None:
            self._stager = HostStager(self.store.device)
        from .vtp import TAIL_KEYS
        arrays = {k: plan[k].astype(np.int32, copy=False)
                  for k in ("teacher_src", "student_local_src", "student_global_src", "t0", "t1") + TAIL_KEYS}
        arrays["w"] = plan["w"].astype(np.float32, copy=False)
        arrays["n_masked_i"] = np.array([plan["n_masked"]], np.int32)
        arrays["n_masked_f"] = np.array([float(plan["n_masked"])], np.float32)
        arrays["masks"] = m.astype(np.uint8)
        up = self._stager.upload(arrays)
        masks_dev = up.pop("masks")
        packed = up.pop("_packed")
        return dict(**{"global": global_crops, "local": local_crops}, masks=masks_dev, plan=plan, dev=up, packed=packed)

    def _step_gen(self, images: torch.Tensor, text: Optional[torch.Tensor], ssl: Optional[dict] = None, rec_images=None):
        """_step_body plus (a) the bookkeeping of which flat ranges have been handed to the gradient exchange so far (known at
        generator time, i.e. also while the body is being captured into hipGraph segments and no collective runs) and (b) the
        OPTIMIZER LANE: the update of a bucket is enqueued on a side stream `lag` bucket events after the event that announced it
        -- lag 1 without collectives (the gradients are final at the announcement), lag 2 with them (the driver launches the
        all-reduce of event k at event k and waits for it at event k + 1, when it has had a whole segment of backward to complete:
        `_handle`).  The side stream is forked from the main stream right behind an event and joined in front of the next one (a
        yield ends a hipGraph segment: nothing forked may be left open there); what is still queued after the last event runs on
        the main stream in the optimizer leg of the body."""
        self._reduced_ranges = []
        self._head_keys = []
        self._opt_queue, self._opt_done, self._hooks_done = [], [], set()
        self._clip_cursor, self._clip_keys = 0, []
        del OVERLAP._deferred[:]  # (an aborted step must not leave an issue queued)
        del self.trunk.bott_wgrads[:]  # (nor a queued bottleneck weight gradient)
        self._opt_ema = ssl is not None
        lag = 2 if self.collectives else 1
        # the lane is joined in front of every event when an event ends a graph segment / launches a collective; with one graph per
        # step (or eager launches without collectives) only in front of the optimizer leg
        lazy_join = not self.collectives and (self.single_graph or not self.use_graphs)
        # this step zeroes the flat gradient buffer and runs every tower's backward exactly once before the optimizer reads it: the
        # grouped weight-gradient launches may write dW instead of adding to it (engine.Stack.wgrad_overwrite; VTP_WGRAD_OVERWRITE=0: off)
        stacks = [e.stack for e in (self.trunk, self.decoder, getattr(self, "text", None)) if e is not None and hasattr(e, "stack")]
        if os.environ.get("VTP_WGRAD_OVERWRITE", "1") not in ("0", "false", "off"):
            for sk in stacks:
                sk.wgrad_overwrite = True
        try:
            for ev in self._step_body(images, text, ssl, rec_images):
                if not lazy_join or callable(ev) or "FINAL" in ev:
                    self._opt_join()
                if callable(ev):
                    yield ev
                    continue
                keys = [k for k in ev if k != "FINAL"]
                self._reduced_ranges += merge_ranges([r for k in keys for r in self._bucket_plan[k]])
                yield ev
                if self.overlap_opt and "FINAL" not in ev:
                    self._opt_queue.append(keys)
                    while len(self._opt_queue) >= lag:
                        self._opt_launch(self._opt_queue.pop(0))
                elif self.overlap_opt:
                    self._opt_queue.append(keys)  # the last buckets: updated by the body's optimizer leg, on the main stream
        finally:
            for sk in stacks:
                sk.wgrad_overwrite = False  # (the autograd boundary shares these engines and must accumulate)

    # ---- optimizer lane -----------------------------------------------------------------------------------------------------
    def _opt_plan(self, keys, ema: bool):
        """static plan of one bucket update: [(lo, hi, teacher_lo | None)] pieces of the flat buffers (a piece lies inside one
        EMA-tracked parameter group or outside all of them) and the runs of the weight-refresh table that hold the bucket's layers
        (student and, with `ema`, the teacher's copies of them)"""
        ck = (tuple(keys), ema)
        plan = self._opt_plans.get(ck)
        if plan is None:
            st = self.store
            rs = merge_ranges([r for k in keys for r in self._bucket_plan[k]])
            pairs = []
            if ema:
                from .vtp import _range
                for t_pref, s_pref in self.model.ema_pairs():
                    (tlo, thi), (slo, shi) = _range(st, t_pref), _range(st, s_pref)
                    assert thi - tlo == shi - slo
                    pairs.append((tlo, slo, shi))
            pieces = lane_pieces(rs, pairs)
            runs = st.desc_runs(rs) + st.desc_runs([(tl, tl + b - a) for a, b, tl in pieces if tl is not None])
            plan = self._opt_plans[ck] = (pieces, runs)
        return plan

    def _opt_update(self, keys):
        """fused AdamW (+ EMA teacher) over the bucket's ranges and the refresh of its bf16 weight copies, on the current stream"""
        st = self.store
        pieces, runs = self._opt_plan(keys, self._opt_ema)
        tab = self.group_tab
        for a, b, tl in pieces:
            teacher = None if tl is None else st.flat_p[tl:tl + b - a]
            if self._skip:
                idx4 = self._group4 if tab is not None else self.nodecay4
                ops.adamw_ema_dev_guarded(st.flat_p[a:b], st.flat_g[a:b], self.m[a:b], self.v[a:b], teacher, b - a, self.hyper,
                                          self.step_skipped, None if idx4 is None else idx4[a // 4:b // 4], tab,
                                          0 if tab is None else tab.shape[0])
            elif tab is not None:
                ops.adamw_ema_dev_grouped(st.flat_p[a:b], st.flat_g[a:b], self.m[a:b], self.v[a:b], teacher, b - a, self.hyper,
                                          self._group4[a // 4:b // 4], tab, tab.shape[0])
            else:
                ops.adamw_ema_dev(st.flat_p[a:b], st.flat_g[a:b], self.m[a:b], self.v[a:b], teacher,
                                  b - a, self.hyper, None if self.nodecay4 is None else self.nodecay4[a // 4:b // 4])
        # (skip_nonfinite: the refresh of the bf16 copies and the weight-norm hooks below need no guard -- on a skipped step they
        # re-derive the same bits from unchanged parameters)
        st.prep_runs(runs)
        # derived weights that depend only on what this bucket updated (the DINO heads' weight-normed last layers, student and -- through
        # the fused EMA -- teacher): re-derived here, beside the backward, not in the serial tail
        touched = [(a, b) for a, b, _ in pieces] + [(tl, tl + b - a) for a, b, tl in pieces if tl is not None]
        for hook, deps in getattr(st, "hook_deps", {}).items():
            if hook not in self._hooks_done and all(any(a <= lo and hi <= b for a, b in touched) for lo, hi in deps):
                hook()
                self._hooks_done.add(hook)
        self._opt_done += [(a, b) for a, b, _ in pieces]

    def _adamw(self, lo, hi, g):
        """AdamW over flat elements [lo, hi) (4-element aligned) with the gradient g: grouped when param_groups were given"""
        st, tab = self.store, self.group_tab
        if self._skip:
            idx4 = self._group4 if tab is not None else self.nodecay4
            ops.adamw_dev_guarded(st.flat_p[lo:hi], g, self.m[lo:hi], self.v[lo:hi], None, hi - lo, self.hyper, self.step_skipped,
                                  None if idx4 is None else idx4[lo // 4:hi // 4], tab, 0 if tab is None else tab.shape[0])
        elif tab is not None:
            ops.adamw_dev_grouped(st.flat_p[lo:hi], g, self.m[lo:hi], self.v[lo:hi], None, hi - lo, self.hyper,
                                  self._group4[lo // 4:hi // 4], tab, tab.shape[0])
        else:
            ops.adamw_dev(st.flat_p[lo:hi], g, self.m[lo:hi], self.v[lo:hi], None, hi - lo, self.hyper,
                          None if self.nodecay4 is None else self.nodecay4[lo // 4:hi // 4])

    def _opt_launch(self, keys):
        if not keys:
            return
        if self._clip:  # the bucket's update needs the global norm: the lane computes its partials, the optimizer leg updates it
            self._clip_keys.append(keys)
            plan = self._clip_plan(self._clip_views(keys))
            work = lambda: self._clip_sumsq(plan)  # noqa: E731
        else:
            work = lambda: self._opt_update(keys)  # noqa: E731
        if not OVERLAP.enabled:  # VTP_OVERLAP=0 (single-stream attribution profiles): same kernels, in line
            return work()
        main = torch.cuda.current_stream()
        if self._opt_stream is None:
            self._opt_stream = torch.cuda.Stream()
        OVERLAP.run_deferred()
        self._opt_stream.wait_stream(main)  # the lane picks up here ...

        def issue():  # ... and its kernels are issued behind the main stream's next kernel (engine.Overlap.defer: queue placement)
            with torch.cuda.stream(self._opt_stream):
                work()
        OVERLAP.defer(issue)
        self._opt_busy = True

    # ---- global gradient-norm clipping ---------------------------------------------------------------------------------------
    def _clip_views(self, keys):
        """the flat-gradient ranges of one bucket (what its AdamW reads): [(f32 view, n)]"""
        rs = self._clip_ranges.get(tuple(keys))
        if rs is None:
            rs = self._clip_ranges[tuple(keys)] = merge_ranges([r for k in keys for r in self._bucket_plan[k]])
        return [(self.store.flat_g[lo:hi], hi - lo) for lo, hi in rs]

    def _clip_plan(self, views):
        """[(f32 view, n)] -> [(view, n, slot base)]: the next slots of the partials buffer.  The launch order of a step is fixed for an
        objective set, so every step (eager, captured, replayed) and every rank lays its partials out the same way."""
        plan = []
        for g, n in views:
            plan.append((g, n, self._clip_cursor))
            self._clip_cursor += ops.sumsq_partials_count(n)
        if self._clip_cursor > self._clip_partials.numel():
            raise RuntimeError(f"gradient clipping: {self._clip_cursor} partials exceed the buffer ({self._clip_partials.numel()})")
        return plan

    def _clip_sumsq(self, plan):
        for g, n, base in plan:
            ops.sumsq_partials(g, n, self._clip_partials[base:])

    def _clip_finalize(self, partials=None, count=None):
        """grad_norm, grad_clip_coef and the clipped gradient multiplier hyper[7] from this step's partials; with skip_nonfinite
        also the step's decision, the counters and the bias corrections hyper[5:7] of the device step count.  Ranks decide alike: in
        all-reduce mode each holds the same reduced gradient, in sharded mode the all-reduced sum feeds the finalize."""
        if partials is None:
            partials, count = self._clip_partials, self._clip_cursor
        if self._skip:
            ops.grad_clip_finalize_guarded(partials, count, self.hyper, self.grad_norm, self.grad_clip_coef, self._skip_state,
                                           self._skip_betas)
        else:
            ops.grad_clip_finalize(partials, count, self.hyper, self.grad_norm, self.grad_clip_coef)

    def _ema(self, t, s, n):
        """EMA teacher update of one range (guarded with skip_nonfinite)"""
        if self._skip:
            ops.ema_dev_guarded(t, s, n, self.momentum_dev, self.step_skipped)
        else:
            ops.ema_dev(t, s, n, self.momentum_dev)

    def _clip_shards(self, recs):
        """sharded optimizer: partials over this rank's fp32 chunks, their sum all-reduced over the group (a collective event of the
        step), then the finalize over that one value"""
        views = []
        for rec in recs:
            n = rec.b - rec.a
            if n > 0:
                if rec.g32 is not rec.g_out:
                    rec.g32.copy_(rec.g_out)
                views.append((rec.g32, n))
        if views:
            self._clip_sumsq(self._clip_plan(views))
            ops.sum_partials(self._clip_partials, self._clip_cursor, self._clip_sum)
        else:  # a rank that owns no element of this step's buckets
            self._clip_sum.zero_()
        dist, total = self.bucketer.dist, self._clip_sum
        yield lambda: dist.all_reduce(total, group=self.group)
        self._clip_finalize(total, 1)

    def _opt_join(self):
        OVERLAP.run_deferred()
        if self._opt_busy:
            torch.cuda.current_stream().wait_stream(self._opt_stream)
            self._opt_busy = False

    def _zero_grads_async(self):
        """step-start zeroing of the flat gradient buffer (1.7 GB for the full VTP-B step) on a side stream, under the forward pass;
        _zero_join() sits in front of the first kernel that writes a gradient"""
        if not (self.overlap_opt and OVERLAP.enabled):
            self.store.zero_grad()
            return
        main = torch.cuda.current_stream()
        if self._zero_stream is None:
            self._zero_stream = torch.cuda.Stream()
        self._zero_stream.wait_stream(main)
        with torch.cuda.stream(self._zero_stream):
            self.store.zero_grad()
        self._zero_busy = True

    def _zero_join(self):
        if self._zero_busy:
            torch.cuda.current_stream().wait_stream(self._zero_stream)
            self._zero_busy = False

    def _separate_rec(self, images, text, rec_images) -> bool:
        """does the reconstruction objective need its own trunk item?  (another tensor than the clip objective's, or another
        stochastic-depth rate -- vtp.py:323-338 takes `image` and `reconstruction_image`, with a drop rate per objective)"""
        return text is not None and (rec_images is not None and rec_images is not images or self.clip_drop_rate != self.rec_drop_rate)

    def _step_body(self, images: torch.Tensor, text: Optional[torch.Tensor], ssl: Optional[dict] = None, rec_images=None):
        st = self.store
        dist = self.bucketer.dist
        sep = self._separate_rec(images, text, rec_images)
        rec_img = images if rec_images is None else rec_images
        leads = [images, rec_img] if sep else [rec_img]   # list items in front of the SSL crops: [clip | rec] or the shared one
        rec_seg = 1 if sep else 0
        Bc, Nc = images.shape[0], (images.shape[2] // 16) * (images.shape[3] // 16) + 1   # the clip item (= item 0)
        B, _, H, W = rec_img.shape
        h, w = H // 16, W // 16
        N = h * w + 1
        self._zero_grads_async()
        self.loss_sum.zero_()
        self.clip_loss_sum.zero_()
        self._deferred = []  # work that only has to be done by the end of the step (runs in the optimizer leg, behind every collective)
        if ssl is not None:  # one student list forward: [clip images | rec images | masked global crops | local crops]
            self.ssl_loss_sum.zero_()
            xnf_all = (yield from self._ssl_gen(ssl, lead_images=leads))["xnf"]
        else:
            xnf_all = self.trunk.forward_list([(im, None) for im in leads], train=True)
            self._zero_join()
        xnf = xnf_all[:Bc * Nc]  # rows of the clip item (item 0; the shared item when rec and clip see the same pass)
        # the text tower's GEMMs are small (M = 77 B rows): it is issued on its own stream (with its own wgrad side stream,
        # OVERLAP lane 1) so that it runs concurrently with the decoder forward / the first decoder-backward blocks
        par_text = text is not None and OVERLAP.enabled
        par_fwd = par_bwd = par_text
        main = torch.cuda.current_stream()
        if par_text:
            if self._text_stream is None:
                self._text_stream = torch.cuda.Stream()
            T = self._text_stream
        if par_fwd:
            T.wait_stream(main)
            with torch.cuda.stream(T), OVERLAP.lane(1):
                f_txt = self.text.forward(text, train=True)
        lat = self.trunk.latents(seg=rec_seg)
        t = self.decoder.forward(lat, B, h, w, train=True)
        dt = self.decoder._ctx[0].get("b.dt", (B * h * w, 768), BF)
        ops.l1_loss_fwd_bwd(t, rec_img, dt, self.loss_sum, B, h, w, self.rec_weight / (B * 3 * H * W))
        if self.perceptual_weight > 0:  # perceptual term: adds its gradient w.r.t. the decoder output into dt
            self.lpips_val = self.lpips.loss_and_grad(t, rec_img, dt, self.perceptual_weight, B, H, W)
        held = None  # bucket keys whose gradients are being produced on the text stream
        pvec = None
        if text is not None:
            d_xnf = self.trunk.d_xnf_buffer()[:Bc * Nc]  # rows of the clip item
            cw = self.clip.ws
            Dt = self.clip.Dt
            f_img = self.clip.image_features(xnf, Bc, Nc)
            img_n, inv_i = self.clip.normalize(f_img, "img")
            if par_fwd:
                main.wait_stream(T)
            else:
                f_txt = self.text.forward(text, train=True)
            txt_n, inv_t = self.clip.normalize(f_txt, "txt")
            Bg = Bc * self.world
            if self.collectives:
                img_all = cw.get("img_all", (Bg, Dt), F32)
                txt_all = cw.get("txt_all", (Bg, Dt), F32)

                def gather():
                    works = [self._all_gather_rows(img_all, img_n, async_op=True), self._all_gather_rows(txt_all, txt_n, async_op=True)]
                    for wk in works:
                        if wk is not None:
                            wk.wait()
                yield gather
            else:
                img_all, txt_all = img_n, txt_n
            d_img_l = cw.get("d_img_l", (Bc, Dt), F32)
            d_txt_l = cw.get("d_txt_l", (Bc, Dt), F32)
            d_img_all = cw.get("d_img_all", (Bg, Dt), F32)
            d_txt_all = cw.get("d_txt_all", (Bg, Dt), F32)
            scratch = cw.get("logits", (2 * Bc * Bg,), F32)
            if st.has("logit_bias"):
                # SigLIP (logit_bias present, vtp.py:185-188): every (local image, any text) pair once across the ranks; the text
                # side gets its gradient through the gathered columns only
                ops.siglip_loss(img_n, txt_all, st.p("logit_scale"), st.p("logit_bias"), Bc, Bg, Dt, self.rank * Bc, self.clip_loss_sum,
                                d_img_l, d_txt_all, st.g("logit_scale"), st.g("logit_bias"), scratch)
                d_txt_l.zero_()
                d_img_all.zero_()
            else:
                ops.clip_loss(img_n, txt_n, img_all, txt_all, st.p("logit_scale"), Bc, Bg, Dt, self.rank * Bc, self.clip_loss_sum,
                              d_img_l, d_txt_l, d_img_all, d_txt_all, st.g("logit_scale"), scratch)
            if self.collectives:
                rs_i = cw.get("rs_i", (Bc, Dt), F32)
                rs_t = cw.get("rs_t", (Bc, Dt), F32)

                def scatter():
                    works = [self._reduce_scatter_rows(rs_i, d_img_all, async_op=True), self._reduce_scatter_rows(rs_t, d_txt_all, async_op=True)]
                    for wk in works:
                        if wk is not None:
                            wk.wait()
                yield scatter
            else:
                rs_i, rs_t = d_img_all, d_txt_all
            # total feature gradient = local-loss term + the terms every rank's loss contributes to these rows
            ops.reduce_slabs(rs_i, Bc * Dt, 1, d_img_l, Bc * Dt, accumulate=True)
            ops.reduce_slabs(rs_t, Bc * Dt, 1, d_txt_l, Bc * Dt, accumulate=True)
            if self.clip_weight != 1.0:
                d_img_l.mul_(self.clip_weight)
                d_txt_l.mul_(self.clip_weight)
                st.g("logit_scale").mul_(self.clip_weight)
                if st.has("logit_bias"):
                    st.g("logit_bias").mul_(self.clip_weight)
            d_f_txt = self.clip.normalize_bwd(d_txt_l, txt_n, inv_t, "txt")
            if par_bwd:  # whole text backward on the text stream; its buckets are announced once it has been joined
                T.wait_stream(main)
                held = []
                # wgrads in-line on the text stream: a side stream forked from an already forked stream (nested fork) crashes
                # hipStreamEndCapture on ROCm 7.2, and the text stream as a whole already runs beside the main one
                with torch.cuda.stream(T), OVERLAP.lane(1):
                    was, OVERLAP.enabled = OVERLAP.enabled, False
                    try:
                        for ev in self._tower_backward("text", self.text.backward(d_f_txt), self.text.depth):
                            held += ev
                    finally:
                        OVERLAP.enabled = was
                held.append("text_head")
            else:
                yield from self._tower_backward("text", self.text.backward(d_f_txt), self.text.depth)
                yield ["text_head"]
            d_f_img = self.clip.normalize_bwd(d_img_l, img_n, inv_i, "img")
            # cls feature: writes the cls rows of the clip item in d_xnf; pooled: the per-image vector the final-norm backward adds to
            # the item's patch rows
            pvec = self.clip.image_backward(d_f_img, xnf, d_xnf, Bc, Nc)
            OVERLAP.join()
            if held is not None:
                held.append("clip_head")
            else:
                yield ["clip_head"]
        # decoder backward; while the text stream is busy the decoder's bucket events are held back (a yield ends a graph segment /
        # launches collectives, and every forked stream must be joined before that): the text backward (few-tile GEMMs, M = 77 B
        # rows) runs beside the WHOLE decoder backward (M = 256 B rows), and both towers' buckets are announced together in front
        # of the trunk backward, whose 20 ms hide their reductions / updates.  (Round 4 joined at the decoder's second event, i.e.
        # after bucket_blocks blocks: the rest of the text backward then ran alone on a mostly empty chip -- measured same-box with
        # bucket_blocks 3 -> 12: 686 -> 705 images/s, all of it from this join)
        def join_head():
            # the SSL head ran on its own stream (_ssl_gen): joined in front of the first event since its fork (an event ends a graph
            # segment) -- with a text tower that is the held event behind the decoder backward -- and at the latest here, in front of
            # the trunk backward its d_xnf rows feed
            if not self._head_keys:
                return []
            main.wait_stream(self._head_stream)
            keys, self._head_keys = self._head_keys, []
            return keys

        dec_gen = self._tower_backward("dec", self.decoder.backward(dt), self.decoder.depth)
        d_lat = None
        while True:
            try:
                ev = next(dec_gen)
            except StopIteration as stop:
                d_lat = stop.value
                break
            if held is not None:
                held += ev
                continue
            yield join_head() + ev
        keys = join_head()
        if held is not None:
            held += keys
        elif keys:
            yield keys
        if held is not None:
            main.wait_stream(T)
            yield held
        yield ["dec_head"]
        if text is None and ssl is None:
            # no head writes the cls rows of d_xnf on this step: clear what an earlier step with another objective set left there
            # (the workspace is keyed by shape, not by objectives)
            self.trunk.d_xnf_buffer().zero_()
        pool = (0, pvec) if pvec is not None else None  # (the clip item is item 0)
        yield from self._tower_backward("trunk", self.trunk.backward(d_lat, lat_seg=rec_seg, pool=pool), self.trunk.depth)
        yield ["trunk_head", "FINAL"]
        for fn in self._deferred:
            fn()
        # ---- optimizer (after every bucket has been reduced)
        ranges = merge_ranges(list(self.ranges_all if text is not None else self.ranges_rec) + (self.ranges_ssl if ssl is not None else []))
        if self.shard_optimizer:
            recs = self._shard_recs(ranges)
            if self._clip:
                yield from self._clip_shards(recs)  # (copies the bf16 chunks to fp32)
            for rec in recs:  # AdamW on this rank's chunk of every bucket (moments outside the own chunks are never touched)
                n = rec.b - rec.a
                if n > 0:
                    if rec.g32 is not rec.g_out and not self._clip:
                        rec.g32.copy_(rec.g_out)
                    self._adamw(rec.a, rec.b, rec.g32)
                    rec.p_send[:n].copy_(st.flat_p[rec.a:rec.b])
            # (skip_nonfinite: the all-gather needs no guard -- every rank took the same decision, a skipped step gathers unchanged chunks)
            yield lambda: self.bucketer.all_gather_params(st.flat_p, recs)
            for rec in recs:
                st.flat_p[rec.lo:rec.hi].copy_(rec.p_recv[:rec.hi - rec.lo])
        elif self.overlap_opt:
            # optimizer lane: most buckets were updated beside the backward; the last ones (announced with / right before FINAL) here
            queue = self._opt_queue
            if self._clip:  # the lane took the partials only: those of the last buckets, the global norm, then every bucket's update
                for keys in queue:
                    if keys:
                        self._clip_sumsq(self._clip_plan(self._clip_views(keys)))
                self._clip_finalize()
                queue = self._clip_keys + queue
            for keys in queue:
                if keys:
                    self._opt_update(keys)
            self._opt_queue = []
            if merge_ranges(self._opt_done) != list(ranges):
                raise RuntimeError(f"optimizer lane: updated ranges {merge_ranges(self._opt_done)} differ from the step's parameter ranges {list(ranges)}")
        else:
            if self._clip:
                self._clip_sumsq(self._clip_plan([(st.flat_g[lo:hi], hi - lo) for lo, hi in ranges]))
                self._clip_finalize()
            for lo, hi in ranges:
                self._adamw(lo, hi, st.flat_g[lo:hi])
        # skip_nonfinite: what follows the updates needs no guard.  The clamp, the bf16 refresh and the weight-norm hooks are
        # idempotent on unchanged parameters (logit_scale was clamped by the previous applied step, or starts below the bound).
        if text is not None:
            st.p("logit_scale").clamp_(max=math.log(100.0))  # OpenCLIP training-loop convention
        if self.overlap_opt:  # EMA and the weight refresh rode along bucket by bucket
            if ssl is not None:
                # ... for the student ranges this step UPDATED.  update_teacher (vtp.py:392-401) moves every EMA pair on every call:
                # a pair whose student got no gradient on this step (visual_proj on an SSL step without captions) still decays
                # towards it -- the serial leg below does that too
                from .vtp import _range
                done = merge_ranges(self._opt_done)
                for t_pref, s_pref in self.model.ema_pairs():
                    (tlo, thi), (slo, shi) = _range(st, t_pref), _range(st, s_pref)
                    for a, b in uncovered(slo, shi, done):
                        ta = tlo + (a - slo)
                        self._ema(st.flat_p[ta:ta + b - a], st.flat_p[a:b], b - a)
                        st.prep_runs(st.desc_runs([(ta, ta + b - a)]))
            st.mark_prepped(self._hooks_done)
            return
        if ssl is not None:  # EMA teacher (vtp.py:388-401) on the freshly updated student
            from .vtp import _range
            for t_pref, s_pref in self.model.ema_pairs():  # trunk, proj (legacy teacher_proj, vtp.py:396-398), dino_head
                (tlo, thi), (slo, shi) = _range(st, t_pref), _range(st, s_pref)
                self._ema(st.flat_p[tlo:thi], st.flat_p[slo:shi], thi - tlo)
        st.prep()

    # feature exchange: RCCL all-gather / reduce-scatter; on backends without them (gloo, used by the single-GPU
    # two-process test) the same result is formed with all_reduce
    def _native_collectives(self) -> bool:
        return self.bucketer.dist.get_backend(self.group) == "nccl"

    def _all_gather_rows(self, out: torch.Tensor, inp: torch.Tensor, async_op: bool = False):
        """async_op (RCCL only): returns the work handle; the caller waits where the data is consumed, so that independent
        collectives (image and text features) are in flight together instead of one stream-blocking call after the other"""
        dist = self.bucketer.dist
        if self._native_collectives():
            return dist.all_gather_into_tensor(out, inp, group=self.group, async_op=async_op)
        else:
            B = inp.shape[0]
            out.zero_()
            out[self.rank * B:(self.rank + 1) * B].copy_(inp)
            dist.all_reduce(out, group=self.group)

    def _reduce_scatter_rows(self, out: torch.Tensor, inp: torch.Tensor, async_op: bool = False):
        dist = self.bucketer.dist
        if self._native_collectives():
            return dist.reduce_scatter_tensor(out, inp, group=self.group, async_op=async_op)
        else:
            B = out.shape[0]
            tmp = inp.clone()
            dist.all_reduce(tmp, group=self.group)
            out.copy_(tmp[self.rank * B:(self.rank + 1) * B])

    def _shard_recs(self, opt_ranges):
        """The buckets reduce-scattered during this step; together they must cover exactly what the optimizer updates."""
        got = merge_ranges(self._reduced_ranges)
        if got != list(opt_ranges):
            raise RuntimeError(f"sharded optimizer: reduced gradient ranges {got} differ from the optimizer's ranges {list(opt_ranges)}")
        # Adam moments live on the rank that owns a chunk, and ownership follows the bucket boundaries: the layout must be the
        # same on every step (a step with another objective set would merge other buckets and hand chunks -- with stale moments --
        # to other owners)
        layout = tuple(self._reduced_ranges)
        if self._shard_layout is None:
            self._shard_layout = layout
        elif layout != self._shard_layout:
            raise RuntimeError("sharded optimizer: the gradient-bucket layout changed between steps (another set of objectives?); the "
                               "rank-sharded Adam moments are tied to the first step's layout -- use one objective set per trainer, "
                               "or shard_optimizer=False")
        return [self.bucketer._rec(lo, hi) for lo, hi in self._reduced_ranges]

    def _timed(self, fn):
        """run a point where the main stream has to wait for RCCL; with time_comm the wait is bracketed by HIP events"""
        if not self.time_comm:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self._comm_events.append((e0, e1))
        return out

    def comm_exposed_ms(self, reset: bool = True) -> float:
        """total time the main stream spent waiting for collectives since the last call (needs time_comm; synchronises)"""
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in self._comm_events)
        if reset:
            self._comm_events = []
        return ms

    def _gather_moments(self):
        """sharded mode: the Adam moments of a chunk live on its owner only -- assemble the full buffers (checkpointing)"""
        if not self.shard_optimizer or not self.bucketer.shards:
            return self.m, self.v
        full = []
        for buf in (self.m, self.v):
            out = buf.clone()
            for rec in self.bucketer.shards.values():
                n = rec.b - rec.a
                rec.p_send.zero_()
                if n > 0:
                    rec.p_send[:n].copy_(buf[rec.a:rec.b])
                self.bucketer.all_gather_params(None, [rec])
                out[rec.lo:rec.hi].copy_(rec.p_recv[:rec.hi - rec.lo])
            full.append(out)
        return full

    def _set_hyper(self):
        tab = None if self.param_groups is None else group_table(self.param_groups)  # (a bad scale raises before anything moves)
        if self._skip and (float(self.betas[0]), float(self.betas[1])) != self._skip_betas:
            raise ValueError(f"betas cannot change with skip_nonfinite=True: the bias corrections are formed on the device from the "
                             f"betas of the constructor {self._skip_betas}, got {tuple(self.betas)!r}")
        self.step_no += 1
        b1, b2 = self.betas
        vals = [self.lr, b1, b2, self.eps, self.wd, 1.0 - b1 ** self.step_no, (1.0 - b2 ** self.step_no) ** 0.5,
                1.0 / self.world, 1.0 / self.teacher_temp, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        if self.ssl_head is not None:
            vals[9] = float(self.teacher_momentum)
        if self._max_grad_norm is not None:
            vals[10] = self._max_grad_norm  # the clip finalize multiplies vals[7] by this step's coefficient, in device memory
        # a ring of pinned staging rows: the host may run several steps ahead of the GPU (graph replay), so a row is rewritten
        # only after the async copy that read it has completed (its event); no per-step allocation
        if self._hyper_ring is None:
            self._hyper_ring = (torch.zeros(8, 16, dtype=torch.float32).pin_memory(), [None] * 8)
        ring, events = self._hyper_ring
        slot = self.step_no % ring.shape[0]
        if events[slot] is not None:
            events[slot].synchronize()
        ring[slot].copy_(torch.tensor(vals, dtype=torch.float32))
        self.hyper.copy_(ring[slot], non_blocking=True)
        if tab is not None:  # the group table rides in the same slot of a ring of its own, under the same event
            if self._group_ring is None:
                self._group_ring = torch.zeros(ring.shape[0], len(tab), dtype=torch.float32).pin_memory()
            self._group_ring[slot].copy_(torch.tensor(tab, dtype=torch.float32))
            self.group_tab.view(-1).copy_(self._group_ring[slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        events[slot] = ev


    def _handle(self, ev):
        if callable(ev):
            self._timed(ev)
            return
        final = "FINAL" in ev
        lane = self.overlap_opt and self.collectives
        if lane and self._works_prev:
            # optimizer lane: the reductions launched at the PREVIOUS bucket event have had a whole segment of backward to complete;
            # the next segment updates that bucket (lag 2 of _step_gen), so the main stream takes them in now
            prev, self._works_prev = self._works_prev, []
            self._timed(lambda: self.bucketer.wait(prev))
        self._reduce([k for k in ev if k != "FINAL"])
        if final:
            self._timed(self.bucketer.wait)  # the generator's next (last) leg is the optimizer
        elif lane:
            self._works_prev, self.bucketer.works = self.bucketer.works, []

    def step(self, images: torch.Tensor, text: Optional[torch.Tensor] = None, ssl: Optional[dict] = None,
             reconstruction_image: Optional[torch.Tensor] = None):
        """One optimizer step.  images: f32 [B,3,H,W]; text: int64 [B, context_length] or None; ssl: prepare_ssl(...)
        output or None; reconstruction_image: the reconstruction objective's own input (the reference's forward takes `image` and
        `reconstruction_image`, vtp.py:323-338) -- None or the same tensor as `images`: rec and clip share one trunk item (identical
        activations when their drop rates agree); another tensor (or clip_drop_rate != rec_drop_rate): each objective gets its own
        item of the list forward, i.e. the reference's separate passes.  Objectives: rec (always) + clip (if text) + DINO/iBOT (if
        ssl; model must be vtp_amd.VTP).  Returns (rec_loss, clip_loss) as device scalar tensors (local to this rank; no host
        sync); the SSL loss is in self.ssl_loss_sum."""
        if ssl is not None and self.ssl_head is None:
            raise RuntimeError("SSL needs a vtp_amd.VTP model (DINO head + EMA teacher)")
        if text is not None and self.text is None:
            raise RuntimeError("CLIP not enabled. Set train_clip=True in config.")
        if text is not None and self._clip_unsupported:
            raise NotImplementedError(self._clip_unsupported)
        same = reconstruction_image is None or reconstruction_image is images
        images = self.model._img(images)  # shape / device / dtype / layout settled at the boundary (raw pointers below)
        rec_images = None if same else self.model._img(reconstruction_image)
        if text is not None:
            text = self.model._ids(text, check_range=False)
        B, _, H, W = (images if rec_images is None else rec_images).shape
        self._set_hyper()
        self._draw_drop_plans(images, text, ssl, rec_images)
        self._works_prev = []
        try:
            if self.use_graphs:
                self._step_graphs(images, text, ssl, rec_images)
            else:
                for ev in self._step_gen(images, text, ssl, rec_images):
                    self._handle(ev)
        finally:
            # the stochastic-depth plan belongs to THIS step: evaluation passes and the autograd path (get_intermediate_layers,
            # TrunkTokens / EncodeLatents / SSLStudent) that follow must not run on its image subsets
            self.trunk.stack.set_drop_plan(None)
            self.decoder.stack.set_drop_plan(None)
        self.model._pver = self.model._param_version()
        return self.loss_sum / float(B * 3 * H * W), self.clip_loss_sum

    def _draw_drop_plans(self, images, text, ssl, rec_images):
        """fresh image subsets for every block / branch of this step (host randperm -> static device index buffers); one rate per
        list item: [clip | rec] or the shared lead item, then the SSL crops"""
        rec_b = (images if rec_images is None else rec_images).shape[0]
        if self._separate_rec(images, text, rec_images):
            items, rates = [images.shape[0], rec_b], [self.clip_drop_rate, self.rec_drop_rate]
        else:
            items, rates = [rec_b], [self.rec_drop_rate]
        if ssl:
            items += [ssl["global"].shape[0], ssl["local"].shape[0]]
            rates += [self.ssl_drop_rate, self.ssl_drop_rate]
        for rts, eng, batches in ((rates, self.trunk, items), ([self.decoder_drop_rate], self.decoder, [rec_b])):
            if max(rts) > 0:
                plan = eng.stack.make_drop_plan([(b, 0, None) for b in batches], rts, self._drop_gen, self.world, self.rank)
                eng.stack.set_drop_plan(plan)
            else:
                eng.stack.set_drop_plan(None)

    def step_rec(self, images: torch.Tensor) -> torch.Tensor:
        return self.step(images, None)[0]

    # ---- training-state checkpoint: the model's own state_dict (student, teacher, heads) travels in the
    # reference's HF layout; this is the rest of the state a resumed run needs
    def _aug_engines(self):
        return [e for e in (getattr(self, "trunk", None), getattr(self, "decoder", None), getattr(self.model, "_t_trunk", None))
                if e is not None and hasattr(e, "rope_aug")]

    def state_dict(self) -> dict:
        """Optimizer moments (as name -> tensor, the same keys as model.state_dict()), step counter and SSL centres.
        With shard_optimizer the moments are gathered from their owners: this is a COLLECTIVE call -- every rank must make it
        (`if rank == 0: trainer.state_dict()` would hang); save from rank 0 afterwards."""
        st = self.store
        sd = {"step": self.step_no, "exp_avg": {}, "exp_avg_sq": {}}
        if self._skip:  # Adam's step count is the device counter (a sync, at checkpoint time); step_no counts attempted steps
            applied, skipped = self._skip_state[:2].tolist()
            sd["step"], sd["skipped_steps"] = int(applied), int(skipped)
        m, v = self._gather_moments()
        for name, (o, k) in st.offsets.items():
            sd["exp_avg"][name] = m[o:o + k].detach().clone().view(st.params[name].shape).cpu()
            sd["exp_avg_sq"][name] = v[o:o + k].detach().clone().view(st.params[name].shape).cpu()
        if self.ssl_head is not None:
            sd["center_dino"], sd["center_ibot"] = self.center_dino.cpu().clone(), self.center_ibot.cpu().clone()
        if self.param_groups is not None:
            sd["param_groups"] = [{k: g[k] for k in ("name", "lr_scale", "wd_scale")} for g in self.param_groups]
        aug = [e.rope_aug.get_state() for e in self._aug_engines() if e.rope_aug.active]
        if aug:  # this rank's RoPE-augmentation streams (per-rank state: saved and restored rank by rank)
            sd["rope_aug_rng"] = aug
        return sd

    def load_state_dict(self, sd: dict):
        st = self.store
        missing = [n for n in st.offsets if n not in sd["exp_avg"] or n not in sd["exp_avg_sq"]]
        if missing:
            raise KeyError(f"optimizer state lacks {len(missing)} parameters, e.g. {missing[:3]}")
        if "param_groups" in sd or self.param_groups is not None:
            # scales are restored by name; a checkpoint written without groups leaves a grouped trainer's scales as constructed
            saved = sd.get("param_groups")
            mine = [g["name"] for g in self.param_groups or []]
            if saved is not None:
                if [g["name"] for g in saved] != mine:
                    raise ValueError(f"checkpoint param groups {[g['name'] for g in saved]} differ from the trainer's {mine}")
                scales = [(_group_scale(g, "lr_scale"), _group_scale(g, "wd_scale")) for g in saved]
                for g, (ls, ws) in zip(self.param_groups, scales):
                    g["lr_scale"], g["wd_scale"] = ls, ws
        self.step_no = int(sd["step"])
        if self._skip:  # a checkpoint written without the guard: every step was applied
            skipped = int(sd.get("skipped_steps", 0))
            self._skip_state.copy_(torch.tensor([self.step_no, skipped, 0, 0], dtype=torch.int32))
            self.step_no += skipped
        for name, (o, k) in st.offsets.items():
            self.m[o:o + k].copy_(sd["exp_avg"][name].reshape(-1))
            self.v[o:o + k].copy_(sd["exp_avg_sq"][name].reshape(-1))
        if self.ssl_head is not None and "center_dino" in sd:
            self.center_dino.copy_(sd["center_dino"])
            self.center_ibot.copy_(sd["center_ibot"])
        engs = [e for e in self._aug_engines() if e.rope_aug.active]
        if "rope_aug_rng" in sd and len(sd["rope_aug_rng"]) == len(engs):
            for e, stt in zip(engs, sd["rope_aug_rng"]):
                e.rope_aug.set_state(stt)
        self.sync_replicas()

    # ---- hipGraph path: one captured graph per segment, replayed every step; collectives between segments ----------
    def _step_graphs(self, images: torch.Tensor, text: Optional[torch.Tensor], ssl: Optional[dict] = None, rec_images=None):
        skey = None
        if ssl is not None:
            pl = ssl["plan"]
            skey = (tuple(ssl["global"].shape), tuple(ssl["local"].shape), pl["Ts"])  # Ts: padded (bucketed) row count
        # host-side scalars that a captured segment bakes in (kernel arguments): a change re-captures instead of replaying stale
        # values; lr / betas / weight decay / teacher temperature / EMA momentum live in device memory and are not part of the key
        baked = (self.clip_weight, self.rec_weight, self.perceptual_weight, self.student_temp, self.koleo_weight, self.centering,
                 self.teacher_temp if self.centering == "sinkhorn_knopp" else None, self.center_momentum)
        key = (tuple(images.shape), None if text is None else tuple(text.shape), skey, None if rec_images is None else tuple(rec_images.shape),
               self.clip_drop_rate, self.ssl_drop_rate, self.rec_drop_rate, self.decoder_drop_rate, baked)
        plan = self._graphs.get(key)
        if plan is None:
            st = self.store
            static_img = images.clone()
            static_rec = None if rec_images is None else rec_images.clone()
            static_txt = None if text is None else text.clone()
            static_ssl = None
            if ssl is not None:  # static copies of every per-step SSL input (crops, masks, index tensors)
                if ssl.get("packed") is not None:
                    # prepare_ssl's arrays arrive as views of ONE packed upload: the static copies are views of one static buffer with the
                    # same layout, refreshed by one device copy per step instead of ten
                    buf, layout = ssl["packed"]
                    sbuf = buf.clone()
                    views = {k: sbuf[o:o + nb].view(_NP2TORCH[dt]).view(shp) for k, o, nb, dt, shp in layout}
                    static_ssl = dict(plan=ssl["plan"], masks=views.pop("masks"), dev=views, packed=(sbuf, layout))
                else:
                    static_ssl = dict(plan=ssl["plan"], masks=ssl["masks"].clone(), dev={k: v.clone() for k, v in ssl["dev"].items()})
                static_ssl["global"], static_ssl["local"] = ssl["global"].clone(), ssl["local"].clone()
            snap = (st.flat_p.clone(), self.m.clone(), self.v.clone())
            hyper0 = self.hyper.clone() if self._clip else None  # the clip finalize rewrites hyper[7]
            skip0 = self._skip_state.clone() if self._skip else None  # ... and, guarded, counts the warm-up as a step
            if ssl is not None:
                snap = snap + (self.center_dino.clone(), self.center_ibot.clone())
            # warm-up in eager mode on a side stream (allocates every workspace buffer, sets kernel attributes); the
            # collectives run for real so that all ranks stay in lock-step
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for ev in self._step_gen(static_img, static_txt, static_ssl, static_rec):
                    self._handle(ev)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            # the warm-up performed a real optimizer step: roll parameters and moments back
            st.flat_p.copy_(snap[0])
            self.m.copy_(snap[1])
            self.v.copy_(snap[2])
            if hyper0 is not None:
                self.hyper.copy_(hyper0)
            if skip0 is not None:
                self._skip_state.copy_(skip0)
            if ssl is not None:
                self.center_dino.copy_(snap[3])
                self.center_ibot.copy_(snap[4])
            st.prep()
            del snap
            segs = []
            pool = torch.cuda.graph_pool_handle()
            for eng in self._aug_engines():
                eng.rope_aug.touched.clear()
            gen = self._step_gen(static_img, static_txt, static_ssl, static_rec)
            done = False
            while not done:
                g = torch.cuda.CUDAGraph()
                ev = None
                # thread_local capture mode: the RCCL watchdog thread keeps querying events while this thread captures
                with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                    while True:
                        try:
                            ev = next(gen)
                        except StopIteration:
                            done = True
                            break
                        if not self.single_graph or callable(ev):
                            break  # something runs between the segments: a collective, or the reductions of a bucket
                        self._handle(ev)  # no collectives: bookkeeping only -- the capture goes on in the same graph
                        ev = None
                segs.append((g, ev))
            plan = (static_img, static_txt, static_ssl, segs, static_rec)
            self._graphs[key] = plan
            self._graph_aug[key] = [(eng, frozenset(eng.rope_aug.touched)) for eng in self._aug_engines() if eng.rope_aug.active]
        static_img, static_txt, static_ssl, segs, static_rec = plan
        # train-time RoPE augmentations: fresh draws into the static table buffers the captured segments read (an eager step
        # draws inside its forward passes; under capture nothing can be drawn)
        for eng, keys in self._graph_aug.get(key, ()):
            eng.rope_aug.refresh_all(keys)
        static_img.copy_(images)
        if rec_images is not None:
            static_rec.copy_(rec_images)
        if text is not None:
            static_txt.copy_(text)
        if ssl is not None:
            static_ssl["global"].copy_(ssl["global"])
            static_ssl["local"].copy_(ssl["local"])
            sp, pk = static_ssl.get("packed"), ssl.get("packed")
            if sp is not None and pk is not None and sp[1] == pk[1]:
                sp[0].copy_(pk[0])
            else:
                static_ssl["masks"].copy_(ssl["masks"])
                for k, v in ssl["dev"].items():
                    static_ssl["dev"][k].copy_(v)
        for g, ev in segs:
            g.replay()
            if ev is not None:
                self._handle(ev)
