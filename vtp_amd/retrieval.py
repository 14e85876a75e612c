"""Cross-modal retrieval on the CLIP heads: image -> text and text -> image recall@K on a captioned set (Flickr30k, MSCOCO-5k), the
evaluation the CLIP paper reports beside zero-shot classification, restated from the papers' description.  Neither CLIP_benchmark
nor OpenCLIP is a reference of this project, so parity with those programs is unpinned; the arithmetic is pinned by the fp64
restatement in tests/retrieval_ref.py.

    r = Retrieval(model, ks=(1, 5, 10))
    for images, image_ids, tokens, caption_image_ids in loader:          # any number of captions per image
        r.add_images(images.cuda(), image_ids.cuda())
        r.add_texts(tokens.cuda(), caption_image_ids.cuda())
    out = r.result()    # {"image_to_text": {"R@1": %, "R@5": %, "R@10": %, "counts": {k: hits}, "rows": n, "median_rank", "mean_rank"},
                        #  "text_to_image": {...}}

Features are get_clip_image_feature / get_clip_text_feature(normalize=True), cast to f32 and stored as they come.  Whether they
come from the bf16 path or from model.enable_fp32_forward() is the caller's choice: this class ranks what it is given, exactly.

Definition.  s(i, j) is the fp32 fmaf chain over the feature columns in ascending order (the bits of ops.gemm_nt_f32).  The
ground truth G(i) of a query is every gallery row with the query's image id: one image per caption, all its captions per image.
Gallery rows are ordered by (similarity descending, gallery index ascending): among equal similarities the lower index wins, the
tie rule of ZeroShot and Knn.  (s*, j*) is the first row of G(i) under that order and rank = #{s > s*} + #{j < j* : s == s*}, the
rows strictly before it.  A query whose id no gallery row carries has rank = the gallery size: a miss at every K and still a row.
R@K = #{rank < K} / rows * 100.  median_rank and mean_rank are 1-based (rank + 1), formed on the host in fp64.

result() recomputes everything from the two banks with csrc/retrieval.hip: the ground-truth lists are built on the device from
the id vectors (a stable sort and searchsorted: integer plumbing only; ids need not be sorted, contiguous or balanced),
vtp_retr_best finds (s*, j*), vtp_retr_rank sweeps the gallery in chunks and counts, vtp_retr_count forms the counters.  The
[queries, gallery] matrix is never written, no row of it is ever held, and the ranks repeat bit for bit whatever chunk_rows or
query_rows.  The host reads one integer per direction (the length of the ground-truth lists) while the lists are built, then the
counters and the ranks.

With `group`, each rank adds ITS OWN rows; result() all-gathers both banks and both id vectors (rank-major) and every rank
computes the whole result redundantly, so every rank returns what a single process fed the rank-major concatenation returns.
There is no CPU path: tensors on the CPU raise."""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .banks import BankSet, Group, Workspace, eval_device, feature_rows, spans
from .knn import neighbour_lists
from .zeroshot import percent

SIDES = ("image", "text")
DIRECTIONS = {"image_to_text": ("image", "text"), "text_to_image": ("text", "image")}  # name -> (queries, gallery)


def clip_image_feature(model, images: torch.Tensor) -> torch.Tensor:
    return model.get_clip_image_feature(images, normalize=True)


def clip_text_feature(model, tokens: torch.Tensor) -> torch.Tensor:
    return model.get_clip_text_feature(tokens, normalize=True)


def check_ks(ks: Sequence[int]) -> Tuple[int, ...]:
    ks = tuple(int(k) for k in ks)
    if not 1 <= len(ks) <= ops.RETR_MAX_KS:
        raise ValueError(f"ks must name 1 to {ops.RETR_MAX_KS} recall levels, got {len(ks)}")
    if ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks must be positive and strictly ascending, got {ks}")
    return ks


class Retrieval:
    """model: a vtp_amd.VTPModel with train_clip, or None when features are given (add_image_features / add_text_features).
    image_feature_fn(model, images) / text_feature_fn(model, tokens) -> [n, D] replace the normalised CLIP features.  capacity: rows
    to allocate per bank up front (a bank doubles when it is full).  chunk_rows / query_rows: gallery rows per vtp_retr_rank call
    and queries per pass over the gallery; results do not depend on either.  group: a process group whose ranks each add their
    own rows."""

    def __init__(self, model, ks: Sequence[int] = (1, 5, 10), group=None, capacity: Optional[int] = None, chunk_rows: int = 1 << 16,
                 query_rows: int = 4096, image_feature_fn: Optional[Callable] = None, text_feature_fn: Optional[Callable] = None,
                 device=None):
        self.ks = check_ks(ks)
        if chunk_rows < 1 or query_rows < 1 or (capacity is not None and capacity < 1):
            raise ValueError("chunk_rows, query_rows and capacity must be positive")
        self.device = eval_device("Retrieval", model, device)
        self.model, self.group = model, group
        self.feature_fn = {"image": image_feature_fn or clip_image_feature, "text": text_feature_fn or clip_text_feature}
        self.chunk_rows, self.query_rows = int(chunk_rows), int(query_rows)
        self._group = Group(group)
        self.banks = BankSet(SIDES, self.device, capacity, {"ids": torch.int64})  # rows as given, and the image id of every row
        self._ws = Workspace(self.device)
        self.reset()

    def reset(self) -> None:
        """empties both banks and forgets the last result"""
        self.banks.clear()
        self._forget()

    def _forget(self) -> None:
        self._rank: Dict[str, torch.Tensor] = {}    # direction -> int32 [queries] on the device
        self._counts: Dict[str, torch.Tensor] = {}  # direction -> int64 [nk + 1] on the device
        self._feats: Dict[str, torch.Tensor] = {}   # side -> the rows of the whole group the last result was computed from

    # ------------------------------------------------------------------------------------------------ banks
    def _features(self, side: str, inputs: torch.Tensor, image_ids: torch.Tensor) -> torch.Tensor:
        if self.model is None:
            raise RuntimeError(f"Retrieval was built without a model: use add_{side}_features")
        if not isinstance(inputs, torch.Tensor) or not inputs.is_cuda:
            raise ValueError(f"{side} inputs must live on the MI355X (got a CPU tensor): there is no CPU path")
        self._check_ids(side, image_ids, inputs.shape[0])  # before any launch
        with torch.no_grad():
            return self.feature_fn[side](self.model, inputs)

    @staticmethod
    def _check_ids(side: str, image_ids: torch.Tensor, n: int) -> None:
        if not isinstance(image_ids, torch.Tensor) or not image_ids.is_cuda:
            raise ValueError(f"the image ids of the {side} rows must live on the MI355X (got a CPU tensor): there is no CPU path")
        if image_ids.is_floating_point() or image_ids.dtype == torch.bool or image_ids.shape != (n,):
            raise ValueError(f"the image ids of the {side} rows must be {n} integers, got {image_ids.dtype} {tuple(image_ids.shape)}")

    def _add(self, side: str, feats: torch.Tensor, image_ids: torch.Tensor) -> None:
        f = feature_rows(feats, f"{side} features")
        self.banks.check_width(f.shape, f"{side} features")
        self._check_ids(side, image_ids, f.shape[0])
        rows, ids = self.banks[side].reserve(*f.shape)
        rows.copy_(f)
        ids.copy_(image_ids.detach())
        self._forget()

    def add_images(self, images: torch.Tensor, image_ids: torch.Tensor) -> None:
        """images [n, 3, H, W] and their ids [n] (integers, any values): device only"""
        self._add("image", self._features("image", images, image_ids), image_ids)

    def add_texts(self, tokens: torch.Tensor, image_ids: torch.Tensor) -> None:
        """token ids [n, context_length] and, per caption, the id [n] of the image it describes: device only"""
        self._add("text", self._features("text", tokens, image_ids), image_ids)

    def add_image_features(self, feats: torch.Tensor, image_ids: torch.Tensor) -> None:
        """appends the rows of feats [n, D] (any float type, stored as f32, not normalised here) and their ids to the image bank"""
        self._add("image", feats, image_ids)

    def add_text_features(self, feats: torch.Tensor, image_ids: torch.Tensor) -> None:
        self._add("text", feats, image_ids)

    def rows(self, side: str) -> torch.Tensor:
        """this rank's rows of a bank ("image" / "text"), f32 [size, D] (a view)"""
        if not self.banks[side].size:
            raise RuntimeError(f"the {side} bank is empty: add_{side}s / add_{side}_features first")
        return self.banks[side].rows

    def ids(self, side: str) -> torch.Tensor:
        """the image ids of this rank's rows of a bank, int64 [size] (a view)"""
        self.rows(side)
        return self.banks[side].column("ids")

    def _gathered(self) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
        """both banks and both id vectors of the whole group, rank-major (BankSet.gathered); a bank without rows raises"""
        rows, columns, totals = self.banks.gathered(self._group)
        where = " on every rank" if self._group.world > 1 else ""
        for s in SIDES:
            if not totals[s]:
                raise RuntimeError(f"the {s} bank is empty{where}: add_{s}s / add_{s}_features first")
        return rows, {s: columns[s]["ids"] for s in SIDES}

    # ------------------------------------------------------------------------------------------------ evaluation
    def ground_truth(self, query_ids: torch.Tensor, gallery_ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """the ground-truth lists as a CSR on the device: (gt_ptr int32 [B + 1], gt_idx int64 [nnz]); the list of a query holds every
        gallery row with its id, ascending.  Integer plumbing only; the host reads nnz."""
        order = torch.sort(gallery_ids, stable=True).indices
        sorted_ids = gallery_ids[order]
        lo = torch.searchsorted(sorted_ids, query_ids, right=False)
        hi = torch.searchsorted(sorted_ids, query_ids, right=True)
        ptr = torch.zeros(query_ids.shape[0] + 1, device=self.device, dtype=torch.int64)
        torch.cumsum(hi - lo, 0, out=ptr[1:])
        nnz = int(ptr[-1])
        if nnz > (1 << 31) - 65:
            raise ValueError(f"the ground-truth lists hold {nnz} entries, more than 2^31 - 65")
        e = torch.arange(nnz, device=self.device, dtype=torch.int64)
        b = torch.searchsorted(ptr[1:], e, right=True)  # the query of entry e
        return ptr.to(torch.int32), order[lo[b] + (e - ptr[b])].contiguous()

    def _direction(self, q: torch.Tensor, q_ids: torch.Tensor, x: torch.Tensor, x_ids: torch.Tensor):
        """queries q [B, D] with ids q_ids against the gallery x [N, D] with ids x_ids -> (rank int32 [B], counts int64 [nk + 1]) on
        the device"""
        B, N = q.shape[0], x.shape[0]
        gt_ptr, gt_idx = self.ground_truth(q_ids, x_ids)
        best_s = torch.empty(B, device=self.device, dtype=torch.float32)
        best_j = torch.empty(B, device=self.device, dtype=torch.int64)
        ops.retr_best(q, x, gt_ptr, gt_idx, best_s, best_j)
        rank = torch.empty(B, device=self.device, dtype=torch.int32)
        counts = torch.zeros(len(self.ks) + 1, device=self.device, dtype=torch.int64)
        beats = torch.empty(min(B, self.query_rows), device=self.device, dtype=torch.int32)
        for b0, b1 in spans(B, self.query_rows):
            pass_beats = beats[:b1 - b0].zero_()
            for n0, n1 in spans(N, self.chunk_rows):
                ops.retr_rank(q[b0:b1], x[n0:n1], n0, best_s[b0:b1], best_j[b0:b1], pass_beats)
            ops.retr_count(pass_beats, self.ks, counts, rank, b0)
        return rank, counts

    def _compute(self) -> None:
        feats, ids = self._gathered()
        if feats["image"].shape[1] != feats["text"].shape[1]:
            raise ValueError(f"image and text features differ in width: {feats['image'].shape[1]} and {feats['text'].shape[1]}")
        for s in SIDES:
            if feats[s].shape[0] >= (1 << 31) - 1:
                raise ValueError(f"the {s} bank holds {feats[s].shape[0]} rows, more than a rank (int32) can count")
        self._feats = feats
        for name, (qs, xs) in DIRECTIONS.items():
            self._rank[name], self._counts[name] = self._direction(feats[qs], ids[qs], feats[xs], ids[xs])

    def result(self) -> Dict[str, Dict]:
        """per direction ("image_to_text", "text_to_image"): "R@k" in percent for every k of ks, "counts" {k: queries with rank < k},
        "rows", "median_rank" and "mean_rank" (1-based, fp64 on the host).  Recomputed from the banks on every call, so rows may be
        added afterwards."""
        self._compute()
        out = {}
        for name in DIRECTIONS:
            c = self._counts[name].cpu()
            rows = int(c[-1])
            r = self._rank[name].cpu().to(torch.float64) + 1
            mid = r.sort().values[(rows - 1) // 2:rows // 2 + 1]  # the middle element, or the two around the middle
            d = {f"R@{k}": percent(int(c[m]), rows) for m, k in enumerate(self.ks)}
            d["counts"] = {k: int(c[m]) for m, k in enumerate(self.ks)}
            d["rows"] = rows
            d["median_rank"] = float(mid.mean())
            d["mean_rank"] = float(r.mean())
            out[name] = d
        return out

    def ranks(self, direction: str) -> torch.Tensor:
        """int32 [queries] on the device: per query of the direction the number of gallery rows before its best ground-truth row
        (0 = retrieved first; the gallery size for a query without ground truth); valid after result()"""
        if direction not in DIRECTIONS:
            raise ValueError(f"direction must be one of {tuple(DIRECTIONS)}, got {direction!r}")
        if direction not in self._rank:
            raise RuntimeError("ranks() is valid after result()")
        return self._rank[direction]

    def top(self, direction: str, k: int) -> torch.Tensor:
        """int64 [queries, k] on the device: the first k gallery rows of every query under (similarity descending, index ascending),
        through ops.knn_topk; valid after result() (it ranks the rows the last result was computed from)"""
        if direction not in DIRECTIONS:
            raise ValueError(f"direction must be one of {tuple(DIRECTIONS)}, got {direction!r}")
        if direction not in self._rank:
            raise RuntimeError("top() is valid after result()")
        qs, xs = DIRECTIONS[direction]
        q, x = self._feats[qs], self._feats[xs]
        B, N = q.shape[0], x.shape[0]
        if not 1 <= int(k) <= min(ops.KNN_MAX_K, N):
            raise ValueError(f"k must be 1 .. {min(ops.KNN_MAX_K, N)}, got {k}")
        k = int(k)
        sims = torch.full((B, k), float("-inf"), device=self.device, dtype=torch.float32)
        idx = torch.full((B, k), -1, device=self.device, dtype=torch.int64)
        neighbour_lists(q, x, k, self._ws, min(self.query_rows, 1024), self.chunk_rows, 0, sims, idx)
        return idx
