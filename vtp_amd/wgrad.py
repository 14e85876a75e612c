"""Host side of the weight gradients of a transformer block: the problem records, the rules that cut a grouped launch
(vtp_gemm_tn_grouped / _limit / _items) into tiles and K slices, and the planner that turns the problems linear_bwd recorded for a
block into one launchable object.  vtp_amd.ops re-exports the public names."""
import os
from collections import namedtuple

import torch

from . import _lib

# One problem of a grouped launch, field for field the GroupProblem of csrc/gemm_group.h (16 x int64 in the device table; the only place
# in Python that knows the layout).  C[M, N] (+)= A[K, M]^T B[K, N]: for dW = dy^T x that is A = dy, B = x, M / N = the layer's output /
# input features, K = the problem's token rows (0: the launch's); colsum: f32 [M] += A's column sums (the bias gradient), 0: none
GroupRecord = namedtuple("GroupRecord", "A B C colsum lda ldb ldc M N c_grp c_pre tile0 accumulate K pad0 pad1", defaults=(0, 0))
# What linear_bwd records for the grouped launch of its block: gw[N * K] (+)= dy^T x, gb[N] += colsum(dy), over Ktok token rows
Problem = namedtuple("Problem", "dy x gw gb N K swiglu_h Ktok")


def _p(t):
    return 0 if t is None else t.data_ptr()


def wgrad_group_fits(Ktok: int, max_ld: int) -> bool:
    """the grouped launch stages its operands with 32-bit byte offsets (k row x leading dimension x 2 B): rows x widest leading
    dimension must stay below 4 GiB -- otherwise the caller takes the per-layer path, which has the ring-kernel fallback"""
    return int(Ktok) * int(max_ld) * 2 < (1 << 32)


def gemm_cus() -> int:
    """workgroup slots the one-workgroup-per-CU GEMM launches may use: 256, or VTP_GEMM_CUS (the library's persistent kernels read the
    same variable) when CUs are to be left to a long-running communication kernel (INTEGRATION.md "Running beside RCCL")"""
    try:
        v = int(os.environ.get("VTP_GEMM_CUS", "0") or 0)
    except ValueError:
        v = 0
    return v - v % 8 if 8 <= v < 256 else 256


def wgrad_group_splits(ntiles: int, Ktok: int):
    """split rule of a grouped launch: tiles x splits fills one round of the CUs (256, or VTP_GEMM_CUS), every K slice keeps >= 16
    k-tiles; returns (k rows per slice, effective slice count) -- the launcher (vtp_gemm_tn_grouped) rounds the same way"""
    s = max(1, min(gemm_cus() // ntiles, Ktok // 1024))
    ks = ((Ktok + s - 1) // s + 63) // 64 * 64
    return ks, (Ktok + ks - 1) // ks


def wgrad_group_kernel(ntiles: int, splits: int, Ktok: int) -> int:
    """which kernel runs a grouped weight-gradient launch: 0 = the 8-phase kernel; 1 = the one-wave-per-SIMD kernel (gemm4w_tn.hip) on the
    same tiles (cut by wgrad_group_items), when the token count allows its 8-row staging pieces and a K slice is long enough to amortise its
    pipeline fill.  VTP_GEMM4W_TN=0 / 1 forces the choice (same-box A/B of the step); a token count that is not a multiple of 8
    always takes the 8-phase kernel."""
    e = os.environ.get("VTP_GEMM4W_TN")
    if Ktok % 8 != 0 or e == "0":
        return 0
    return int(e == "1" or Ktok // max(splits, 1) >= W4_TN_MIN_SLICE)


def wgrad_k_cuts(Ktok: int, n: int):
    """[(kbeg, kcount)] of a K range cut into n slices of whole k-tiles (64 rows): fewer than n when the rounding leaves none for the last"""
    ks = ((Ktok + n - 1) // n + 63) // 64 * 64
    return [(b, min(Ktok, b + ks) - b) for b in range(0, Ktok, ks)]


def wgrad_group_items(rows, Ktok: int, base_splits: int, cus: int = None):
    """work-item list of a grouped launch on the one-wave-per-SIMD kernel (vtp_gemm_tn_grouped_items).  rows: the GroupProblem records
    (WgradGroup.rows, or any 16-long sequences in that order).  Every tile is cut into `base_splits` K ranges, except the tiles that also
    form a bias gradient -- the first tile column of a problem with a colsum target: their k loop carries 64 v_dot2 per k-tile beside
    its 64 MFMAs and measures 27 % slower (tools/wgrad_timeline.py: 470 vs 365 us at 34 144 rows) -- which get ONE MORE slice when the
    launch still fits one round of the CUs and the shorter slice keeps >= 16 k-tiles.  Returns (items [n, 8] int32 rows {tile, kbeg, kcount, nparts, part, 0, 0, 0}, slots).
    Order: per problem, the heavier-cut tiles first, slice-major inside a group -- the kernel deals contiguous chunks of the list to
    the XCDs, so the workgroups that stream the same K range of the same operand panels sit behind one L2."""
    cus = gemm_cus() if cus is None else cus
    rows = [GroupRecord._make(r) for r in rows]
    tiles = []  # (tile index, problem, has colsum work)
    for pi, r in enumerate(rows):
        tn = (r.N + 255) // 256  # the C of a problem is dW [r.M, r.N]: r.M rows from dy's columns, r.N columns from x's
        for lt in range(((r.M + 255) // 256) * tn):
            tiles.append((r.tile0 + lt, pi, r.colsum != 0 and lt % tn == 0))
    ncs = sum(1 for t in tiles if t[2])
    # token rows per problem (0 = Ktok).  Problems over different row counts (the last trunk block: qkv over every row,
    # proj / w12 / w3 over the tail rows) are cut per problem, so that the workgroup counts follow the work (wgrad_mixed_splits)
    Ks = [int(r.K) or int(Ktok) for r in rows]
    if len(set(Ks)) > 1:
        per = wgrad_mixed_splits([sum(1 for t in tiles if t[1] == pi) for pi in range(len(rows))], Ks, cus)
    else:
        per = [base_splits] * len(rows)
    n_items = sum(per[t[1]] for t in tiles)
    items, slots = [], 1
    for pi in range(len(rows)):
        more = ncs > 0 and n_items + ncs <= cus and Ks[pi] // (per[pi] + 1) >= 1024
        for heavy in (True, False):
            grp = [t for t in tiles if t[1] == pi and t[2] == heavy]
            if not grp:
                continue
            cs = wgrad_k_cuts(Ks[pi], per[pi] + 1 if (heavy and more) else per[pi])
            slots = max(slots, len(cs))
            for z, (kb, kc) in enumerate(cs):
                items += [[t[0], kb, kc, len(cs), z, 0, 0, 0] for t in grp]
    return items, slots


def wgrad_mixed_splits(ntiles, Ks, cus: int):
    """K slices per tile for each problem of a grouped launch whose problems have DIFFERENT token counts Ks (ntiles: their tile counts).
    One round of the CUs runs every workgroup at once, so the launch lasts as long as its longest K slice: starting from one slice per
    tile, the problems that share the longest slice are cut once more, as long as the launch still fits `cus` workgroups and every
    slice keeps >= 16 k-tiles."""
    n = len(Ks)
    per = [1] * n
    length = lambda p: ((Ks[p] + per[p] - 1) // per[p] + 63) // 64 * 64
    while True:
        top = max(length(p) for p in range(n))
        grp = [p for p in range(n) if length(p) == top]
        total = sum(per[p] * ntiles[p] for p in range(n))
        if total + sum(ntiles[p] for p in grp) > cus or any(Ks[p] // (per[p] + 1) < 1024 for p in grp):
            return per
        for p in grp:
            per[p] += 1


def wgrad_group_mixed_ok(Ks) -> bool:
    """may problems over the token counts Ks share ONE grouped launch?  Only the item-list kernel cuts each problem's own K range: the
    counts must allow its 8-row staging pieces and the kernel must be the measured choice for every one of them (wgrad_group_kernel);
    otherwise the caller launches one group per token count"""
    return all(wgrad_group_kernel(0, 1, k) == 1 for k in Ks)  # (one slice: each count against the kernel's shortest useful slice)


def wgrad_group_uniform_items(ntiles: int, Ktok: int, splits: int):
    """the uniform tiles x slices cut (the geometry of the 8-phase kernel's grouped launch) as a work-item list: every tile in `splits`
    K ranges, slice-major over all tiles (items[z * ntiles + tile]), so a workgroup gets the tile and slice that grid would give it.
    Returns (items, slots) like wgrad_group_items."""
    cs = wgrad_k_cuts(Ktok, max(int(splits), 1))
    return [[t, kb, kc, len(cs), z, 0, 0, 0] for z, (kb, kc) in enumerate(cs) for t in range(ntiles)], len(cs)


W4_TN_MIN_SLICE = 4096  # token rows per K slice from which the one-wave-per-SIMD kernel is taken (tools/wgrad_kernel_ab.py against the two-phase 8-phase kernel: x0.97 at 1232 .. 2048 rows, x1.01 at 4096, x1.06 at 8224, x1.08 .. 1.12 at 17072)


class WgradGroup:
    """The weight gradients of one transformer block as ONE launch (vtp_gemm_tn_grouped): problems dW_g[N_g, K_g] (+)= dy_g^T x_g
    over the same token rows.  add() the problems, finalize() once (the operand buffers are static: the device descriptor table
    is built a single time), launch() every step."""

    def __init__(self, Ktok: int, k_rows=None):
        """k_rows (int32 [1] on the device): the problems sum over the token rows [0, min(Ktok, k_rows[0])) only and read no row beyond
        them (vtp_gemm_tn_grouped_limit: the 8-phase kernel, one K slice per tile)"""
        self.k_rows = k_rows
        self.Ktok, self.rows, self.ntiles, self.keep = int(Ktok), [], 0, []
        self.table = self.part = self.ticket = None
        self._uniform = {}  # splits -> (items, nitems, slots): uniform lists of a forced launch(kernel=1)

    def add(self, dy, x, gw, gb, N: int, K: int, swiglu_h: int = 0, accumulate: bool = True, Ktok: int = None):
        """dy bf16 [Ktok, N] (row stride dy.stride(0)), x bf16 [Ktok, K], gw f32 [N * K], gb f32 [N] or None (bias gradient =
        column sums of dy, fused).  swiglu_h: dy's columns are the 8|8-interleaved w1|w2 pre-activation gradients; the rows of gw
        (and gb) are w1's H rows followed by w2's.  Ktok: token rows of THIS problem when they differ from the group's (item-list
        kernel only: finalize() refuses a mixed group it cannot run there)."""
        # limits of BOTH grouped kernels (16-B staging pieces, clamped tail columns): checked here because the kernels read the records
        # from device memory and cannot refuse them -- e.g. ffn_layer="mlp" with an odd int(D * ratio) takes the per-layer path
        if N % 8 or K % 8 or dy.stride(0) % 8 or x.stride(0) % 8 or N < 8 or K < 8:
            raise ValueError(f"WgradGroup.add: N = {N}, K = {K} and the leading dimensions ({dy.stride(0)}, {x.stride(0)}) must be multiples "
                             "of 8 (use the per-layer weight-gradient path: linear_bwd without `defer`)")
        self.rows.append(GroupRecord(A=dy.data_ptr(), B=x.data_ptr(), C=gw.data_ptr(), colsum=_p(gb), lda=dy.stride(0), ldb=x.stride(0),
                                     ldc=K, M=N, N=K, c_grp=-1 if swiglu_h else 0, c_pre=swiglu_h, tile0=self.ntiles,
                                     accumulate=int(accumulate), K=0 if Ktok is None or int(Ktok) == self.Ktok else int(Ktok)))
        self.ntiles += ((N + 255) // 256) * ((K + 255) // 256)
        self.keep += [dy, x, gw, gb]

    def finalize(self, device, scratch=None):
        """split factor: tiles x splits fills one round of the 256 CUs, every K slice keeps >= 16 k-tiles.  scratch: a dict shared by
        the groups that never run concurrently (one partial-sum / ticket buffer for all of them)."""
        assert 1 <= len(self.rows) <= 8
        rows = self.rows = [GroupRecord._make(r) for r in self.rows]
        Ks = [r.K or self.Ktok for r in rows]
        self.mixed = len(set(Ks)) > 1
        if not self.mixed and Ks[0] != self.Ktok:  # one count after all: it is the group's (the uniform-grid kernel reads only that)
            self.Ktok = Ks[0]
            rows = self.rows = [r._replace(K=0) for r in rows]
        if self.mixed and any(k % 8 or k < 8 for k in Ks):
            raise ValueError(f"WgradGroup: problems over different token counts {Ks} need multiples of 8 (the item-list kernel); "
                             "launch one group per token count")
        if not all(wgrad_group_fits(k, max(r.lda, r.ldb)) for k, r in zip(Ks, rows)):
            raise ValueError("WgradGroup: token rows x leading dimension exceed the 32-bit staging offsets of vtp_gemm_tn_grouped; "
                             "use the per-layer weight-gradient path (linear_bwd without `defer`)")
        _, self.splits = wgrad_group_splits(self.ntiles, self.Ktok)
        self.table = torch.tensor(rows, dtype=torch.int64, device=device)
        if self.k_rows is not None:  # a device token count: one slice (a slice may turn out empty, and nobody may wait on its ticket)
            if self.mixed:
                raise ValueError("WgradGroup: a device token count takes one static token count for every problem")
            self.splits, self.kernel, self.items, self.nitems, self.slots = 1, 0, None, None, 1
            return self
        self.kernel = 1 if self.mixed else wgrad_group_kernel(self.ntiles, self.splits, self.Ktok)
        self.items, self.nitems, self.slots = None, None, self.splits
        if self.kernel == 1:  # uneven cut: the tiles with bias-gradient work get one slice more (wgrad_group_items)
            items, self.slots = wgrad_group_items(rows, self.Ktok, self.splits)
            self.nitems = len(items)
            self.items = torch.tensor(items, dtype=torch.int32, device=device)
        if self.slots > 1:
            scratch = {} if scratch is None else scratch
            need = self.ntiles * self.slots * 65536
            if scratch.get("part") is None or scratch["part"].numel() < need:
                scratch["part"] = torch.empty(need, dtype=torch.float32, device=device)
            if scratch.get("ticket") is None or scratch["ticket"].numel() < self.ntiles:
                scratch["ticket"] = torch.zeros(max(self.ntiles, 256), dtype=torch.int32, device=device)
            self.part, self.ticket = scratch["part"], scratch["ticket"]
        return self

    def launch(self, kernel=None):
        """kernel: 0 = the 8-phase kernel on the uniform tiles x self.splits grid, 1 = the one-wave-per-SIMD kernel (gemm4w_tn.hip) on the
        work-item list of finalize() -- or, forced on a group for which finalize() built none (tools, tests), on the uniform cut of the
        current self.splits written as a list -- None = the measured choice made by finalize() (wgrad_group_kernel)"""
        lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
        kernel = self.kernel if kernel is None else kernel
        if self.k_rows is not None:
            if kernel != 0:
                raise ValueError("WgradGroup.launch: a device token count runs on the 8-phase kernel only")
            _lib.check(lib.vtp_gemm_tn_grouped_limit(_p(self.table), len(self.rows), self.ntiles, self.Ktok, _p(self.k_rows), s),
                       "vtp_gemm_tn_grouped_limit")
            return
        if kernel == 0 and self.mixed:
            raise ValueError("WgradGroup.launch: the 8-phase kernel takes one token count for every problem")
        if kernel == 0:
            _lib.check(lib.vtp_gemm_tn_grouped(_p(self.table), len(self.rows), self.ntiles, self.Ktok, self.splits, _p(self.part),
                                               _p(self.ticket), s), "vtp_gemm_tn_grouped")
            return
        if kernel != 1:
            raise ValueError(f"WgradGroup.launch: kernel must be 0, 1 or None, not {kernel!r}")
        items, nitems, slots = self.items, self.nitems, self.slots
        if items is None:
            if self.splits not in self._uniform:
                rows, slots = wgrad_group_uniform_items(self.ntiles, self.Ktok, self.splits)
                self._uniform[self.splits] = (torch.tensor(rows, dtype=torch.int32, device=self.table.device), len(rows), slots)
            items, nitems, slots = self._uniform[self.splits]
        _lib.check(lib.vtp_gemm_tn_grouped_items(_p(self.table), len(self.rows), self.ntiles, self.Ktok, _p(items), nitems, slots,
                                                 _p(self.part), _p(self.ticket), s), "vtp_gemm_tn_grouped_items")


class WgradGroups(list):
    """WgradGroup objects launched back to back: a block whose problems sum over different token counts, where one launch cannot take them"""

    def launch(self):
        for g in self:
            g.launch()


def plan_block(problems, *, M: int, k_rows, accumulate: bool, device, scratch):
    """The weight gradients of one block (its Problem records; M: the block's token rows) as one object to launch().  Problems over
    different token counts (tail rows: proj / w12 / w3 over the compact rows beside qkv over all M) share the launch where the item-list
    kernel runs it, cut per problem (wgrad_group_mixed_ok); otherwise one group per count, the larger first, back to back."""
    counts = sorted({pr.Ktok for pr in problems}, reverse=True)
    if len(counts) > 1 and wgrad_group_mixed_ok(counts):
        counts = [None]
    parts = []
    for kt in counts:
        g = WgradGroup(M if kt is None else kt, k_rows=k_rows)
        for pr in problems:
            if kt is None or pr.Ktok == kt:
                g.add(pr.dy, pr.x, pr.gw, pr.gb, pr.N, pr.K, pr.swiglu_h, accumulate=accumulate, Ktok=pr.Ktok)
        parts.append(g.finalize(device, scratch))
    return parts[0] if len(parts) == 1 else WgradGroups(parts)
