"""The grouped weight-gradient launches (csrc/gemm4w_tn.hip + gemm4w_tn_ktile.inc: the one-wave kernel on a work-item list;
gemm8p_grouped_tn_kernel / _limit_kernel of csrc/gemm8p.hip: the 8-phase kernel on a uniform tiles x splits grid) restated on the CPU in
float64, the case tables of tests/test_wgrad_kernels_gpu.py, and the bars.  Not a test module; tests/test_wgrad_ref_host.py pins the
item-list emulation against the plain product and shows, at the GPU test's own inputs, that wrong variants are rejected.  Conventions,
`U`, `PREFILL`, `SENTINEL`, `same_bits`, `ratio`, `assert_exact_case` and `draw` are those of tests/glue_ref.py.

Kernel terms throughout: a problem is C[M, N] (+)= A[Kp, M]^T B[Kp, N] with A = dy, B = x, so M = rows of dW = columns of dy, N = columns
of dW = columns of x, Kp = the problem's own token rows.  (ops.WgradGroup.add names the same two numbers N and K.)  A tile is 256 x 256, a
staged k-tile is 64 token rows, a staging piece 8 rows, the prologue of the one-wave kernel 2 k-tiles.

What the kernels do with `accumulate`: gw (+)= product, per problem; the bias sums always ACCUMULATE into gb (one atomic per row and K
slice, straight from the k loop: they never pass through the combine), so gb = prefill + launches x column sums in both modes.

Bars.  Integer cases: live values are integers in [-3, 3], |prefill| + launches sum|dy||x| < 2^14 per output, every fp32 partial sum is
exact in any order and the result must EQUAL the float64 value; tickets all zero afterwards; the guard elements behind gw and gb keep
their bits.  Normal draws: |got - ref64| <= C_BAR n U (|prefill| + launches sum|dy||x|) per element, n = Kp + nparts + launches the
length of the longest chain (one rounding per product, one per combined part, one per accumulate).  C_BAR = 2 allows for MFMA and v_dot2
internal additions that may round toward zero instead of to nearest; how CDNA4 rounds there is not something this project has measured:
a stated allowance, not a fit.  The bar is loose on purpose (the expected error grows like sqrt(n) U); the integer cases are the sharp
ones, the normal draws catch what small integers cannot (a bf16 operand reinterpreted, an exponent path).

Wrong variants of the emulation (`wrong=`): 'drop_krow' (one k row of one slice missing), 'dup_krow' (the row at a 64-row k-tile boundary
counted twice), 'no_zero_pad' (a slice whose length is no multiple of 64 also sums the rows up to the next multiple), 'no_clamp' (a
slice clamped by the problem's K sums to kbeg + kcount), 'skip_part' (the combine leaves one part out), 'stale_part' (the combine adds a
slot nobody wrote: the NaN the part buffer is prefilled with), 'no_swiglu', 'ignore_accumulate', 'colsum_every_tile_column' (every tile
column adds the bias sum) and 'colsum_clamped_cols' (the staging columns clamped to M - 8 are duplicates of the last eight; their sums
are not masked and land on remap(m) for m >= M).

Item lists (c): the planner (wgrad_group_items) keeps every tile at ONE slice below 1024 rows per slice whatever `cus` is -- its
`>= 1024` rule; tests/test_wgrad_ref_host.py asserts that for cus = 16 and 64 on the launches here -- so the uneven lists are written by
hand (uneven_items: the bias tiles one slice more than the others, in the planner's order)."""
import functools
import random
from collections import namedtuple

import torch

from glue_ref import BF, F32, F64, GUARD, NAN, PREFILL, SENTINEL, U, assert_exact_case, draw, gen, ratio, same_bits  # noqa: F401
from vtp_amd.wgrad import GroupRecord, wgrad_group_items, wgrad_group_uniform_items, wgrad_k_cuts  # host-side planner: loads no library

C_BAR = 2.0
DEAD_ROWS = 64               # NaN rows behind the launch's token count in every operand
LDA_PAD, LDB_PAD = 24, 8     # wide operands: lda = M + 24, ldb = N + 8 ...
A_COL0, B_COL0 = 16, 8       # ... the live columns start here; everything else is NaN
WRONG = ("drop_krow", "dup_krow", "no_zero_pad", "no_clamp", "skip_part", "stale_part", "no_swiglu", "ignore_accumulate",
         "colsum_every_tile_column", "colsum_clamped_cols")

# one problem: swiglu_h > 0 sends row m of the product to (m >> 4) * 8 + (m & 7) (+ swiglu_h if m & 8); wide: the operands are column
# slices of wider matrices
Spec = namedtuple("Spec", "M N Kp bias acc swiglu_h wide")
# one launch geometry: K = GroupArgs.K, the launch's token count (a problem with Kp < K makes the launch a mixed one)
Launch = namedtuple("Launch", "name specs K")


def S(M, N, Kp, bias, acc, swiglu_h=0, wide=0):
    return Spec(M, N, Kp, int(bias), int(acc), swiglu_h, int(wide))


# ------------------------------------------------------------------------------------------------------------------ the tables
SHAPES = ((8, 8, 0), (64, 72, 0), (120, 136, 0), (128, 128, 0), (136, 120, 0), (256, 256, 0), (264, 248, 0), (248, 264, 0), (520, 8, 0),
          (8, 520, 0), (688, 128, 344))          # (M, N, swiglu_h); the last: three row tiles, 176 rows in the last, the map crosses tiles
ROWS_BOTH = (8, 56, 64, 72, 120, 128, 136, 192, 200, 256, 264, 392)
ROWS_8P = (1, 7, 63, 65, 130)                    # the one-wave kernel needs multiples of 8
STATIC_LIMIT, K_ROWS = 264, (0, 1, 8, 63, 64, 65, 130, 264, 1000)

# The pairing table: (shape index, token rows, bias, accumulate, wide).  Every shape and every count meets bias 1 and 0 and
# accumulate 1 and 0 (test_wgrad_ref_host.py checks that); half the cases are wide.  Both kernels run all of PAIRS.
PAIRS = (
    (0, 8, 1, 1, 0), (1, 56, 0, 0, 1), (2, 64, 1, 0, 0), (3, 72, 0, 1, 1), (4, 120, 1, 1, 1), (5, 128, 0, 0, 0),
    (6, 136, 1, 0, 1), (7, 192, 0, 1, 0), (8, 200, 1, 1, 0), (9, 256, 0, 0, 1), (10, 264, 1, 0, 0), (0, 392, 0, 0, 1),
    (1, 128, 1, 1, 0), (5, 256, 1, 1, 1), (9, 392, 1, 1, 0), (2, 136, 0, 1, 1), (6, 264, 0, 1, 0), (10, 64, 0, 1, 1),
    (3, 192, 1, 0, 0), (7, 72, 1, 0, 1), (4, 200, 0, 0, 0), (8, 8, 0, 0, 1), (0, 56, 1, 1, 0), (5, 120, 0, 0, 1),
)
# ... and the 8-phase kernel alone these
PAIRS_8P = (
    (0, 1, 1, 1, 0), (6, 1, 0, 0, 1), (2, 7, 1, 0, 0), (10, 7, 0, 1, 1), (3, 63, 1, 1, 1), (8, 63, 0, 0, 0),
    (9, 65, 1, 0, 1), (4, 65, 0, 1, 0), (7, 130, 1, 1, 0), (1, 130, 0, 0, 1),
)


def pair_launch(pair):
    si, rows, bias, acc, wide = pair
    M, N, h = SHAPES[si]
    return Launch(f"{M}x{N}{'sw' if h else ''}_k{rows}_b{bias}a{acc}{'w' if wide else ''}", (S(M, N, rows, bias, acc, h, wide),), rows)


# multi-problem launches of the one-wave kernel
UNEVEN = Launch("uneven", (S(264, 520, 392, 1, 1, 0, 1), S(688, 128, 392, 1, 0, 344, 0), S(136, 120, 392, 0, 1, 0, 1)), 392)
UNEVEN_264 = Launch("uneven264", (S(264, 248, 264, 1, 0, 0, 0), S(8, 520, 264, 1, 1, 0, 1), S(248, 264, 264, 0, 1, 0, 0)), 264)
LEN1 = Launch("len1", (S(8, 8, 8, 1, 1),), 8)
LEN7 = Launch("len7", (S(256, 256, 448, 1, 1),), 448)
LEN8 = Launch("len8", (S(520, 8, 72, 1, 0, 0, 1), S(8, 520, 72, 0, 1), S(264, 248, 72, 1, 1, 0, 1)), 72)
LEN9 = Launch("len9", (S(520, 8, 136, 1, 1, 0, 1),), 136)
LONG = Launch("len315", tuple(S(520, 520, 448, i & 1, (i >> 1) & 1, 0, i % 3 == 0) for i in range(5)), 448)   # 45 tiles x 7 slices
MIXED = Launch("mixed", (S(264, 248, 256, 1, 1, 0, 1), S(136, 120, 136, 1, 0)), 256)
SLOTS3 = Launch("slots3", (S(256, 256, 200, 1, 1), S(8, 8, 200, 1, 0, 0, 1)), 200)


def limit_launch(k_rows):
    live = min(STATIC_LIMIT, k_rows)
    return Launch(f"limit{k_rows}", (S(264, 248, live, 1, 1, 0, 1), S(688, 128, live, 1, 0, 344, 0), S(8, 520, live, 0, 1, 0, 1)), STATIC_LIMIT)


def cdiv(a, b):
    return -(-a // b)


def tiles_of(spec):
    return cdiv(spec.M, 256), cdiv(spec.N, 256)


def tile0s(launch):
    t, out = 0, []
    for s in launch.specs:
        out.append(t)
        t += tiles_of(s)[0] * tiles_of(s)[1]
    return out, t


def records(launch):
    """the GroupRecord rows ops.WgradGroup.add would build, without a device: pointers are 0 / 1 (only `colsum != 0` is ever read)"""
    t0, _ = tile0s(launch)
    return [GroupRecord(A=0, B=0, C=0, colsum=s.bias, lda=s.M, ldb=s.N, ldc=s.N, M=s.M, N=s.N, c_grp=-1 if s.swiglu_h else 0,
                        c_pre=s.swiglu_h, tile0=t, accumulate=s.acc, K=0 if s.Kp == launch.K else s.Kp) for s, t in zip(launch.specs, t0)]


# ------------------------------------------------------------------------------------------------------------------ item lists
def cut_items(launch, cuts_of):
    """every tile of problem p cut as cuts_of(p), slice-major over the launch's tiles (the order of wgrad_group_uniform_items)"""
    t0, _ = tile0s(launch)
    per_tile = []
    for p, s in enumerate(launch.specs):
        cs = cuts_of(p)
        per_tile += [(t0[p] + lt, cs) for lt in range(tiles_of(s)[0] * tiles_of(s)[1])]
    deepest = max(len(cs) for _, cs in per_tile)
    items = [[t, cs[z][0], cs[z][1], len(cs), z, 0, 0, 0] for z in range(deepest) for t, cs in per_tile if z < len(cs)]
    return items, deepest


def uniform_items(launch, n):
    """(b): every tile in the n uniform cuts of wgrad_k_cuts -- for one token count this IS wgrad_group_uniform_items, and the grid of
    the 8-phase kernel with `splits = n`"""
    items, slots = cut_items(launch, lambda p: wgrad_k_cuts(launch.specs[p].Kp, n))
    if all(s.Kp == launch.K for s in launch.specs):
        assert (items, slots) == wgrad_group_uniform_items(tile0s(launch)[1], launch.K, n)
    return items, slots


def uneven_items(launch, base):
    """(c), by hand: the tiles that also form a bias gradient (first tile column, bias target) in base + 1 slices, the others in base;
    the planner's order: per problem, the heavier-cut tiles first, slice-major inside a group"""
    items, slots = [], 1
    for s, r in zip(launch.specs, records(launch)):
        tm, tn = tiles_of(s)
        for heavy in (True, False):
            grp = [r.tile0 + lt for lt in range(tm * tn) if (bool(s.bias) and lt % tn == 0) == heavy]
            if not grp:
                continue
            cs = wgrad_k_cuts(s.Kp, base + 1 if heavy else base)
            slots = max(slots, len(cs))
            for z, (kb, kc) in enumerate(cs):
                items += [[t, kb, kc, len(cs), z, 0, 0, 0] for t in grp]
    return items, slots


def fixed_cut_items(launch, size):
    """(f): every problem cut at multiples of `size` up to the LAUNCH's K -- a short problem's later slices are clamped or empty"""
    cs = [(b, min(launch.K, b + size) - b) for b in range(0, launch.K, size)]
    return cut_items(launch, lambda p: cs)


def slots3_items():
    """(g): the 256 x 256 tile in three parts, the 8 x 8 tile in one"""
    return [[0, 0, 64, 3, 0, 0, 0, 0], [1, 0, 200, 1, 0, 0, 0, 0], [0, 64, 64, 3, 1, 0, 0, 0], [0, 128, 72, 3, 2, 0, 0, 0]], 3


def orders(name, items, slots):
    """(d): the list, reversed, and a fixed-seed shuffle -- any order is valid, the last arriver combines"""
    sh = list(items)
    random.Random(len(items) * 7919 + slots).shuffle(sh)
    return [(name, items, slots), (name + "_reversed", items[::-1], slots), (name + "_shuffled", sh, slots)]


def pair_lists(launch):
    """lists of a pairing case on the one-wave kernel: (a) one slice per tile; (b) 2 and 3 uniform cuts where the token count gives
    that many, each also reversed and shuffled (d)"""
    out, seen = [("one",) + uniform_items(launch, 1)], {1}
    for n in (2, 3):
        items, slots = uniform_items(launch, n)
        if slots not in seen:
            seen.add(slots)
            out += orders(f"cut{slots}", items, slots)
    return out


def multi_lists():
    """[(launch, list name, items, slots)] of the multi-problem launches: (c) + (d), (e), (f), (g)"""
    out = []
    for L in (UNEVEN, UNEVEN_264):
        for base in (1, 2):
            out += [(L,) + o for o in orders(f"bias{base + 1}_rest{base}", *uneven_items(L, base))]
    out.append((LEN1, "one") + uniform_items(LEN1, 1))
    out.append((LEN7, "cut7") + uniform_items(LEN7, 7))
    out.append((LEN8, "one") + uniform_items(LEN8, 1))
    out.append((LEN9, "cut3") + uniform_items(LEN9, 3))
    out.append((LONG, "cut7") + uniform_items(LONG, 7))
    out += [(MIXED,) + o for size in (128, 64) for o in orders(f"every{size}", *fixed_cut_items(MIXED, size))]
    out += [(SLOTS3,) + o for o in orders("parts3and1", *slots3_items())]
    return out


def valid_items(rows, items, Ktok, piece=8, live=None):
    """asserts a list well formed: per tile the parts 0 .. nparts - 1 once each with one nparts; kbeg % 64 == 0 and kcount % piece == 0
    (8 rows for the one-wave kernel; 1 for the grid of the 8-phase kernel written as a list); the ranges, clamped to the problem's own
    token count, partition [0, Kp).  rows: GroupRecord-like (M, N, tile0, K).  live: the device count of a _limit launch, which bounds
    every problem instead of its record (and may be 0)."""
    rows = [GroupRecord._make(r) for r in rows]
    ntiles = sum(cdiv(r.M, 256) * cdiv(r.N, 256) for r in rows)
    by_tile = {}
    for it in items:
        tile, kbeg, kcount, nparts, part = (int(v) for v in it[:5])
        assert 0 <= tile < ntiles, f"tile {tile} outside [0, {ntiles})"
        assert kbeg >= 0 and kbeg % 64 == 0, f"tile {tile}: kbeg {kbeg} is no multiple of 64"
        assert kcount >= 0 and kcount % piece == 0, f"tile {tile}: kcount {kcount} is no multiple of {piece}"
        by_tile.setdefault(tile, []).append((kbeg, kcount, nparts, part))
    assert sorted(by_tile) == list(range(ntiles)), "every tile needs its items"
    for tile, its in by_tile.items():
        r = max((r for r in rows if r.tile0 <= tile), key=lambda r: r.tile0)
        Kp = (int(r.K) or int(Ktok)) if live is None else int(live)
        assert piece == 1 or Kp % piece == 0, f"token count {Kp}"
        nparts = its[0][2]
        assert all(i[2] == nparts for i in its), f"tile {tile}: inconsistent nparts"
        assert sorted(i[3] for i in its) == list(range(nparts)), f"tile {tile}: parts {sorted(i[3] for i in its)} of {nparts}"
        pos = 0
        for kbeg, kcount, _, _ in sorted(its):
            n = max(0, min(kcount, Kp - kbeg))
            if n == 0:
                continue
            assert kbeg == pos, f"tile {tile}: {'gap' if kbeg > pos else 'overlap'} at row {pos} (next range starts at {kbeg})"
            pos = kbeg + n
        assert pos == Kp, f"tile {tile}: rows [{pos}, {Kp}) not covered"
    return True


# ------------------------------------------------------------------------------------------------------------------ operands
class Problem:
    """host tensors of one problem: A / B bf16 [Kp + dead, ld] with NaN in the dead rows and pad columns, a / b the column slices the
    kernel gets (all rows: the dead ones lie behind the token count), and where its tiles start"""

    def __init__(self, spec, A, B, tile0):
        self.spec, self.A, self.B, self.tile0 = spec, A, B, tile0
        c0a, c0b = (A_COL0, B_COL0) if spec.wide else (0, 0)
        self.a, self.b = A[:, c0a:c0a + spec.M], B[:, c0b:c0b + spec.N]

    def dest(self, wrong=None):
        """destination row of product row m"""
        m = torch.arange(self.spec.M + 256)
        if self.spec.swiglu_h and wrong != "no_swiglu":
            return (m >> 4) * 8 + (m & 7) + torch.where((m & 8) != 0, self.spec.swiglu_h, 0)
        return m


@functools.lru_cache(maxsize=None)
def build(launch, integer):
    """the operands of a launch: live values integers in [-3, 3] or a normal draw; everything else NaN"""
    t0, _ = tile0s(launch)
    out = []
    for p, (s, t) in enumerate(zip(launch.specs, t0)):
        g = gen(s.M, s.N, s.Kp, p, integer, s.wide, 59)
        rows = launch.K + DEAD_ROWS
        A = torch.full((rows, s.M + (LDA_PAD if s.wide else 0)), NAN, dtype=BF)
        B = torch.full((rows, s.N + (LDB_PAD if s.wide else 0)), NAN, dtype=BF)
        pr = Problem(s, A, B, t)
        pr.a[:s.Kp] = draw((s.Kp, s.M), g, integer, BF)
        pr.b[:s.Kp] = draw((s.Kp, s.N), g, integer, BF)
        out.append(pr)
    return out


def outputs(problems):
    """[(gw f32 [M N + GUARD], gb f32 [M + GUARD] or None)] as they stand before a launch: PREFILL, the guards SENTINEL"""
    out = []
    for pr in problems:
        s = pr.spec
        gw = torch.full((s.M * s.N + GUARD,), PREFILL)
        gw[s.M * s.N:] = SENTINEL
        gb = None
        if s.bias:
            gb = torch.full((s.M + GUARD,), PREFILL)
            gb[s.M:] = SENTINEL
        out.append((gw, gb))
    return out


# ------------------------------------------------------------------------------------------------------------------ the reference
Ref = namedtuple("Ref", "gw gb absw absb")   # float64: gw [M, N]; gb [M + GUARD] (guard = SENTINEL) or None; sum|dy||x|, sum|dy| alike


def _finish(pr, W, cb, launches, wrong, extra=None):
    """product rows -> destinations, prefill and accumulate; extra: (destination, value) pairs a wrong variant adds to gb"""
    s = pr.spec
    dst = pr.dest(wrong)[:s.M]
    acc = bool(s.acc) != (wrong == "ignore_accumulate")
    gw = torch.zeros(s.M, s.N, dtype=F64)
    gw[dst] = W
    gw = PREFILL + launches * gw if acc else gw
    gb = None
    if s.bias:
        gb = torch.full((s.M + GUARD,), float(SENTINEL), dtype=F64)
        gb[:s.M] = PREFILL
        gb[dst] += launches * cb
        for d, v in extra or ():
            gb[d] += launches * v
    return gw, gb


def wgrad_ref(problems, items=None, launches=1, wrong=None, slots=None):
    """[Ref] per problem.  items None: the plain product over the problem's own Kp rows.  Otherwise the emulation of the item list:
    each item adds the rows [kbeg, kbeg + max(0, min(kcount, Kp - kbeg))) of its tile, the parts of a tile are summed, the bias sums
    come from the first tile column only.  With wrong=None both are the same numbers for every valid list."""
    out = []
    once = {"drop_krow": False, "dup_krow": False, "skip_part": False}   # variants that hit ONE item / tile of the launch
    slots = slots if slots is not None else max([int(it[3]) for it in items], default=1) if items is not None else 1
    for pr in problems:
        s = pr.spec
        a, b = pr.a[:s.Kp].double(), pr.b[:s.Kp].double()
        absw, absb = a.abs().T @ b.abs(), a.abs().sum(0)
        extra = []
        if items is None:
            assert wrong is None
            W, cb = a.T @ b, a.sum(0)
        else:
            Af, Bf = pr.a.double(), pr.b.double()      # all rows: a wrong variant may reach the dead ones
            W, cb = torch.zeros(s.M, s.N, dtype=F64), torch.zeros(s.M, dtype=F64)
            tm, tn = tiles_of(s)
            for lt in range(tm * tn):
                m0, n0 = lt // tn * 256, lt % tn * 256
                m1, n1 = min(m0 + 256, s.M), min(n0 + 256, s.N)
                mine = [it for it in items if int(it[0]) == pr.tile0 + lt]
                nparts = int(mine[0][3])
                if wrong == "stale_part" and nparts < slots:
                    W[m0:m1, n0:n1] += NAN
                for it in mine:
                    kbeg, kcount, part = int(it[1]), int(it[2]), int(it[4])
                    n = max(0, min(kcount, s.Kp - kbeg))
                    rows = list(range(kbeg, kbeg + n))
                    if wrong == "drop_krow" and n > 0 and not once[wrong]:
                        rows, once[wrong] = rows[:-1], True
                    if wrong == "dup_krow" and n > 64 and not once[wrong]:
                        rows, once[wrong] = rows + [kbeg + 64], True
                    if wrong == "no_zero_pad" and n % 64:
                        rows = list(range(kbeg, min(kbeg + cdiv(n, 64) * 64, Af.shape[0])))
                    if wrong == "no_clamp" and n < kcount:
                        rows = list(range(kbeg, min(kbeg + kcount, Af.shape[0])))
                    if wrong == "skip_part" and nparts > 1 and part == nparts - 1 and not once[wrong]:
                        once[wrong] = True
                        continue
                    W[m0:m1, n0:n1] += Af[rows, m0:m1].T @ Bf[rows, n0:n1]
                    if s.bias and (n0 == 0 or wrong == "colsum_every_tile_column"):
                        cb[m0:m1] += Af[rows, m0:m1].sum(0)
                        if wrong == "colsum_clamped_cols" and m1 == s.M:
                            dst = pr.dest()
                            for m in range(s.M, m0 + 256):
                                if int(dst[m]) < s.M + GUARD:
                                    extra.append((int(dst[m]), Af[rows, s.M - 8 + (m & 7)].sum(0)))
        gw, gb = _finish(pr, W, cb, launches, wrong, extra)
        aw, ab = _finish(pr, absw, absb, launches, None)
        aw = aw if s.acc else aw + PREFILL          # the bar counts |prefill| in both modes
        if ab is not None:
            ab[s.M:] = 0.0                          # the guard: a zero bar, met exactly
        out.append(Ref(gw, gb, aw, ab))
    return out


# ------------------------------------------------------------------------------------------------------------------ the comparisons
def parts_of(launch, items):
    """the longest combine of each problem (its largest nparts)"""
    t0, nt = tile0s(launch)
    ends = t0[1:] + [nt]
    return [max(int(it[3]) for it in items if lo <= int(it[0]) < hi) for lo, hi in zip(t0, ends)]


def exact_ok(got_gw, got_gb, ref):
    """integer cases: equality with the float64 value, element for element (a NaN is never equal)"""
    ok = bool((got_gw.double().view_as(ref.gw) == ref.gw).all())
    if ref.gb is not None:
        ok = ok and bool((got_gb.double() == ref.gb).all())
    return ok


def bar_ratio(got_gw, got_gb, ref, Kp, nparts, launches):
    """normal draws: worst |got - ref| / (C_BAR n U (|prefill| + launches sum|terms|)); ref.absw / absb already hold the bracket"""
    n = Kp + nparts + launches
    r = ratio(got_gw.view_as(ref.gw), ref.gw, C_BAR * n * U * ref.absw)
    if ref.gb is not None:
        r = max(r, ratio(got_gb, ref.gb, C_BAR * n * U * ref.absb))
    return r


def check_exact_inputs(problems, refs):
    """the premise of the integer cases, per output"""
    for pr, rf in zip(problems, refs):
        s = pr.spec
        assert_exact_case(rf.absw.max() if rf.absw.numel() else 0.0, 0.0, pr.a[:s.Kp], pr.b[:s.Kp])   # (absw holds |prefill| already)
        assert float(rf.absw.max()) < 2.0 ** 14
        assert not torch.isnan(rf.gw).any() and (rf.gb is None or not torch.isnan(rf.gb).any())


def first_wrong(launch, items, p, got_gw, ref):
    """names the first wrong element of problem p's gw: destination (row, column), the tile it comes from and the items covering it"""
    s = launch.specs[p]
    bad = (got_gw.double().view_as(ref.gw) != ref.gw).nonzero()
    if not len(bad):
        return f"problem {p} {tuple(s)}: gw equal; gb or a guard differs"
    r, c = (int(v) for v in bad[0])
    dst = Problem(s, torch.empty(0, s.M + LDA_PAD), torch.empty(0, s.N + LDB_PAD), 0).dest()[:s.M]
    m = int((dst == r).nonzero()[0])
    tile = tile0s(launch)[0][p] + (m // 256) * tiles_of(s)[1] + c // 256
    cover = [tuple(int(v) for v in it[:5]) for it in items if int(it[0]) == tile]
    return (f"problem {p} {tuple(s)}: first wrong gw[{r}, {c}] = {float(got_gw.view_as(ref.gw)[r, c])!r}, expected {float(ref.gw[r, c])!r} "
            f"({len(bad)} wrong); product row {m}, tile {tile}, items (tile, kbeg, kcount, nparts, part) {cover}")
