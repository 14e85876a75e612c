"""The grouped weight-gradient kernels one by one, at their smallest cuts, against float64: the one-wave kernel on hand-built work-item
lists (csrc/gemm4w_tn.hip + gemm4w_tn_ktile.inc, vtp_gemm_tn_grouped_items), the 8-phase kernel with `splits` forced
(gemm8p_grouped_tn_kernel, vtp_gemm_tn_grouped) and its _limit sibling on a device token count.  Reference, tables and bars:
tests/wgrad_ref.py (pinned without a GPU by tests/test_wgrad_ref_host.py).  Integer inputs in [-3, 3] make every fp32 sum exact in any
order: those comparisons are EQUALITY with the float64 product, plus tickets back at zero and untouched guards.  Normal draws are held
to C_BAR n U (|prefill| + launches sum|dy||x|), and with one slice the one-wave kernel's gw is bit for bit the 8-phase kernel's.
Every list is checked by valid_items before it is launched; the whole `part` buffer is NaN before every launch; every operand has NaN
in its pad columns and in the rows behind the token count.  A launch with accumulate = 1 anywhere runs twice on the same scratch.

Where each mechanism that had no test is reached (names as printed, `wgrad_kernels: <kernel> <launch> <list>`):
  * a K slice shorter than one k-tile ................ one-wave 8x8_k8_b1a1 one, 64x72_k56_b0a0w one; 8-phase *_k1_*, *_k7_*, *_k63_*
  * ... shorter than the two-tile prologue ........... one-wave 120x136_k64_b1a0 one, 128x128_k72_b0a1w one, 136x120_k120_b1a1w one
  * an odd k-tile count (padded with a zero k-tile) .. one-wave 248x264_k192_b0a1 one and 264x248_k136_b1a0w one (3 k-tiles),
                                                       688x128sw_k264_b1a0 one (5), 8x8_k392_b0a0w cut3 ((0,192) (192,192) (384,8): 3, 3
                                                       and 1), len7 cut7 (1 per slice)
  * a slice the problem's token count clamps short ... one-wave mixed every128 (the second slice of the 136-row problem keeps 8 rows)
  * ... or empty (it still draws its ticket) ......... one-wave mixed every64 (its fourth slice); 8-phase limit0 (no k-tile at all)
  * outputs smaller than a wave's 64-column image .... 8x8, 520x8, 8x520 on both kernels; 64x72, 120x136, 136x120
  * item lists longer than one round of the CUs ...... one-wave len315 cut7 (five 520 x 520 problems over 448 rows, 45 tiles x 7)
  * item orders other than the planner's ............. every *_reversed and *_shuffled list
  * a tile with fewer parts than `slots` ............. one-wave slots3 parts3and1; uneven bias2_rest1 / bias3_rest2 (hand-written
                                                       uneven cuts: the planner cuts nothing at these sizes, see wgrad_ref.py)
  * leading dimensions wider than the operand ........ every launch name ending in `w`, and the `wide` problems of the named launches
Also: list lengths 1, 7, 8, 9 (len1, len7, len8, len9), the SwiGLU destination map across three row tiles (688x128sw), accumulate 0 / 1
and bias target or none on every shape and count, device counts 0 .. 1000 against the static 264 (limit0 .. limit1000).  The device count
0 IS launched: with k_split = 0 the 8-phase body computes no k-tile, stages nothing (H = 0), its barriers stay paired and nothing divides
by k_split, so the epilogue adds zeros -- read in gemm8p_body before this test was written."""
import pytest
import torch

import wgrad_ref as R
from test_kernels_gpu import DEV, ops

pytestmark = pytest.mark.gpu
KERNEL = {1: "one-wave", 0: "8-phase"}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(L, integer, kernel, items=None, slots=1, splits=None, k_rows=None):
    """one launch geometry on the device: returns ([(gw, gb)] on the CPU with their guards, tickets all zero?, the launch count)"""
    o = ops()
    probs = R.build(L, integer)
    outs = [(gw.to(DEV), None if gb is None else gb.to(DEV)) for gw, gb in R.outputs(probs)]
    dev = [(pr.A.to(DEV), pr.B.to(DEV)) for pr in probs]
    launches = 2 if any(s.acc for s in L.specs) else 1
    grp = o.WgradGroup(L.K, k_rows=None if k_rows is None else torch.tensor([k_rows], dtype=torch.int32, device=DEV))
    for pr, (A, B), (gw, gb) in zip(probs, dev, outs):
        s = pr.spec
        c0a, c0b = (R.A_COL0, R.B_COL0) if s.wide else (0, 0)
        grp.add(A[:, c0a:c0a + s.M], B[:, c0b:c0b + s.N], gw, gb, s.M, s.N, s.swiglu_h, accumulate=bool(s.acc),
                Ktok=None if k_rows is not None else s.Kp)
    grp.finalize(DEV, {})
    if k_rows is None:
        depth = slots if kernel == 1 else splits
        grp.part = torch.full((grp.ntiles * depth * 65536,), R.NAN, device=DEV)
        grp.ticket = torch.zeros(max(grp.ntiles, 256), dtype=torch.int32, device=DEV)
        if kernel == 1:
            grp.items, grp.nitems, grp.slots = torch.tensor(items, dtype=torch.int32, device=DEV), len(items), slots
        else:
            grp.splits = splits
    for _ in range(launches):
        grp.launch(kernel=kernel)
    torch.cuda.synchronize()
    clean = k_rows is not None or int(grp.ticket.abs().sum()) == 0
    return [(gw.cpu(), None if gb is None else gb.cpu()) for gw, gb in outs], clean, launches


def _guards_ok(L, got):
    ok = True
    for s, (gw, gb) in zip(L.specs, got):
        ok = ok and R.same_bits(gw[s.M * s.N:], torch.full((R.GUARD,), R.SENTINEL))
        ok = ok and (gb is None or R.same_bits(gb[s.M:], torch.full((R.GUARD,), R.SENTINEL)))
    return ok


def _check(L, name, kernel, items, slots, piece=8, live=None, **how):
    """the integer launch (exact) and the normal draw (barred) of one list; returns the normal draw's outputs"""
    assert R.valid_items(R.records(L), items, L.K, piece, live=live)
    tag = f"wgrad_kernels: {KERNEL[kernel]} {L.name} {name}"
    nparts = R.parts_of(L, items)
    for integer in (True, False):
        got, clean, launches = _run(L, integer, kernel, items=items, slots=slots, **how)
        refs = R.wgrad_ref(R.build(L, integer), launches=launches)
        guards = _guards_ok(L, got)
        if integer:
            R.check_exact_inputs(R.build(L, integer), refs)
            eq = [R.exact_ok(gw[:s.M * s.N], gb, rf) for s, (gw, gb), rf in zip(L.specs, got, refs)]
            yn = lambda b: "yes" if b else "NO"
            print(f"{tag}: {len(items)} items, {slots} slots, integers: exact {yn(all(eq))}, tickets zero {yn(clean)}, guards {yn(guards)}")
            for p, ok in enumerate(eq):
                assert ok, f"{tag}: " + R.first_wrong(L, items, p, got[p][0][:L.specs[p].M * L.specs[p].N], refs[p])
        else:
            rs = [R.bar_ratio(gw[:s.M * s.N], gb, rf, s.Kp, nparts[p], launches) for p, (s, (gw, gb), rf) in enumerate(zip(L.specs, got, refs))]
            print(f"{tag}: normal draw: worst error / bar = {max(rs):.4f}")
            for p, r in enumerate(rs):
                assert r <= 1.0, f"{tag}: problem {p} {tuple(L.specs[p])}: worst error / bar = {r:.4g}"
        assert clean, f"{tag}: tickets must return to zero"
        assert guards, f"{tag}: a guard element behind gw or gb was written"
    return got


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: R.pair_launch(p).name)
def test_one_wave_pairing_table(pair):
    """(a), (b), (d) on every (shape, token rows) pairing; with one slice, bit for bit the 8-phase kernel"""
    L = R.pair_launch(pair)
    for name, items, slots in R.pair_lists(L):
        got = _check(L, name, 1, items, slots)
        if name == "one":
            other, _, _ = _run(L, False, 0, splits=1)
            same = all(R.same_bits(a[0], b[0]) for a, b in zip(got, other))
            print(f"wgrad_kernels: one-wave {L.name} one: normal draw: gw bit for bit the 8-phase kernel's {'yes' if same else 'NO'}")
            assert same, f"{L.name}: one slice, and gw differs from the 8-phase kernel"


@pytest.mark.parametrize("pair", R.PAIRS + R.PAIRS_8P, ids=lambda p: R.pair_launch(p).name)
def test_eight_phase_pairing_table(pair):
    """`splits` 1, 2 and 3 forced; the launcher rounds the slices to whole k-tiles, so fewer may come out"""
    L = R.pair_launch(pair)
    for n in (1, 2, 3):
        items, slots = R.uniform_items(L, n)
        _check(L, f"splits{n}_gives{slots}", 0, items, slots, piece=1, splits=n)


MULTI = R.multi_lists()


@pytest.mark.parametrize("i", range(len(MULTI)), ids=[f"{t[0].name}_{t[1]}" for t in MULTI])
def test_one_wave_item_lists(i):
    """(c) - (g): uneven cuts, orders, list lengths up to 315, clamped and empty slices, a tile with fewer parts than slots"""
    L, name, items, slots = MULTI[i]
    _check(L, name, 1, items, slots)


@pytest.mark.parametrize("k_rows", R.K_ROWS)
def test_eight_phase_device_token_count(k_rows):
    """the _limit kernel: static count 264, rows from min(264, k_rows) on are NaN; 0 adds nothing (zeros in overwrite mode)"""
    L = R.limit_launch(k_rows)
    items, _ = R.cut_items(L, lambda p: [(0, L.K)])
    _check(L, "one", 0, items, 1, piece=1, live=min(L.K, k_rows), k_rows=k_rows)
