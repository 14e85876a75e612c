"""tests/wgrad_ref.py checked on the CPU (no GPU, no library load): on the tables of tests/test_wgrad_kernels_gpu.py the emulation of an
item list equals the plain float64 product for every list that test launches and valid_items accepts them all; valid_items rejects
malformed lists; and every wrong variant of the emulation is rejected -- by the integer comparison at EVERY case where it changes
anything, by the barred comparison at the normal draws of those same cases."""
import pytest
import torch

import wgrad_ref as R


def _all_lists():
    """[(launch, list name, items, slots, piece)]: everything the GPU test launches.  The grid of the 8-phase kernel with `splits`
    forced is the uniform list of that many cuts (piece = 1: its token counts need not be multiples of 8)."""
    out = []
    for pair in R.PAIRS:
        L = R.pair_launch(pair)
        out += [(L, name, items, slots, 8) for name, items, slots in R.pair_lists(L)]
    for pair in R.PAIRS + R.PAIRS_8P:
        L = R.pair_launch(pair)
        out += [(L, f"8p_splits{n}") + R.uniform_items(L, n) + (1,) for n in (1, 2, 3)]
    out += [t + (8,) for t in R.multi_lists()]
    return out


ALL = _all_lists()
CANON = [t for t in ALL if not t[1].endswith(("_reversed", "_shuffled"))]   # the emulation sums per tile: the order cannot matter to it


def test_tables_cover_what_they_claim():
    for table, counts in ((R.PAIRS, R.ROWS_BOTH), (R.PAIRS_8P, R.ROWS_8P)):
        for key, wanted in ((0, range(len(R.SHAPES)) if table is R.PAIRS else ()), (1, counts)):
            for v in wanted:
                mine = [p for p in table if p[key] == v]
                assert {p[2] for p in mine} == {0, 1} and {p[3] for p in mine} == {0, 1}, (key, v, mine)
    assert {p[0] for p in R.PAIRS + R.PAIRS_8P} == set(range(len(R.SHAPES)))
    assert sum(p[4] for p in R.PAIRS) * 2 == len(R.PAIRS) and sum(p[4] for p in R.PAIRS_8P) * 2 == len(R.PAIRS_8P)
    assert all(rows % 8 == 0 for rows in R.ROWS_BOTH) and all(rows % 8 for rows in R.ROWS_8P)
    # the lists the issue names: 392 rows in 3; lengths 1, 7, 8, 9 and one past the 256 CUs; a clamped and an empty slice; parts < slots
    L = R.pair_launch(R.PAIRS[11])
    assert [tuple(it[1:3]) for it in R.uniform_items(L, 3)[0]] == [(0, 192), (192, 192), (384, 8)]
    lengths = {L.name: len(items) for L, _, items, _ in R.multi_lists()}
    assert [lengths[n] for n in ("len1", "len7", "len8", "len9", "len315")] == [1, 7, 8, 9, 315]
    every128, every64 = R.fixed_cut_items(R.MIXED, 128)[0], R.fixed_cut_items(R.MIXED, 64)[0]
    assert [tuple(it[1:3]) for it in every128 if it[0] == 2] == [(0, 128), (128, 128)]          # 136 rows: the second slice keeps 8
    assert [tuple(it[1:3]) for it in every64 if it[0] == 2] == [(0, 64), (64, 64), (128, 64), (192, 64)]   # ... the last one none
    items, slots = R.slots3_items()
    assert slots == 3 and sorted(it[3] for it in items) == [1, 3, 3, 3]
    for L, base in ((R.UNEVEN, 2), (R.UNEVEN_264, 1)):
        items, slots = R.uneven_items(L, base)
        assert slots == base + 1 and {it[3] for it in items} == {base, base + 1}


def test_planner_keeps_small_launches_at_one_slice():
    """why the uneven lists (c) are written by hand: below 1024 rows per slice the planner cuts nothing, whatever `cus` is"""
    for L in (R.UNEVEN, R.UNEVEN_264, R.MIXED):
        for cus in (16, 64):
            items, slots = R.wgrad_group_items(R.records(L), L.K, 1, cus=cus)
            assert slots == 1 and len(items) == R.tile0s(L)[1] and all(it[3] == 1 for it in items)
            R.valid_items(R.records(L), items, L.K)


@pytest.mark.parametrize("integer", [True, False])
def test_emulation_equals_the_plain_product(integer):
    for L, name, items, slots, piece in ALL:
        assert R.valid_items(R.records(L), items, L.K, piece)
        probs = R.build(L, integer)
        for launches in (1, 2):
            plain, emu = R.wgrad_ref(probs, launches=launches), R.wgrad_ref(probs, items, launches=launches, slots=slots)
            for p, (a, b) in enumerate(zip(plain, emu)):
                if integer:
                    ok = bool((a.gw == b.gw).all()) and (a.gb is None or bool((a.gb == b.gb).all()))
                else:   # float64 in another order: 1e-12 of the sum of absolute terms
                    ok = bool(((a.gw - b.gw).abs() <= 1e-12 * a.absw).all()) and (a.gb is None or bool(((a.gb - b.gb).abs() <= 1e-12 * (a.absb + 1)).all()))
                assert ok, (L.name, name, p)
        if integer:
            R.check_exact_inputs(probs, R.wgrad_ref(probs, launches=2))
    for k_rows in R.K_ROWS:
        L = R.limit_launch(k_rows)
        items, _ = R.cut_items(L, lambda p: [(0, L.K)])
        assert R.valid_items(R.records(L), items, L.K, 1, live=min(L.K, k_rows))
        plain, emu = R.wgrad_ref(R.build(L, integer), launches=2), R.wgrad_ref(R.build(L, integer), items, launches=2)
        assert all(torch.allclose(a.gw, b.gw, rtol=0, atol=1e-9) for a, b in zip(plain, emu))
    zero = R.wgrad_ref(R.build(R.limit_launch(0), integer), launches=2)      # nothing added; in overwrite mode that is zeros
    assert [float(r.gw.abs().max()) for r in zero] == [R.PREFILL, 0.0, R.PREFILL] and float(zero[0].gb[:-R.GUARD].abs().max()) == R.PREFILL


def test_valid_items_rejects_malformed_lists():
    L = R.pair_launch(R.PAIRS[7])                        # 248 x 264 over 192 rows: two tiles
    rows = R.records(L)
    good, _ = R.uniform_items(L, 3)                      # (0, 64) (64, 64) (128, 64) on both tiles
    assert R.valid_items(rows, good, L.K)

    def edit(i, **kw):
        names = ("tile", "kbeg", "kcount", "nparts", "part")
        items = [list(it) for it in good]
        for k, v in kw.items():
            items[i][names.index(k)] = v
        return items

    bad = {     # what: (the list, what valid_items must say about it)
        "a duplicated part": (edit(2, part=0), r"parts \[0, 0, 2\] of 3"),
        "a gap": (edit(2, kcount=56), "gap at row 120"),
        "an overlap": (edit(2, kbeg=0, kcount=128), "overlap at row 64"),
        "kbeg 32": (edit(2, kbeg=32, kcount=96), "kbeg 32 is no multiple of 64"),
        "kcount 4": (edit(4, kcount=4), "kcount 4 is no multiple of 8"),
        "inconsistent nparts": (edit(0, nparts=2), "inconsistent nparts"),
        "a missing tile": ([it for it in good if it[0] == 0], "every tile needs its items"),
        "a short cover": (edit(4, kcount=56), r"rows \[184, 192\) not covered"),
    }
    for what, (items, says) in bad.items():
        with pytest.raises(AssertionError, match=says):
            R.valid_items(rows, items, L.K)
            pytest.fail(f"valid_items accepted {what}")


# Why a variant may change no normal-draw case: none such -- each one moves an output by a whole product, a whole partial sum, the
# prefill (3.0) or a NaN, all far above a bar of some 1e-5 of the sum of absolute terms; the test below holds every variant to that.
@pytest.mark.parametrize("wrong", R.WRONG)
def test_wrong_variant_is_rejected(wrong):
    changed = 0
    for L, name, items, slots, piece in CANON:
        launches = 2
        for integer in (True, False):
            probs = R.build(L, integer)
            refs = R.wgrad_ref(probs, launches=launches)
            right = R.wgrad_ref(probs, items, launches=launches, slots=slots)
            off = R.wgrad_ref(probs, items, launches=launches, slots=slots, wrong=wrong)
            nparts = R.parts_of(L, items)
            for p, (rf, ok, w) in enumerate(zip(refs, right, off)):
                same = bool(((ok.gw == w.gw) | (torch.isnan(ok.gw) & torch.isnan(w.gw))).all()) and \
                    (ok.gb is None or bool(((ok.gb == w.gb) | (torch.isnan(ok.gb) & torch.isnan(w.gb))).all()))
                got_w, got_b = w.gw.float(), None if w.gb is None else w.gb.float()      # what a kernel that wrong would hand back
                if integer:
                    assert R.exact_ok(ok.gw.float(), None if ok.gb is None else ok.gb.float(), rf), (L.name, name, p)
                    assert R.exact_ok(got_w, got_b, rf) == same, f"{wrong} at {L.name} {name} problem {p}: changed but equal"
                    changed += not same
                else:
                    r = R.bar_ratio(got_w, got_b, rf, L.specs[p].Kp, nparts[p], launches)
                    assert R.bar_ratio(ok.gw.float(), None if ok.gb is None else ok.gb.float(), rf, L.specs[p].Kp, nparts[p], launches) <= 1.0
                    assert same or r > 1.0, f"{wrong} at {L.name} {name} problem {p}: worst error / bar = {r:.3g} passes"
    assert changed > 0, f"{wrong} changes no case of the tables: the inputs are wrong"
