"""Host side of the tail-row plan (no GPU): the rows of the student's list forward that the SSL head reads, as the trunk's last block
takes them (ssl_engine.tail_row_plan / tail_row_map), and the work-item list of a grouped weight-gradient launch whose problems sum
over different token counts (ops.wgrad_group_items)."""
import numpy as np
import pytest
import torch

from vtp_amd import ops
from vtp_amd.ssl_engine import build_ssl_indices, tail_row_map

B, HW, N_LOCAL, HW_LOCAL = 2, 16, 2, 4
N = HW + 1


def _masks(kind):
    m = np.zeros((2 * B, HW), bool)
    if kind == "one_image_unmasked":  # crop 1 has no masked patch; n_masked < Tm
        m[0, [0, 5, 6]] = True
        m[2, [15]] = True
        m[3, 3:9] = True
    elif kind == "below_Tm":
        m[:, ::3] = True
    elif kind == "exactly_Tm":  # every patch of every crop: 64 = upperbound = Tm
        m[:] = True
    return m


def _gather(src_rows, idx):
    """gather_token_rows on row NUMBERS: -1 (padding) stays -1"""
    idx = np.asarray(idx)
    return np.where(idx >= 0, src_rows[np.maximum(idx, 0)], -1)


@pytest.mark.parametrize("kind", ["one_image_unmasked", "below_Tm", "exactly_Tm"])
@pytest.mark.parametrize("lead_rows", [0, 3 * N])
def test_tail_row_plan(kind, lead_rows):
    m = _masks(kind)
    p = build_ssl_indices(m, B, HW, N_LOCAL, HW_LOCAL, 1.0, 1.0, upperbound=64)
    assert p["Tm"] == 64 and (p["n_masked"] == 64) == (kind == "exactly_Tm")
    Ts, nl, L = p["Ts"], N_LOCAL * B, lead_rows
    g_rows, l_rows = 2 * B * N, N_LOCAL * B * (HW_LOCAL + 1)
    M = L + g_rows + l_rows
    tail, keep = p["student_tail_src"], p["student_tail_keep"]
    assert tail.dtype == np.int32 and keep.dtype == np.int32 and tail.shape == keep.shape == (Ts,)
    # the head's own order: [local cls | global cls | masked patches padded to Tm], padding stays -1
    assert np.array_equal(tail[:nl], p["student_local_src"] + g_rows)
    assert np.array_equal(tail[nl:], p["student_global_src"])
    n_pad = p["Tm"] - p["n_masked"]
    assert int((tail < 0).sum()) == n_pad and (n_pad == 0 or np.all(tail[Ts - n_pad:] == -1))
    assert np.array_equal(keep, np.where(tail >= 0, np.arange(Ts), -1))
    assert np.array_equal(p["teacher_keep"], np.where(p["teacher_src"] >= 0, np.arange(p["teacher_src"].shape[0]), -1))
    # compact rows = [0, L) | L + tail: what the head gathers from them is what the two gathers over the full rows give
    full = np.arange(M)
    compact = np.concatenate([full[:L], np.where(tail >= 0, L + tail, -1)])
    assert np.array_equal(compact[:L], np.arange(L)), "the prefix is the identity"
    old = np.concatenate([_gather(full[L + g_rows:], p["student_local_src"]), _gather(full[L:], p["student_global_src"])])
    new = _gather(compact[L:], keep)
    assert np.array_equal(old, new)
    # the inverse map: the prefix on itself, every kept row on its compact row, no duplicates, padding nowhere
    inv = tail_row_map(tail, L, M)
    assert inv.shape == (M,) and np.array_equal(inv[:L], np.arange(L))
    hit = inv[inv >= 0]
    assert len(np.unique(hit)) == len(hit) == L + Ts - n_pad
    for t in range(Ts):
        if tail[t] >= 0:
            assert inv[L + tail[t]] == L + t
        else:
            assert not np.any(inv == L + t), "a padding row of the compact buffer has no full row"
    assert np.all(compact[inv[inv >= 0]] == np.flatnonzero(inv >= 0))


def _group(problems, Ktok):
    """WgradGroup records without a device: [(N, K, has bias sum, token rows or None)]"""
    g = ops.WgradGroup(Ktok)
    for N_, K_, cs, kt in problems:
        rows = Ktok if kt is None else kt
        g.add(torch.empty(rows, N_, dtype=torch.bfloat16), torch.empty(rows, K_, dtype=torch.bfloat16), torch.empty(N_ * K_),
              torch.empty(N_) if cs else None, N_, K_, Ktok=kt)
    return g


def _check_items(g, items, slots, cus):
    Ks = [r[13] or g.Ktok for r in g.rows]
    by_tile = {}
    for tile, kbeg, kcount, nparts, part, *rest in items:
        assert rest == [0, 0, 0] and kbeg % 64 == 0 and kcount % 8 == 0 and kcount > 0
        by_tile.setdefault(tile, []).append((kbeg, kcount, nparts, part))
    assert sorted(by_tile) == list(range(g.ntiles)), "every tile of the launch has work"
    for tile, its in by_tile.items():
        p = max(i for i, r in enumerate(g.rows) if r[11] <= tile)
        its.sort()
        assert [x[3] for x in its] == list(range(len(its))) and all(x[2] == len(its) for x in its) and len(its) <= slots
        pos = 0
        for kbeg, kcount, _, _ in its:  # the K range of the tile's OWN problem, covered exactly once
            assert kbeg == pos
            pos += kcount
        assert pos == Ks[p], f"tile {tile} of problem {p}: covered [0, {pos}) of {Ks[p]} token rows"
    assert len(items) <= cus
    return Ks


@pytest.mark.parametrize("bias", [False, True])
def test_wgrad_group_items_mixed_token_counts_small(bias):
    """token counts (1280, 448, 448, 72): an even and an odd number of k-tiles and a K below one k-tile pair; N, K of 256 / 512"""
    probs = [(512, 256, bias, None), (256, 512, False, 448), (512, 512, bias, 448), (256, 256, bias, 72)]
    g = _group(probs, 1280)
    assert [r[13] for r in g.rows] == [0, 448, 448, 72]
    items, slots = ops.wgrad_group_items(g.rows, 1280, 0, cus=256)
    _check_items(g, items, slots, 256)


def test_wgrad_group_items_mixed_token_counts_bench_geometry():
    """the last trunk block of the default benchmark step: w3 / w12 / proj over the 11 040 tail rows, qkv over all 34 144; the workgroup
    counts follow the work -- qkv's tiles are cut until no K slice is longer than the tail problems' single one"""
    D, H, M, Mc = 768, 2048, 34144, 11040
    g = _group([(D, H, False, Mc), (2 * H, D, True, Mc), (D, D, False, Mc), (3 * D, D, True, None)], M)
    items, slots = ops.wgrad_group_items(g.rows, M, 0, cus=256)
    _check_items(g, items, slots, 256)
    assert max(it[2] for it in items) <= (Mc + 63) // 64 * 64
    uniform, _ = ops.wgrad_group_items(_group([(D, H, False, None), (2 * H, D, True, None), (D, D, False, None), (3 * D, D, True, None)], M).rows,
                                       M, 2, cus=256)
    assert max(it[2] for it in items) < 0.7 * max(it[2] for it in uniform)
    assert ops.wgrad_mixed_splits([24, 48, 9, 27], [Mc, Mc, Mc, M], 256) == [1, 1, 1, 4]
    assert ops.wgrad_group_mixed_ok([M, Mc]) and not ops.wgrad_group_mixed_ok([2134, 598])


def test_wgrad_group_items_uniform_cut_is_unchanged():
    """one token count for every problem: the list is the uniform base_splits cut (+ one slice for the bias-sum tiles) as before"""
    g = _group([(768, 2048, False, None), (4096, 768, True, None), (768, 768, False, None), (2304, 768, True, None)], 34144)
    items, slots = ops.wgrad_group_items(g.rows, 34144, 2, cus=256)
    _check_items(g, items, slots, 256)
    heavy = {it[0] for it in items if it[3] == 3}
    assert slots == 3 and len(heavy) == 16 + 9 and len(items) == 108 * 2 + 25
