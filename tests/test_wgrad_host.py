"""Host side of the weight gradients (vtp_amd/wgrad.py), no GPU and no launch: the named problem record against the hand-written
lists the older tests feed the planning code, what linear_bwd records with `defer`, and plan_block's partition of a block's problems
by token count -- one group per count, or one mixed item-list launch, exactly as Stack.backward decided it inline before."""
import pytest
import torch

from test_tail_rows_host import _check_items
from vtp_amd import _lib, ops, wgrad
from vtp_amd.engine import linear_bwd

BF = torch.bfloat16
MOVED = ("WgradGroup", "wgrad_group_fits", "gemm_cus", "wgrad_group_splits", "wgrad_group_kernel", "wgrad_k_cuts", "wgrad_group_items",
         "wgrad_mixed_splits", "wgrad_group_mixed_ok", "wgrad_group_uniform_items", "W4_TN_MIN_SLICE")


def test_ops_re_exports_the_moved_names():
    for n in MOVED:
        assert getattr(ops, n) is getattr(wgrad, n), n
    assert not hasattr(wgrad, "ops"), "wgrad.py stands below ops.py"


def test_group_record_is_the_abi_order_and_matches_the_hand_written_rows():
    assert wgrad.GroupRecord._fields == ("A", "B", "C", "colsum", "lda", "ldb", "ldc", "M", "N", "c_grp", "c_pre", "tile0", "accumulate",
                                         "K", "pad0", "pad1")
    D, H, Ktok = 768, 2048, 16
    g, t0 = ops.WgradGroup(Ktok), 0
    for N, K, gb in ((D, H, 0), (2 * H, D, 1), (D, D, 0), (3 * D, D, 1)):  # test_host_logic.py::rows(): w3, w12 (+bias), proj, qkv (+bias)
        hand = [1, 2, 3, gb, N, K, K, N, K, 0, 0, t0, 1, 0, 0, 0]
        t0 += ((N + 255) // 256) * ((K + 255) // 256)
        dy, x, gw = torch.empty(Ktok, N, dtype=BF), torch.empty(Ktok, K, dtype=BF), torch.empty(N * K)
        bias = torch.empty(N) if gb else None
        g.add(dy, x, gw, bias, N, K)
        r = g.rows[-1]
        assert isinstance(r, wgrad.GroupRecord) and (r.A, r.B, r.C) == (dy.data_ptr(), x.data_ptr(), gw.data_ptr())
        assert r.colsum == (bias.data_ptr() if gb else 0)
        assert list(r)[4:] == hand[4:] and r[7] == r.M == N and r[8] == r.N == K and r[11] == r.tile0
    assert g.ntiles == t0
    # the SwiGLU pair and a token count of its own land in their named slots
    g.add(torch.empty(8, 2 * H, dtype=BF), torch.empty(8, D, dtype=BF), torch.empty(2 * H * D), None, 2 * H, D, swiglu_h=H,
          accumulate=False, Ktok=8)
    r = g.rows[-1]
    assert (r.c_grp, r.c_pre, r.accumulate, r.K, r.pad0, r.pad1) == (-1, H, 0, 8, 0, 0)


def test_linear_bwd_with_defer_records_a_problem_and_launches_nothing(monkeypatch):
    def no_launch():
        raise AssertionError("linear_bwd(defer=...) must not reach the library")
    monkeypatch.setattr(_lib, "load", no_launch)
    M, N, K = 130, 64, 32
    dy, x, gw, gb = torch.empty(M, N, dtype=BF), torch.empty(M, K, dtype=BF), torch.empty(N * K), torch.empty(N)
    probs = []
    linear_bwd(None, "t", None, dy, x, M, None, need_dx=False, gw=gw, gb=gb, N=N, K=K, defer=probs)
    linear_bwd(None, "t", None, dy, x, M - 2, None, need_dx=False, gw=gw, gb=gb, N=N, K=K, bias_grad_done=True, swiglu_h=32, defer=probs)
    assert len(probs) == 2 and all(isinstance(p, wgrad.Problem) for p in probs)
    p = probs[0]
    assert (p.dy, p.x, p.gw, p.gb) == (dy, x, gw, gb) and (p.N, p.K, p.swiglu_h, p.Ktok) == (N, K, 0, M)
    assert probs[1].gb is None and probs[1].swiglu_h == 32 and probs[1].Ktok == M - 2


def _block(Mc, M, D=128, H=256):
    """the four problems of a block as its backward records them: w3, w12 and proj over Mc token rows, then qkv over all M"""
    out = []
    for N, K, bias, sh, rows in ((D, H, False, 0, Mc), (2 * H, D, True, H, Mc), (D, D, False, 0, Mc), (3 * D, D, True, 0, M)):
        out.append(wgrad.Problem(dy=torch.empty(rows, N, dtype=BF), x=torch.empty(rows, K, dtype=BF), gw=torch.empty(N * K),
                                 gb=torch.empty(N) if bias else None, N=N, K=K, swiglu_h=sh, Ktok=rows))
    return out


def _plan(probs, M, k_rows=None):
    return wgrad.plan_block(probs, M=M, k_rows=k_rows, accumulate=True, device="cpu", scratch={})


def test_plan_block_one_group_per_token_count(monkeypatch):
    """130 and 514 rows, no multiples of 8 (the smallest counts at which the split by count exists): two groups, the larger count first"""
    monkeypatch.delenv("VTP_GEMM4W_TN", raising=False)
    probs = _block(130, 514)
    grp = _plan(probs, 514)
    assert isinstance(grp, wgrad.WgradGroups) and [type(g) for g in grp] == [ops.WgradGroup] * 2
    assert [g.Ktok for g in grp] == [514, 130] and [len(g.rows) for g in grp] == [1, 3]
    for g in grp:
        assert not g.mixed and g.kernel == 0 and g.items is None and all(r.K == 0 for r in g.rows) and g.table.shape == (len(g.rows), 16)
    assert grp[0].rows[0].A == probs[3].dy.data_ptr() and [r.A for r in grp[1].rows] == [p.dy.data_ptr() for p in probs[:3]]
    assert [r.tile0 for r in grp[1].rows] == [0, 1, 3] and grp[1].ntiles == 4
    monkeypatch.setenv("VTP_GEMM4W_TN", "1")  # forcing the item-list kernel does not make these counts mixable
    assert [g.Ktok for g in _plan(probs, 514)] == [514, 130]
    monkeypatch.delenv("VTP_GEMM4W_TN")
    # multiples of 8 below the measured slice length: still one group per count; one count: one plain group
    assert [g.Ktok for g in _plan(_block(136, 520), 520)] == [520, 136]
    one = _plan(_block(520, 520), 520)
    assert type(one) is ops.WgradGroup and one.Ktok == 520 and len(one.rows) == 4 and not one.mixed


def test_plan_block_mixed_item_list(monkeypatch):
    monkeypatch.setenv("VTP_GEMM4W_TN", "1")
    g = _plan(_block(136, 520), 520)
    assert type(g) is ops.WgradGroup and g.mixed and g.kernel == 1 and g.Ktok == 520
    assert [r.K for r in g.rows] == [136, 136, 136, 0]
    items = g.items.tolist()
    assert len(items) == g.nitems and g.items.dtype == torch.int32
    assert _check_items(g, items, g.slots, 256) == [136, 136, 136, 520]


def test_plan_block_device_token_count_refuses_mixed_counts(monkeypatch):
    monkeypatch.setenv("VTP_GEMM4W_TN", "1")
    with pytest.raises(ValueError, match="a device token count takes one static token count for every problem"):
        _plan(_block(136, 520), 520, k_rows=torch.zeros(1, dtype=torch.int32))
    g = _plan(_block(520, 520), 520, k_rows=torch.zeros(1, dtype=torch.int32))
    assert (g.splits, g.kernel, g.items, g.slots) == (1, 0, None, 1)
