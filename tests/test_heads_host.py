"""CPU-side checks of the head store LinearProbe and SegProbe share (vtp_amd/heads.py): the grouping, the learning rates and the
order the checkpoint code walks the heads in.  No library and no GPU: the store is plain torch."""
import math

import pytest
import torch

from vtp_amd.heads import HeadStore, cosine_factor

D, C = 8, 3


def _init(heads):
    """distinct host tensors per key, in the list's order"""
    g = torch.Generator().manual_seed(0)
    return {key: (torch.randn(C, K, generator=g), torch.randn(C, generator=g)) for key, _, K, _, _ in heads}


def _probe_like():
    """LinearProbe's mapping: group id (n, avgpool), K = (n + avgpool) D, col0 = (n_max - n) D; n_max = 4, groups interleaved"""
    spec = [("a", 1, True, 0.1), ("b", 4, True, 0.2), ("c", 1, True, 0.3), ("d", 4, False, 0.4), ("e", 4, True, 0.5)]
    return [(k, (n, ap), (n + (1 if ap else 0)) * D, (4 - n) * D, lr) for k, n, ap, lr in spec]


def _seg_like():
    """SegProbe's mapping: group id n, K = n D, col0 = (n_max - n) D; n_max = 2"""
    return [(k, n, n * D, (2 - n) * D, lr) for k, n, lr in (("one_a", 1, 0.5), ("two", 2, 0.25), ("one_b", 1, 0.1))]


def test_groups_stand_in_first_appearance_order_and_keys_group_by_group():
    heads = _probe_like()
    init = _init(heads)
    s = HeadStore(heads, init, "cpu")
    assert [g.id for g in s.groups] == [(1, True), (4, True), (4, False)]
    assert [g.keys for g in s.groups] == [["a", "c"], ["b", "e"], ["d"]] and s.keys == ["a", "c", "b", "e", "d"]
    assert [(g.H, g.K, g.col0, g.off) for g in s.groups] == [(2, 2 * D, 3 * D, 0), (2, 5 * D, 0, 2), (1, 4 * D, 0, 4)]
    assert [g.base_lr for g in s.groups] == [[0.1, 0.3], [0.2, 0.5], [0.4]]
    for g in s.groups:
        assert g.weight.shape == (g.H, C, g.K) and g.bias.shape == (g.H, C) and g.lr.shape == (g.H,)
        for t in (g.weight, g.bias, g.m_weight, g.m_bias, g.lr):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert not bool(g.m_weight.any()) and not bool(g.m_bias.any()) and not bool(g.lr.any())
        for i, k in enumerate(g.keys):  # the caller's tensors, stacked: the store draws nothing
            assert torch.equal(g.weight[i], init[k][0]) and torch.equal(g.bias[i], init[k][1])

    seg = HeadStore(_seg_like(), _init(_seg_like()), "cpu")
    assert [g.id for g in seg.groups] == [1, 2] and seg.keys == ["one_a", "one_b", "two"]
    assert [(g.H, g.K, g.col0, g.off) for g in seg.groups] == [(2, D, D, 0), (1, 2 * D, 0, 2)]


def test_the_store_consumes_no_random_numbers():
    torch.manual_seed(3)
    want = torch.rand(4)
    torch.manual_seed(3)
    HeadStore(_seg_like(), _init(_seg_like()), "cpu")
    assert torch.equal(torch.rand(4), want)


@pytest.mark.parametrize("max_iter", [None, 10])
def test_learning_rates_follow_the_closed_form(max_iter):
    heads = _probe_like()
    s = HeadStore(heads, _init(heads), "cpu", max_iter)
    base = {k: lr for k, _, _, _, lr in heads}
    for step in (0, 1, 7, 10):
        f = 1.0 if max_iter is None else 0.5 * (1.0 + math.cos(math.pi * step / max_iter))
        assert cosine_factor(step, max_iter) == f
        got = s.learning_rates(step)
        assert list(got) == s.keys and got == {k: base[k] * f for k in s.keys}
    if max_iter is not None:
        assert s.learning_rates(0) == base and all(abs(v) < 1e-16 for v in s.learning_rates(max_iter).values())


def test_set_lr_rounds_the_fp64_product_once():
    heads = [("x", 0, D, 0, 0.1), ("y", 0, D, 0, 1.0 / 3.0), ("z", 1, D, 0, 0.7)]
    s = HeadStore(heads, _init(heads), "cpu", 10)
    f = cosine_factor(3, 10)
    g = s.groups[0]
    s.set_lr(g, f)
    want = torch.tensor([0.1 * f, (1.0 / 3.0) * f], dtype=torch.float64).to(torch.float32)
    assert torch.equal(g.lr, want) and not bool(s.groups[1].lr.any())  # only the group asked for
    # ... which is not the product of the two fp32 roundings: the pair below differs in the last bit
    lr32, f32 = torch.tensor(1.0 / 3.0, dtype=torch.float32), torch.tensor(f, dtype=torch.float32)
    assert float(lr32 * f32) != float(want[1]) or float(torch.tensor(0.1, dtype=torch.float32) * f32) != float(want[0])


def test_entries_walk_the_heads_in_key_order_weight_before_bias():
    heads = _probe_like()
    s = HeadStore(heads, _init(heads), "cpu")
    entries = list(s.entries())
    assert [(k, p) for k, p, _, _ in entries] == [(k, p) for k in s.keys for p in ("weight", "bias")]
    for k, p, param, mom in entries:
        g = next(g for g in s.groups if k in g.keys)
        i = g.keys.index(k)
        stacked, m_stacked = (g.weight, g.m_weight) if p == "weight" else (g.bias, g.m_bias)
        assert param.data_ptr() == stacked[i].data_ptr() and mom.data_ptr() == m_stacked[i].data_ptr()  # views, not copies
        assert param.shape == mom.shape == stacked[i].shape
    entries[0][2].fill_(7.0)
    entries[1][3].fill_(5.0)
    assert bool((s.groups[0].weight[0] == 7.0).all()) and bool((s.groups[0].m_bias[0] == 5.0).all())
