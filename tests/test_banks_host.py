"""CPU tests of vtp_amd/banks.py, the plumbing the evaluation classes share: the chunk loop, the growable bank, the width rule of a
bank set, the grow-only workspace and the rank-major gather of two gloo ranks (loopback only)."""
import datetime
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def test_spans_cover_the_range_in_order():
    from vtp_amd.banks import spans
    assert list(spans(5, 2)) == [(0, 2), (2, 4), (4, 5)]
    assert list(spans(4, 2)) == [(0, 2), (2, 4)]
    assert list(spans(1, 1 << 20)) == [(0, 1)]
    assert list(spans(0, 3)) == []


def _append(bank, rows, ids):
    dst, col = bank.reserve(*rows.shape)
    dst.copy_(rows)
    col.copy_(ids)


def test_bank_doubles_and_keeps_every_row_and_column_entry():
    from vtp_amd.banks import Bank
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(9, 8, generator=g)
    rows[0, 0], rows[4, 3] = float("nan"), -0.0  # compared as bits below
    ids = torch.randint(-(1 << 62), 1 << 62, (9,), generator=g)
    bank = Bank(CPU, columns={"ids": torch.int64})
    assert (bank.size, bank.capacity, bank.width) == (0, 0, None) and bank.rows.shape[0] == 0 and bank.column("ids").shape == (0,)
    at = 0
    for n, cap in ((3, 4), (1, 4), (5, 16)):
        _append(bank, rows[at:at + n], ids[at:at + n])
        at += n
        assert (bank.size, bank.capacity, bank.width) == (at, cap, 8)
        assert bank.rows.dtype == torch.float32 and bank.rows.shape == (at, 8)
        assert torch.equal(bank.rows.view(torch.int32), rows[:at].view(torch.int32))
        assert bank.column("ids").dtype == torch.int64 and torch.equal(bank.column("ids"), ids[:at])
    with pytest.raises(ValueError, match="like the bank"):
        bank.reserve(1, 16)
    assert bank.size == 9

    fixed = Bank(CPU, capacity=4096, columns={"labels": torch.int32})
    for n in (1000, 3000, 96):
        dst, lab = fixed.reserve(n, 8)
        assert dst.shape == (n, 8) and lab.shape == (n,) and lab.dtype == torch.int32 and fixed.capacity == 4096
    assert fixed.size == 4096
    fixed.reserve(1, 8)
    assert (fixed.size, fixed.capacity) == (4097, 8192)


def test_bank_clear_keeps_the_storage():
    from vtp_amd.banks import Bank
    bank = Bank(CPU, capacity=4)
    (dst,) = bank.reserve(3, 8)
    dst.fill_(1.0)
    ptr = bank.rows.data_ptr()
    bank.clear()
    assert (bank.size, bank.capacity, bank.width) == (0, 4, None) and bank.rows.shape == (0, 8)
    (dst,) = bank.reserve(2, 8)
    assert dst.data_ptr() == ptr and (bank.size, bank.capacity) == (2, 4)


def _reserve(banks, name, n, D, what="rows"):
    """what an owner does with a batch: the width rule of the set, then the room in one bank"""
    banks.check_width((n, D), what)
    return banks[name].reserve(n, D)


def test_bank_set_refuses_a_second_width():
    from vtp_amd.banks import BankSet
    banks = BankSet(("real", "fake"), CPU)
    _reserve(banks, "real", 4, 8, "fake features")[0].zero_()
    with pytest.raises(ValueError, match=r"fake features must be \[n, 8\] like the real bank, got \(4, 16\)"):
        _reserve(banks, "fake", 4, 16, "fake features")
    assert banks["fake"].size == 0 and banks["fake"].capacity == 0
    _reserve(banks, "fake", 2, 8, "fake features")[0].zero_()
    with pytest.raises(ValueError, match="like the real bank"):
        _reserve(banks, "real", 1, 24, "real features")
    banks.clear()  # no rows, no width: the next rows decide again
    _reserve(banks, "fake", 1, 16, "fake features")
    with pytest.raises(ValueError, match="like the fake bank"):
        _reserve(banks, "real", 1, 8, "real features")
    with pytest.raises(ValueError, match="no CPU path"):  # append() takes a batch through feature_rows first
        banks.append("fake", torch.zeros(1, 16), "fake features")


def test_workspace_grows_and_never_shrinks():
    from vtp_amd.banks import Workspace
    ws = Workspace(CPU)
    a = ws.at_least(100)
    assert a.dtype == torch.uint8 and a.numel() == 100
    assert ws.at_least(100) is a and ws.at_least(7) is a and ws.at_least(0) is a
    b = ws.at_least(101)
    assert b.numel() == 101 and b is not a
    assert ws.at_least(1) is b


def test_feature_rows_and_the_device_have_no_cpu_path():
    from vtp_amd.banks import eval_device, feature_rows
    with pytest.raises(ValueError, match="rows must live on the MI355X .* no CPU path"):
        feature_rows(torch.zeros(4, 8), "rows")
    with pytest.raises(ValueError, match="no CPU path"):
        feature_rows([[0.0] * 8], "rows")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=r"vtp_amd\.Knn runs on the MI355X kernels only \(no CPU fallback\)"):
            eval_device("Knn")
    else:
        assert eval_device("Knn").type == "cuda"
        with pytest.raises(RuntimeError, match=r"vtp_amd\.Knn .* the model / device must be cuda \(no CPU fallback\)"):
            eval_device("Knn", device="cpu")
        with pytest.raises(RuntimeError, match="must be cuda"):
            eval_device("Knn", model=torch.nn.Linear(2, 2))


def test_a_group_of_one_sums_and_gathers_nothing():
    from vtp_amd.banks import BankSet, Group
    one = Group(None)
    t = torch.arange(3)
    assert (one.world, one.rank) == (1, 0) and one.summed(t) is t
    banks = BankSet(("image", "text"), CPU, columns={"ids": torch.int64})
    assert banks.gathered(one)[2] == {"image": 0, "text": 0}
    rows, ids = _reserve(banks, "text", 2, 8)
    rows.fill_(2.0)
    ids.copy_(torch.tensor([5, 6]))
    rows, columns, totals = banks.gathered(one)
    assert totals == {"image": 0, "text": 2}
    assert rows["text"].data_ptr() == banks["text"].rows.data_ptr() and columns["text"]["ids"].tolist() == [5, 6]


# ---------------------------------------------------------------------------------------------------------------- two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SHARDS = {"image": (3, 0), "text": (2, 5)}  # rows per rank: rank 1 holds an empty image bank


def _shard(name, rank, D=8):
    """rows and ids of one rank's shard, a function of (bank, rank, row, column) alone"""
    n = SHARDS[name][rank]
    base = (1000 if name == "text" else 0) + 100 * rank
    rows = (torch.arange(n * D, dtype=torch.float32).view(n, D) + base) / 7
    return rows, torch.arange(n, dtype=torch.int64) + base - (1 << 40)


def _fill(banks, name, rows, ids):
    dst, col = _reserve(banks, name, *rows.shape)
    dst.copy_(rows)
    col.copy_(ids)


def _gather_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from vtp_amd.banks import BankSet, Group
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))  # a rank that misses a collective fails, it does not hang
    group = Group(dist.group.WORLD)
    res = {"world": group.world, "rank": group.rank}
    t = torch.tensor([rank + 1, 10])
    res["summed"], res["kept"] = group.summed(t), t

    def make():
        return BankSet(("image", "text"), CPU, columns={"ids": torch.int64})

    # uneven shards, one of them empty
    banks = make()
    for name in SHARDS:
        if SHARDS[name][rank]:
            _fill(banks, name, *_shard(name, rank))
    res["uneven"] = banks.gathered(group)
    # the widths differ: every rank hears of it
    banks = make()
    _fill(banks, "image", torch.zeros(2, 8 * (rank + 1)), torch.zeros(2, dtype=torch.int64))
    try:
        banks.gathered(group)
        res["widths"] = "no error"
    except ValueError as e:
        res["widths"] = str(e)
    # nothing anywhere: zero totals, for the owner to refuse in its own words
    res["nothing"] = make().gathered(group)
    # rank 1 added nothing at all and knows no width: it still takes part in every collective
    banks = make()
    if rank == 0:
        for name in SHARDS:
            _fill(banks, name, *_shard(name, 0))
    res["one_sided"] = banks.gathered(group)
    out[rank] = res
    dist.destroy_process_group()


def test_two_gloo_ranks_gather_rank_major():
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_gather_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    for r in range(world):
        res = out[r]
        assert (res["world"], res["rank"]) == (2, r)
        assert res["summed"].tolist() == [3, 20] and res["kept"].tolist() == [r + 1, 10]  # summed() leaves its argument alone
        rows, columns, totals = res["uneven"]
        assert totals == {"image": 3, "text": 7}
        for name in SHARDS:
            want_rows, want_ids = zip(*(_shard(name, k) for k in range(world)))
            assert rows[name].dtype == torch.float32 and torch.equal(rows[name], torch.cat(want_rows)), (r, name)
            assert columns[name]["ids"].dtype == torch.int64 and torch.equal(columns[name]["ids"], torch.cat(want_ids)), (r, name)
        assert "different widths: [8, 16]" in res["widths"], r
        assert res["nothing"] == ({}, {}, {"image": 0, "text": 0})
        rows, columns, totals = res["one_sided"]
        assert totals == {"image": 3, "text": 2}
        for name in SHARDS:
            want_rows, want_ids = _shard(name, 0)
            assert torch.equal(rows[name], want_rows) and torch.equal(columns[name]["ids"], want_ids), (r, name)
