"""CPU-side checks of the k-NN evaluation (vtp_amd/knn.py, csrc/knn.hip): the export, the argument checks of the class, the wrappers
and the C entry points (refused before any HIP call), the fp64 restatement tests/knn_ref.py against a brute-force evaluation of a
case written out by hand, and the register budget of the new kernels."""
import ctypes
import importlib.util
import math
import os

import pytest
import torch

import knn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def test_export_and_constructor_validation():
    import vtp_amd
    from vtp_amd import knn
    assert vtp_amd.Knn is knn.Knn
    assert knn.check_ks([10, 20, 100, 200]) == (10, 20, 100, 200) and knn.check_ks((256,)) == (256,)
    for bad in ((20, 10), (10, 10), (0, 5), (10, 257), (), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="ks"):
            knn.Knn(None, ks=bad)
    with pytest.raises(ValueError, match="at least 5 classes"):
        knn.Knn(None, num_classes=4)
    with pytest.raises(ValueError, match="temperature"):
        knn.Knn(None, temperature=0.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            knn.Knn(None)


def test_cpu_tensors_raise():
    from vtp_amd import ops
    q, x = torch.zeros(2, 8), torch.zeros(16, 8)
    sims, idx, ws = torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int64), torch.zeros(1024, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.knn_topk(q, x, 0, 4, sims, idx, ws)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.knn_vote(sims, idx, torch.zeros(16, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), (1, 4), 1 / 0.07, 5,
                     torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="float32"):
        ops.knn_topk(q.double(), x, 0, 4, sims, idx, ws)
    if torch.cuda.is_available():
        from vtp_amd import Knn
        knn = Knn(None, num_classes=5, ks=(1, 2))
        with pytest.raises(ValueError, match="no CPU path"):
            knn.add_bank_features(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="without a model"):
            knn.add_bank(torch.zeros(1, 3, 16, 16, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(64)
    err = lambda: lib.vtp_last_error()
    # topk: Q ldq X ldx index_base B N D K sims idx workspace workspace_bytes splits sims_out lds stream
    ok = [p, 8, p, 8, 0, 2, 16, 8, 4, p, p, p, 1 << 20, 0, None, 0, None]
    for i in (0, 2, 9, 10, 11):
        a = list(ok)
        a[i] = None
        assert lib.vtp_knn_topk(*a) == -1 and b"null" in err(), i
    for i, v, msg in ((7, 12, b"D"), (7, 0, b"D"), (8, 0, b"K"), (8, 257, b"K"), (5, 0, b"B"), (6, 0, b"N"), (1, 4, b"ldq"), (3, 10, b"ldx"),
                      (13, -1, b"splits"), (13, 1025, b"splits"), (4, -1, b"index_base"), (12, 8, b"workspace")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_knn_topk(*a) == -1 and msg in err(), (i, v, err())
    for i in (0, 2, 11):
        a = list(ok)
        a[i] = ctypes.c_void_p(68)
        assert lib.vtp_knn_topk(*a) == -1 and b"aligned" in err(), i
    a = list(ok)
    a[14], a[15] = p, 8  # sims_out given with a row stride below N
    assert lib.vtp_knn_topk(*a) == -1 and b"lds" in err()
    # vote: sims idx labels n_total targets ks nk inv_T num_classes B K counts rank_out pred_out stream
    ks = (ctypes.c_int * 2)(2, 4)
    kp = ctypes.cast(ks, ctypes.c_void_p)
    ok = [p, p, p, 16, p, kp, 2, 1 / 0.07, 5, 2, 4, p, None, None, None]
    for i in (0, 1, 2, 4, 5):
        a = list(ok)
        a[i] = None
        assert lib.vtp_knn_vote(*a) == -1 and b"null" in err(), i
    for i, v, msg in ((6, 0, b"nk"), (6, 9, b"nk"), (8, 4, b"num_classes"), (9, 0, b"B"), (10, 0, b"K"), (10, 257, b"K"), (10, 3, b"ks"),
                      (3, 0, b"n_total")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_knn_vote(*a) == -1 and msg in err(), (i, v, err())
    for bad in ((4, 2), (2, 2), (0, 4)):
        a = list(ok)
        a[5] = ctypes.cast((ctypes.c_int * 2)(*bad), ctypes.c_void_p)
        assert lib.vtp_knn_vote(*a) == -1 and b"ks must ascend" in err(), bad


def test_workspace_bytes(lib):
    from vtp_amd import ops
    assert ops.knn_workspace_bytes(67, 200, 3) == 3 * 67 * 200 * 12
    assert ops.knn_workspace_bytes(1, 1, 1) == 12
    # splits = 0: room for whatever the heuristic may pick at this B -- at least one split, never less than a forced single one
    assert ops.knn_workspace_bytes(256, 200, 0) >= ops.knn_workspace_bytes(256, 200, 1)
    assert ops.knn_workspace_bytes(256, 200, 0) % (256 * 200 * 12) == 0
    for args, msg in (((0, 4, 1), "B"), ((4, 0, 1), "K"), ((4, 257, 1), "K"), ((4, 4, 1025), "splits"), ((1 << 20, 256, 1024), "2 GiB")):
        with pytest.raises(ValueError, match=msg):
            ops.knn_workspace_bytes(*args)


# ---------------------------------------------------------------------------------------------------------------- the restatement
T, C, KS = 0.07, 6, (2, 4)
# six queries written out by hand: (similarities of the 4 neighbours, their labels, target)
HAND = [
    ([0.9, 0.8, 0.7, 0.6], [1, 1, 2, 3], 1),      # the target's class leads at both k
    ([0.9, 0.8, 0.7, 0.6], [2, 2, 4, 4], 3),      # a target without a neighbour: behind 2 and 4, and behind 0 and 1 (score 0, lower index)
    ([0.9, 0.8, 0.7, 0.6], [2, 2, 4, 4], 5),      # as above, one place too far for top-5 at k = 4
    ([0.5, 0.5, 0.25, 0.25], [4, 2, 4, 2], 4),    # an exact score tie at both k: class 2 before class 4
    ([0.9, 0.8, 0.7, 0.6], [0, 1, 2, 3], -1),     # targets outside [0, C): a miss at every k
    ([0.9, 0.8, 0.7, 0.6], [0, 1, 2, 3], C),
]


def brute(sims, labels, target, k):
    """dense fp64: every class has a score, the ranking is a sort"""
    score = [0.0] * C
    for j in range(k):
        score[labels[j]] += math.exp((sims[j] - sims[0]) / T)
    order = sorted(range(C), key=lambda c: (-score[c], c))
    return (order.index(target) if 0 <= target < C else C), order[:5], score


def test_knn_ref_agrees_with_brute_force_on_the_hand_written_case():
    sims = torch.tensor([h[0] for h in HAND], dtype=torch.float64)
    labels = torch.tensor([h[1] for h in HAND])
    targets = torch.tensor([h[2] for h in HAND])
    rank, pred, gap1, gap5 = R.vote(sims, labels, targets, KS, T, C)
    for b, (s, l, t) in enumerate(HAND):
        for m, k in enumerate(KS):
            r, p, score = brute(s, l, t, k)
            assert int(rank[b, m]) == r and pred[b, m].tolist() == p, (b, k, rank[b, m], r, pred[b, m], p)
            top = sorted(score, reverse=True)
            assert gap1[b, m].tolist() == top[:2] and gap5[b, m].tolist() == top[4:6], (b, k)
    # what the cases are there for, written out: the zero-score rule and the tie
    # (classes seen and positive) + target - (those of them below the target), at k = 2 and k = 4
    assert rank[1].tolist() == [1 + 3 - 1, 2 + 3 - 1] and rank[2].tolist() == [1 + 5 - 1, 2 + 5 - 2]
    assert rank[3].tolist() == [1, 1] and pred[3, 1, :2].tolist() == [2, 4] and bool(R.close(gap1[3]).all())
    assert not bool(R.close(gap5[1]).any())  # two zeros are ordered by index, exactly: not a near-tie
    assert rank[4].tolist() == [C, C] and rank[5].tolist() == [C, C]
    assert R.counts_of(rank).tolist() == [[1, 3, 6], [1, 3, 6]]
    # the order of the neighbours: a stable sort by -s
    S = torch.tensor([[0.5, 0.75, 0.5, 0.75, 0.25], [0.0, 0.0, 0.0, 0.0, 0.0]])
    s, i = R.neighbours(S, 3, index_base=10)
    assert i.tolist() == [[11, 13, 10], [10, 11, 12]] and s.tolist() == [[0.75, 0.75, 0.5], [0.0, 0.0, 0.0]]


def test_knn_kernels_do_not_spill(lib):
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    obj = os.path.join(ROOT, "vtp_amd", "lib", "knn.o")
    rows = {name: vs for name, vs, *_ in sr.report_built(obj)}
    for k in ("vtp::knn_topk_kernel", "vtp::knn_merge_kernel", "vtp::knn_vote_kernel"):
        hit = [n for n in rows if n.startswith(k + "(")]
        assert hit, f"kernel {k} not in {obj}: {sorted(rows)}"
        assert rows[hit[0]] == 0, f"{k}: {rows[hit[0]]} spilled VGPRs"
    assert len(rows) == 3, sorted(rows)
