"""CPU-side checks of the retrieval evaluation (vtp_amd/retrieval.py, csrc/retrieval.hip): the export, the argument checks of the
class, the wrappers and the C entry points (refused before any HIP call), the two statements of the rank in tests/retrieval_ref.py
against each other and against a case written out by hand, and the register budget of the new kernels."""
import ctypes
import importlib.util
import os

import pytest
import torch

import retrieval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def test_export_and_constructor_validation():
    import vtp_amd
    from vtp_amd import ops, retrieval
    assert vtp_amd.Retrieval is retrieval.Retrieval
    assert ops.RETR_MAX_KS == 8
    assert retrieval.check_ks([1, 5, 10]) == (1, 5, 10) and retrieval.check_ks((1000,)) == (1000,)
    for bad in ((5, 1), (1, 1), (0, 5), (), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="ks"):  # ahead of the GPU check
            retrieval.Retrieval(None, ks=bad)
    for kw in (dict(chunk_rows=0), dict(query_rows=0), dict(capacity=0)):
        with pytest.raises(ValueError, match="positive"):
            retrieval.Retrieval(None, **kw)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            retrieval.Retrieval(None)


def test_cpu_tensors_and_wrong_dtypes_or_shapes_raise():
    from vtp_amd import ops
    q, x = torch.zeros(2, 8), torch.zeros(16, 8)
    ptr, idx = torch.zeros(3, dtype=I32), torch.zeros(4, dtype=I64)
    bs, bj, beats, counts = torch.zeros(2), torch.zeros(2, dtype=I64), torch.zeros(2, dtype=I32), torch.zeros(3, dtype=I64)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.retr_best(q, x, ptr, idx, bs, bj)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.retr_rank(q, x, 0, bs, bj, beats)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.retr_count(beats, (1, 5), counts)
    # dtype and shape come before the device
    with pytest.raises(ValueError, match="float32"):
        ops.retr_best(q.double(), x, ptr, idx, bs, bj)
    with pytest.raises(ValueError, match="float32"):
        ops.retr_rank(q, x.half(), 0, bs, bj, beats)
    with pytest.raises(ValueError, match=r"\[B, D\] and \[N, D\]"):
        ops.retr_rank(q, torch.zeros(16, 16), 0, bs, bj, beats)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.retr_best(q, torch.zeros(8, 16).t(), ptr, idx, bs, bj)
    with pytest.raises(ValueError, match="gt_ptr must be"):
        ops.retr_best(q, x, ptr.long(), idx, bs, bj)
    with pytest.raises(ValueError, match="gt_ptr must be"):
        ops.retr_best(q, x, ptr[:2], idx, bs, bj)
    with pytest.raises(ValueError, match="gt_idx must be"):
        ops.retr_best(q, x, ptr, idx.int(), bs, bj)
    with pytest.raises(ValueError, match="best_j must be"):
        ops.retr_rank(q, x, 0, bs, bj.int(), beats)
    with pytest.raises(ValueError, match="beats must be"):
        ops.retr_rank(q, x, 0, bs, bj, torch.zeros(3, dtype=I32))
    with pytest.raises(ValueError, match="sims_out must be"):
        ops.retr_rank(q, x, 0, bs, bj, beats, sims_out=torch.zeros(2, 15))
    with pytest.raises(ValueError, match="counts must be"):
        ops.retr_count(beats, (1, 5, 10), counts)
    with pytest.raises(ValueError, match="rank holds"):
        ops.retr_count(beats, (1, 5), counts, torch.zeros(3, dtype=I32), 2)
    if torch.cuda.is_available():
        from vtp_amd import Retrieval
        dev = "cuda"
        r = Retrieval(None)
        ids = torch.zeros(4, dtype=I64, device=dev)
        with pytest.raises(ValueError, match="no CPU path"):
            r.add_image_features(torch.zeros(4, 8), ids)
        with pytest.raises(ValueError, match="no CPU path"):
            r.add_image_features(torch.zeros(4, 8, device=dev), ids.cpu())
        with pytest.raises(ValueError, match="multiple of 8"):
            r.add_text_features(torch.zeros(4, 12, device=dev), ids)
        with pytest.raises(ValueError, match="must be 4 integers"):
            r.add_text_features(torch.zeros(4, 8, device=dev), ids[:3])
        with pytest.raises(ValueError, match="must be 4 integers"):
            r.add_text_features(torch.zeros(4, 8, device=dev), ids.float())
        with pytest.raises(RuntimeError, match="without a model"):
            r.add_images(torch.zeros(1, 3, 16, 16, device=dev), ids[:1])
        r.add_image_features(torch.zeros(4, 8, device=dev), ids)
        with pytest.raises(ValueError, match="like the image bank"):
            r.add_text_features(torch.zeros(4, 16, device=dev), ids)
        with pytest.raises(RuntimeError, match="text bank is empty"):
            r.result()
        with pytest.raises(RuntimeError, match="after result"):
            r.ranks("image_to_text")
        with pytest.raises(ValueError, match="direction"):
            r.ranks("text_to_text")


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(64)
    err = lambda: lib.vtp_last_error()
    # best: Q ldq X ldx n_total gt_ptr gt_idx nnz B D best_s best_j stream
    name, ok = b"vtp_retr_best", [p, 8, p, 8, 16, p, p, 4, 2, 8, p, p, None]
    for i in (0, 2, 5, 6, 10, 11):
        a = list(ok)
        a[i] = None
        assert lib.vtp_retr_best(*a) == -1 and err().startswith(name) and b"null" in err(), i
    for i, v, msg in ((9, 12, b"D"), (9, 0, b"D"), (8, 0, b"B"), (4, 0, b"n_total"), (4, 1 << 31, b"n_total"), (1, 4, b"ldq"), (1, 10, b"ldq"),
                      (3, 4, b"ldx"), (3, 10, b"ldx"), (7, -1, b"nnz"), (7, (1 << 31) - 64, b"nnz")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_retr_best(*a) == -1 and err().startswith(name) and msg in err(), (i, v, err())
    for i in (0, 2):
        a = list(ok)
        a[i] = ctypes.c_void_p(68)
        assert lib.vtp_retr_best(*a) == -1 and err().startswith(name) and b"aligned" in err(), i
    # rank: Q ldq X ldx index_base B N D best_s best_j beats splits sims_out lds stream
    name, ok = b"vtp_retr_rank", [p, 8, p, 8, 0, 2, 16, 8, p, p, p, 0, None, 0, None]
    for i in (0, 2, 8, 9, 10):
        a = list(ok)
        a[i] = None
        assert lib.vtp_retr_rank(*a) == -1 and err().startswith(name) and b"null" in err(), i
    for i, v, msg in ((7, 12, b"D"), (7, 0, b"D"), (5, 0, b"B"), (6, 0, b"N"), (1, 4, b"ldq"), (3, 4, b"ldx"), (3, 10, b"ldx"),
                      (11, -1, b"splits"), (11, 1025, b"splits"), (4, -1, b"index_base"), (4, (1 << 31) - 16, b"index_base")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_retr_rank(*a) == -1 and err().startswith(name) and msg in err(), (i, v, err())
    for i in (0, 2):
        a = list(ok)
        a[i] = ctypes.c_void_p(68)
        assert lib.vtp_retr_rank(*a) == -1 and err().startswith(name) and b"aligned" in err(), i
    a = list(ok)
    a[12], a[13] = p, 8  # sims_out given with a row stride below N
    assert lib.vtp_retr_rank(*a) == -1 and err().startswith(name) and b"lds" in err()
    # count: beats B ks nk counts rank rank_offset stream
    ks = (ctypes.c_int * 9)(1, 2, 3, 4, 5, 6, 7, 8, 9)
    kp = ctypes.cast(ks, ctypes.c_void_p)
    name, ok = b"vtp_retr_count", [p, 2, kp, 3, p, None, 0, None]
    for i in (0, 2, 4):
        a = list(ok)
        a[i] = None
        assert lib.vtp_retr_count(*a) == -1 and err().startswith(name) and b"null" in err(), i
    for i, v, msg in ((1, 0, b"B"), (3, 0, b"nk"), (3, 9, b"nk"), (6, -1, b"rank_offset")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_retr_count(*a) == -1 and err().startswith(name) and msg in err(), (i, v, err())
    for bad in ((5, 1, 10), (1, 1, 10), (0, 5, 10), (1, 10, 5)):
        a = list(ok)
        a[2] = ctypes.cast((ctypes.c_int * 3)(*bad), ctypes.c_void_p)
        assert lib.vtp_retr_count(*a) == -1 and err().startswith(name) and b"ascend" in err(), bad


# ---------------------------------------------------------------------------------------------------------------- the restatement
# one query per row: similarities of six gallery rows, its ground-truth rows, and the rank read off by inspection
HAND = [
    ([0.9, 0.5, 0.7, 0.1, 0.3, 0.2], [0], 0),           # the ground truth leads
    ([0.9, 0.5, 0.7, 0.1, 0.3, 0.2], [3], 5),           # it comes last
    ([0.9, 0.5, 0.7, 0.1, 0.3, 0.2], [4, 1, 3], 2),     # several: the best of them (row 1) counts; 0.9 and 0.7 are before it
    ([0.5, 0.5, 0.5, 0.5, 0.5, 0.5], [2], 2),           # all equal: the rows of lower index are before it
    ([0.5, 0.5, 0.5, 0.5, 0.5, 0.5], [4, 2], 2),        # two equal ground-truth rows: the lower index is the best, row 4 is not counted
    ([0.5, 0.7, 0.5, 0.7, 0.5, 0.7], [2, 5], 2),        # rows 1 and 3 are before row 5 (equal, lower index); no ground-truth row counts
    ([0.9, 0.5, 0.7, 0.1, 0.3, 0.2], [], 6),            # no ground truth: the gallery size
    ([0.9, 0.5, 0.7, 0.1, 0.3, 0.2], [-1, 6, 17], 6),   # every index out of range: as none
    ([0.9, 0.5, 0.7, 0.1, 0.3, 0.2], [6, 2, -3], 1),    # out-of-range entries beside a good one are ignored
]


def test_the_two_statements_agree_with_the_hand_written_case():
    S = torch.tensor([h[0] for h in HAND], dtype=F64)
    lists = [h[1] for h in HAND]
    want = torch.tensor([h[2] for h in HAND], dtype=I32)
    bs, bj = R.best_of(S, lists)
    assert bj.tolist() == [0, 3, 1, 2, 2, 5, -1, -1, 2] and bs[6] == R.NEG and bs[2] == 0.5
    assert torch.equal(R.rank_by_count(S, bs, bj), want)
    assert torch.equal(R.rank_by_sort(S, lists), want)
    assert R.counts_of(want, (1, 3, 6)).tolist() == [1, 6, 7, 9]
    s = R.summary(want, (1, 3))
    assert s["R@1"] == 1 / 9 * 100 and s["counts"] == {1: 1, 3: 6} and s["rows"] == 9
    assert s["median_rank"] == 3.0 and s["mean_rank"] == (sum(h[2] for h in HAND) + 9) / 9
    assert R.summary(want[:4], (1,))["median_rank"] == 3.0  # ranks 1 3 3 6 (1-based): the mean of the two in the middle
    # a chunk of the gallery: the best row may lie in another chunk, and the counts of the chunks add up to the rank
    for cuts in ((0, 2, 6), (0, 1, 2, 3, 4, 5, 6), (0, 5, 6)):
        total = sum(R.rank_by_count(S[:, a:b], bs, bj, index_base=a) for a, b in zip(cuts, cuts[1:]))
        assert torch.equal(total.to(I32), want), cuts
    # ... and the best over chunks is the best of the chunks' bests
    b0, j0 = R.best_of(S[:, :3], lists, 0)
    b1, j1 = R.best_of(S[:, 3:], lists, 3)
    assert j0.tolist() == [0, -1, 1, 2, 2, 2, -1, -1, 2] and j1.tolist() == [-1, 3, 4, -1, 4, 5, -1, -1, -1]
    # a NaN is never the best and never counted
    Sn = S.clone()
    Sn[1, 3] = float("nan")
    Sn[0, 2] = float("nan")
    bs, bj = R.best_of(Sn, lists)
    assert bj[1] == -1 and R.rank_by_count(Sn, bs, bj).tolist()[:2] == [0, 6]
    # ids -> lists -> CSR
    q_ids, g_ids = torch.tensor([7, 3, 9, 3]), torch.tensor([3, 7, 3, 5, 7, 3])
    lists = R.gt_lists(q_ids, g_ids)
    assert lists == [[1, 4], [0, 2, 5], [], [0, 2, 5]]
    ptr, idx = R.csr(lists)
    assert ptr.tolist() == [0, 2, 5, 5, 8] and idx.tolist() == [1, 4, 0, 2, 5, 0, 2, 5] and ptr.dtype == I32 and idx.dtype == I64


@pytest.mark.parametrize("B,N,D,seed", [(40, 300, 8, 0), (33, 129, 24, 1), (7, 50, 768, 2)])
def test_the_two_statements_agree_on_random_data_with_ties_and_empty_sets(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = R.dyadic((N, D), g)
    q = R.dyadic((B, D), g)
    x[N // 2] = x[3]   # duplicated gallery rows
    x[N - 1] = x[3]
    q[:3] = x[:3]      # queries that equal gallery rows
    S = R.sims_64(q, x)
    assert torch.equal(S.to(F32).to(F64), S)  # exact in fp32 as well
    lens = [0, 1, 5, 17]
    lists = []
    for b in range(B):
        l = torch.randint(-2, N + 2, (lens[b % 4],), generator=g).tolist()  # out-of-range entries occur
        lists.append(l)
    lists[2] = [N // 2, 3, N - 1]  # a tie between ground-truth rows
    lists[1] = [N - 1]             # rows 3 and N // 2 are equal to it and come first
    bs, bj = R.best_of(S, lists)
    by_count, by_sort = R.rank_by_count(S, bs, bj), R.rank_by_sort(S, lists)
    assert torch.equal(by_count, by_sort)
    assert int(bj[2]) == 3 and int(by_count[0]) == N and bj[0] == -1
    # forced ties matter: somewhere a row of equal similarity and lower index stands before the best ground-truth row
    tied = ((S == bs.to(F64)[:, None]) & (torch.arange(N)[None, :] < bj[:, None])).sum(1)
    assert int(tied.sum()) > 0
    # and the chunked count adds up
    for step in (1, 127, N):
        total = sum(R.rank_by_count(S[:, a:a + step], bs, bj, index_base=a) for a in range(0, N, step))
        assert torch.equal(total.to(I32), by_sort), step


def test_retrieval_kernels_do_not_spill(lib):
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    obj = os.path.join(ROOT, "vtp_amd", "lib", "retrieval.o")
    rows = {name: vs for name, vs, *_ in sr.report_built(obj)}
    for k in ("vtp::retr_best_kernel", "vtp::retr_rank_kernel", "vtp::retr_count_kernel"):
        hit = [n for n in rows if n.startswith(k + "(")]
        assert hit, f"kernel {k} not in {obj}: {sorted(rows)}"
        assert rows[hit[0]] == 0, f"{k}: {rows[hit[0]]} spilled VGPRs"
    assert len(rows) == 3, sorted(rows)
