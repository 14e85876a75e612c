"""CPU-side checks of the precision / recall evaluation (vtp_amd/precision_recall.py, csrc/precision_recall.hip): the export, the
argument checks of the class, the wrappers and the C entry points (refused before any HIP call), the workspace formula, the
restatement tests/pr_ref.py against a 2-D case written out by hand and against the recorded table of the test cases, and the
register budget of the new kernels."""
import ctypes
import importlib.util
import os

import pytest
import torch

import pr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def test_export_and_constructor_validation():
    import vtp_amd
    from vtp_amd import ops, precision_recall
    assert vtp_amd.PrecisionRecall is precision_recall.PrecisionRecall
    assert ops.PR_MAX_K == 8 == R.MAX_K
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="k must be"):  # ahead of the GPU check
            precision_recall.PrecisionRecall(k=bad)
    for kw in (dict(chunk_rows=0), dict(query_rows=0), dict(capacity=0)):
        with pytest.raises(ValueError, match="positive"):
            precision_recall.PrecisionRecall(**kw)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="MI355X"):
            precision_recall.PrecisionRecall()


def test_cpu_tensors_and_wrong_dtypes_or_shapes_raise():
    from vtp_amd import ops
    q, x = torch.zeros(2, 8), torch.zeros(16, 8)
    qn, xn, r2 = torch.zeros(2), torch.zeros(16), torch.zeros(16)
    dist, ws, hits = torch.zeros(2, 8), torch.zeros(1024, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.pr_sqnorm(x, xn)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.pr_knn_dist(q, qn, x, xn, dist, ws)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.pr_cover(q, qn, x, xn, r2, hits)
    # dtype and shape come before the device
    with pytest.raises(ValueError, match="float32"):
        ops.pr_sqnorm(x.double(), xn)
    with pytest.raises(ValueError, match="float32"):
        ops.pr_knn_dist(q.double(), qn, x, xn, dist, ws)
    with pytest.raises(ValueError, match="float32"):
        ops.pr_cover(q, qn, x.half(), xn, r2, hits)
    with pytest.raises(ValueError, match="int32"):
        ops.pr_cover(q, qn, x, xn, r2, hits.long())
    with pytest.raises(ValueError, match="uint8"):
        ops.pr_knn_dist(q, qn, x, xn, dist, ws.float())
    with pytest.raises(ValueError, match="out must be"):
        ops.pr_sqnorm(x, qn)
    with pytest.raises(ValueError, match=r"\[B, D\] and \[N, D\]"):
        ops.pr_knn_dist(q, qn, torch.zeros(16, 16), xn, dist, ws)
    with pytest.raises(ValueError, match="dist must be"):
        ops.pr_knn_dist(q, qn, x, xn, torch.zeros(2, 4), ws)
    with pytest.raises(ValueError, match="xn must be"):
        ops.pr_knn_dist(q, qn, x, qn, dist, ws)
    with pytest.raises(ValueError, match="d2_out must be"):
        ops.pr_knn_dist(q, qn, x, xn, dist, ws, d2_out=torch.zeros(2, 15))
    with pytest.raises(ValueError, match="unit column stride"):
        ops.pr_cover(q, qn, torch.zeros(8, 16).t(), xn, r2, hits)
    with pytest.raises(ValueError, match="r2 must be"):
        ops.pr_cover(q, qn, x, xn, qn, hits)
    with pytest.raises(ValueError, match="hits must be"):
        ops.pr_cover(q, qn, x, xn, r2, torch.zeros(3, dtype=torch.int32))
    if torch.cuda.is_available():
        from vtp_amd import PrecisionRecall
        pr = PrecisionRecall(k=1)
        with pytest.raises(ValueError, match="no CPU path"):
            pr.add_real_features(torch.zeros(4, 8))
        with pytest.raises(ValueError, match="multiple of 8"):
            pr.add_fake_features(torch.zeros(4, 12, device="cuda"))
        pr.add_real_features(torch.zeros(4, 8, device="cuda"))
        with pytest.raises(ValueError, match="like the real bank"):
            pr.add_fake_features(torch.zeros(4, 16, device="cuda"))
        pr.add_fake_features(torch.zeros(1, 8, device="cuda"))
        with pytest.raises(RuntimeError, match="fewer than k \\+ 1"):
            pr.result()
        with pytest.raises(RuntimeError, match="after result"):
            pr.radii("real")


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(64)
    err = lambda: lib.vtp_last_error()
    # sqnorm: X ldx N D out stream
    name, ok = b"vtp_pr_sqnorm", [p, 8, 16, 8, p, None]
    for i in (0, 4):
        a = list(ok)
        a[i] = None
        assert lib.vtp_pr_sqnorm(*a) == -1 and err().startswith(name) and b"null" in err(), i
    for i, v, msg in ((3, 12, b"D"), (3, 0, b"D"), (2, 0, b"N"), (1, 4, b"ldx"), (1, 10, b"ldx")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_pr_sqnorm(*a) == -1 and err().startswith(name) and msg in err(), (i, v, err())
    a = list(ok)
    a[0] = ctypes.c_void_p(68)
    assert lib.vtp_pr_sqnorm(*a) == -1 and err().startswith(name) and b"aligned" in err()
    # knn_dist: Q ldq qn X ldx xn query_base index_base B N D dist workspace workspace_bytes splits d2_out ldo stream
    name, ok = b"vtp_pr_knn_dist", [p, 8, p, p, 8, p, 0, 0, 2, 16, 8, p, p, 1 << 20, 0, None, 0, None]
    for i in (0, 2, 3, 5, 11, 12):
        a = list(ok)
        a[i] = None
        assert lib.vtp_pr_knn_dist(*a) == -1 and err().startswith(name) and b"null" in err(), i
    for i, v, msg in ((10, 12, b"D"), (10, 0, b"D"), (8, 0, b"B"), (9, 0, b"N"), (1, 4, b"ldq"), (4, 4, b"ldx"), (4, 10, b"ldx"),
                      (14, -1, b"splits"), (14, 1025, b"splits"), (6, -2, b"query_base"), (7, -1, b"index_base"), (13, 8, b"workspace"),
                      (13, 63, b"workspace")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_pr_knn_dist(*a) == -1 and err().startswith(name) and msg in err(), (i, v, err())
    a = list(ok)
    a[14], a[13] = 3, 3 * 2 * 32 - 1  # a forced split count sizes the workspace
    assert lib.vtp_pr_knn_dist(*a) == -1 and err().startswith(name) and b"workspace" in err()
    for i in (0, 3, 11, 12):
        a = list(ok)
        a[i] = ctypes.c_void_p(68)
        assert lib.vtp_pr_knn_dist(*a) == -1 and err().startswith(name) and b"aligned" in err(), i
    a = list(ok)
    a[15], a[16] = p, 8  # d2_out given with a row stride below N
    assert lib.vtp_pr_knn_dist(*a) == -1 and err().startswith(name) and b"ldo" in err()
    # cover: Q ldq qn X ldx xn r2 B N D hits splits stream
    name, ok = b"vtp_pr_cover", [p, 8, p, p, 8, p, p, 2, 16, 8, p, 0, None]
    for i in (0, 2, 3, 5, 6, 10):
        a = list(ok)
        a[i] = None
        assert lib.vtp_pr_cover(*a) == -1 and err().startswith(name) and b"null" in err(), i
    for i, v, msg in ((9, 12, b"D"), (9, 0, b"D"), (7, 0, b"B"), (8, 0, b"N"), (1, 4, b"ldq"), (4, 4, b"ldx"), (11, -1, b"splits"),
                      (11, 1025, b"splits")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_pr_cover(*a) == -1 and err().startswith(name) and msg in err(), (i, v, err())
    for i in (0, 3):
        a = list(ok)
        a[i] = ctypes.c_void_p(68)
        assert lib.vtp_pr_cover(*a) == -1 and err().startswith(name) and b"aligned" in err(), i
    # workspace_bytes: B splits
    for args in ((0, 1), (4, -1), (4, 1025)):
        assert lib.vtp_pr_workspace_bytes(*args) == -1 and err().startswith(b"vtp_pr_workspace_bytes"), args


def test_workspace_bytes(lib):
    from vtp_amd import ops
    # splits * B * 8 floats
    assert ops.pr_workspace_bytes(67, 3) == 3 * 67 * 8 * 4 == 6432
    assert ops.pr_workspace_bytes(1, 1) == 32
    # splits = 0: room for whatever the heuristic may pick at this B: ceil(512 / row blocks of 128), at most 256
    assert ops.pr_workspace_bytes(1024, 0) == 64 * 1024 * 32
    assert ops.pr_workspace_bytes(100, 0) == 256 * 100 * 32
    for args, msg in (((0, 1), "B"), ((4, 1025), "splits"), ((1 << 20, 1024), "2 GiB")):
        with pytest.raises(ValueError, match=msg):
            ops.pr_workspace_bytes(*args)


# ---------------------------------------------------------------------------------------------------------------- the restatement
# a 2-D case whose every number is written out by inspection (integer coordinates: every distance is exact)
REAL = [(0, 0), (0, 0), (3, 0), (3, 4), (10, 0), (10, 1), (-30, 0)]  # rows 0 and 1 are an exact duplicate pair
FAKE = [(0, 0), (3, 2), (10, 2), (20, 20), (6, 0), (20, 21)]
# k = 1: the squared distance to the nearest OTHER row.  Rows 0 / 1 find each other at 0; (3, 0) finds the pair at 9; (3, 4) finds
# (3, 0) at 16; (10, 0) and (10, 1) each other at 1; (-30, 0) the pair at 900
REAL_R1 = [0, 0, 9, 16, 1, 1, 900]
# k = 2: (3, 0) sees BOTH duplicates at 9, so its second neighbour is at 9 as well
REAL_R2 = [9, 9, 9, 25, 49, 50, 900]
FAKE_R1 = [13, 13, 20, 1, 13, 1]
# generated row against the real balls (k = 1):
#   (0, 0): the pair at 0 <= 0 (two hits), (3, 0) at 9 <= 9 and (-30, 0) at 900 <= 900 (both on the boundary); (3, 4) at 25 > 16
#   (3, 2): (3, 0) at 4 <= 9, (3, 4) at 4 <= 16; the pair at 13 > 0
#   (10, 2): (10, 1) at 1 <= 1 (boundary); (10, 0) at 4 > 1
#   (6, 0): (3, 0) at 9 <= 9 (boundary); (10, 0) at 16 > 1, (3, 4) at 25 > 16
HITS_FAKE = [4, 2, 1, 0, 1, 0]
# real row against the generated balls (k = 1):
#   (0, 0) twice: (0, 0) at 0 <= 13, (3, 2) at 13 <= 13 (boundary); (6, 0) at 36 > 13
#   (3, 0): (0, 0) at 9, (3, 2) at 4, (6, 0) at 9, all <= 13; (10, 2) at 53 > 20
#   (3, 4): (3, 2) at 4; (0, 0) and (6, 0) at 25 > 13
#   (10, 0): (10, 2) at 4 <= 20; (6, 0) at 16 > 13
#   (10, 1): (10, 2) at 1 <= 20; (6, 0) at 17 > 13
#   (-30, 0): (0, 0) at 900 > 13
HITS_REAL = [2, 2, 3, 1, 1, 1, 0]


def test_pr_ref_agrees_with_the_hand_written_case():
    real, fake = torch.tensor(REAL, dtype=F32), torch.tensor(FAKE, dtype=F32)
    assert R.radii_64(real, 1).tolist() == REAL_R1 and R.radii_64(real, 2).tolist() == REAL_R2
    assert R.radii_64(fake, 1).tolist() == FAKE_R1
    out = R.pr_64(real, fake, 1)
    assert out["hits_fake"].tolist() == HITS_FAKE and out["hits_real"].tolist() == HITS_REAL
    assert out["counts"] == (4, 2, 6, 1) and out["precision"] == 4 / 6 and out["recall"] == 6 / 7
    # a radius of 0 is hit by an exact duplicate alone
    assert R.hits_64(fake, real[:2], torch.zeros(2)).tolist() == [2, 0, 0, 0, 0, 0]
    # fewer than k other rows: the radius is infinite
    assert R.radii_64(real[:2], 2).tolist() == [INF, INF] and R.radii_64(real[:2], 1).tolist() == [0, 0]
    # the fp32 oracle on exact data equals fp64, and its lists are the sorted rows with the excluded pair left out by index
    d2 = R.oracle32(real @ real.T, (real * real).sum(1), (real * real).sum(1))
    assert torch.equal(d2.to(F64), R.d2_64(real, real))
    lists = R.lists32(d2, query_base=0)
    assert lists[2].tolist() == [9, 9, 16, 49, 50, 1089, INF, INF] and lists[0].tolist() == [0, 9, 25, 100, 101, 900, INF, INF]
    assert R.lists32(d2)[0].tolist()[:3] == [0, 0, 9]
    # the excluded pair follows the bases: rows 2 .. 4 as queries against the bank from row 1 on
    part = R.lists32(d2[2:5, 1:], query_base=2, index_base=1)
    assert part[0].tolist()[:3] == [9, 16, 49] and part[2].tolist()[:2] == [1, 49]
    assert torch.equal(R.kth_other(d2.to(F64), 1), R.radii_64(real, 1))
    assert R.hits32(R.oracle32(fake @ real.T, (fake * fake).sum(1), (real * real).sum(1)), torch.tensor(REAL_R1, dtype=F32)).tolist() == HITS_FAKE
    # negatives become 0 and a NaN stays a NaN
    z = R.oracle32(torch.tensor([[2.0, float("nan")]]), torch.tensor([1.0]), torch.tensor([1.0, 1.0]))
    assert z[0, 0] == 0 and bool(z[0, 1].isnan())


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_cases_reproduce_the_recorded_table_and_keep_the_floor(i):
    """the generators and the fp64 restatement give the recorded counts, and every decision compared leaves FLOOR rows on each side"""
    for k, want in R.TABLE[i].items():
        got = R.case_64(i, k)["counts"]
        assert got == want, (k, got, want)
        assert min(got) >= R.FLOOR
    assert set(R.ks_of(i)) >= {1, 3}
    real, fake = R.case(i)
    assert (real.shape[0], fake.shape[0], real.shape[1]) == R.CASES[i][1][:3] and real.dtype == F32


def test_pr_kernels_do_not_spill(lib):
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    obj = os.path.join(ROOT, "vtp_amd", "lib", "precision_recall.o")
    rows = {name: vs for name, vs, *_ in sr.report_built(obj)}
    for k in ("vtp::pr_knn_kernel", "vtp::pr_cover_kernel", "vtp::pr_fold_kernel", "vtp::pr_sqnorm_kernel"):
        hit = [n for n in rows if n.startswith(k + "(")]
        assert hit, f"kernel {k} not in {obj}: {sorted(rows)}"
        assert rows[hit[0]] == 0, f"{k}: {rows[hit[0]]} spilled VGPRs"
    assert len(rows) == 4, sorted(rows)
