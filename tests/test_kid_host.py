"""CPU-side checks of the Kernel Inception Distance (vtp_amd/kid.py, csrc/mmd.hip): the restatement tests/mmd_ref.py against numpy and
against a property of the estimator, the oracle's summation table, the subset draws, the argument checks of the C entry points, the
wrappers and the class (refused before any HIP call), GenEval's result keys, and the register budget of the new kernels."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import mmd_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_kid_64_agrees_with_numpy_on_a_tiny_case():
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(7, 8, generator=g), torch.randn(5, 8, generator=g) + 0.5
    a, b = x.double().numpy(), y.double().numpy()
    k = lambda p, q: (p @ q.T / 8 + 1) ** 3
    want = ((k(a, a).sum() - np.trace(k(a, a))) / (7 * 6) + (k(b, b).sum() - np.trace(k(b, b))) / (5 * 4) - 2 * k(a, b).mean())
    got = M.kid_64(x, y)["kid"]
    assert abs(got - want) <= 1e-13 * abs(want) and want > 0
    # other kernel parameters
    k2 = lambda p, q: (p @ q.T * 0.25 + 2) ** 2
    want2 = ((k2(a, a).sum() - np.trace(k2(a, a))) / 42 + (k2(b, b).sum() - np.trace(k2(b, b))) / 20 - 2 * k2(a, b).mean())
    assert abs(M.kid_64(x, y, gamma=0.25, coef0=2.0, degree=2)["kid"] - want2) <= 1e-13 * abs(want2)


def test_a_set_against_its_own_permutation_gives_the_known_value():
    """y = a permutation of x: Sxx = Syy = the off-diagonal sum and Sxy = the whole sum, so MMD^2_u = (2 / m) (mean off-diagonal -
    mean diagonal) -- negative for most sets: the unbiased estimator does not know that the samples are shared"""
    x, _ = M.case(2)
    m = x.shape[0]
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(1))
    k = M.kernel_64(x, x, 1.0 / x.shape[1], 1.0, 3)
    diag = float(k.diagonal().sum())
    off = float(k.sum()) - diag
    want = (2.0 / m) * (off / (m * (m - 1)) - diag / m)
    got = M.kid_64(x, x[perm])["kid"]
    assert abs(got - want) <= 1e-12 * (abs(off) / (m * (m - 1)) + diag / m) and want < 0


def test_the_summation_table_is_a_permutation_and_the_oracle_sums_every_pair_once():
    assert sorted(M.TABLE.flatten().tolist()) == list(range(128)) == M.NATURAL.flatten().tolist()
    assert M.TABLE[0, :5].tolist() == [0, 1, 2, 3, 8] and M.TABLE[1, 0] == 4 and M.TABLE[2, 16] == 96 and M.TABLE[3, 31] == 127
    g = torch.Generator().manual_seed(3)
    S = torch.randn(2, 37, 300, generator=g)
    for base in (-1, 0, 128):
        k = M.pair_values(S, 0.3, 1.0, 3)
        if base >= 0:
            same = (torch.arange(37)[:, None] + base) == (torch.arange(300)[None, :] + 128)
            k = torch.where(same, torch.zeros((), dtype=F64), k)
        for table in (M.NATURAL, M.TABLE):
            part = M.oracle_part(S, 0.3, 1.0, 3, query_base=base, index_base=128, table=table)
            assert part.shape == (2, 3, 37) and part.dtype == F64
            for t in range(3):
                cols = k[..., t * 128:(t + 1) * 128]
                # a sum of at most 128 terms in any order is within 128 u sum |k| of any other
                assert bool(((part[:, t] - cols.sum(-1)).abs() <= 128 * M.U64 * cols.abs().sum(-1)).all()), (base, t)
        rowsum = M.oracle_fold(part)
        assert bool(((rowsum - k.sum(-1)).abs() <= 300 * M.U64 * k.abs().sum(-1)).all())
        total = M.oracle_total(rowsum)
        assert total.shape == (2,) and bool(((total - k.sum((-1, -2))).abs() <= 337 * M.U64 * k.abs().sum((-1, -2))).all())
    # degree 1 with integers: every sum is exact whatever the order, and the excluded pair is missing
    S = torch.arange(130 * 130, dtype=F32).view(130, 130) % 7
    part = M.oracle_part(S, 2.0, 1.0, 1, query_base=0)
    want = (2 * S.double() + 1)
    want.fill_diagonal_(0)
    assert torch.equal(M.oracle_fold(part), want.sum(1)) and float(M.oracle_total(M.oracle_fold(part))) == float(want.sum())
    # the tree: pairs of neighbours, an odd element moves up
    v = torch.tensor([1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53, 2.0 ** -52], dtype=F64)
    assert float(M.oracle_total(v)) == ((1.0 + 2.0 ** -53) + (2.0 ** -53 + 2.0 ** -53)) + 2.0 ** -52 == 1.0 + 2.0 ** -51
    # a NaN pair that is left out does not reach the sum; one that is kept does
    S = torch.zeros(2, 2)
    S[0, 0] = float("nan")
    r = M.oracle_fold(M.oracle_part(S, 1.0, 1.0, 3, query_base=0))
    assert r.tolist() == [1.0, 1.0] and bool(M.oracle_fold(M.oracle_part(S, 1.0, 1.0, 3))[0].isnan())


def test_the_subset_draws_are_a_function_of_the_seed_alone():
    from vtp_amd.kid import subset_tables
    a, b = M.draws(300, 257, 3, 129, 5), M.draws(300, 257, 3, 129, 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], M.draws(300, 257, 3, 129, 6)[0])
    for t, n in zip(a, (300, 257)):
        assert t.shape == (3, 129) and all(len(set(row)) == 129 and max(row) < n for row in t.tolist())  # without replacement
    # the first subsets do not depend on how many follow, and the class draws the same tables
    assert torch.equal(M.draws(300, 257, 1, 129, 5)[0][0], a[0][0])
    tab = subset_tables(300, 257, 3, 129, 5)
    assert tab["real"].dtype == torch.int32 and torch.equal(tab["real"].long(), a[0]) and torch.equal(tab["fake"].long(), a[1])
    # the standard generator: real then fake from one stream
    g = torch.Generator().manual_seed(5)
    assert torch.equal(torch.randperm(300, generator=g)[:129], a[0][0]) and torch.equal(torch.randperm(257, generator=g)[:129], a[1][0])


def test_the_bound_is_small_beside_the_distance_on_every_case():
    """the comparison of the GPU test cannot pass by vacuity: the a-priori bound is below 1 % of |KID| on every case"""
    for i in range(len(M.CASES)):
        kid, bnd = M.case_64(i)
        print(f"KID {M.IDS[i]}: kid_64 = {kid:.6f}, bound = {bnd:.3e} ({bnd / abs(kid):.2e} of |kid|)")
        assert 0 < bnd <= 0.01 * abs(kid)


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(64)
    kp = (ctypes.c_double * 2)(0.5, 1.0)
    kpp = ctypes.cast(kp, ctypes.c_void_p)
    err = lambda: lib.vtp_last_error()
    # Q ldq q_rows qi X ldx x_rows xi query_base index_base B N D P kparams degree part part_bytes stream
    name, ok = b"vtp_mmd_poly_part", [p, 8, 2, None, p, 8, 16, None, 0, 0, 2, 16, 8, 1, kpp, 3, p, 1 << 20, None]
    for i in (0, 4, 14, 16):
        a = list(ok)
        a[i] = None
        assert lib.vtp_mmd_poly_part(*a) == -1 and err().startswith(name) and b"null" in err(), i
    for i, v, msg in ((12, 12, b"D"), (12, 0, b"D"), (10, 0, b"B"), (11, 0, b"N"), (13, 0, b"P"), (13, 65536, b"P"), (1, 4, b"ldq"), (5, 4, b"ldx"),
                      (5, 10, b"ldx"), (15, 0, b"degree"), (15, 9, b"degree"), (8, -2, b"query_base"), (9, -128, b"index_base"),
                      (9, 64, b"index_base"), (9, 129, b"index_base"), (17, 2 * 8 - 1, b"part")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_mmd_poly_part(*a) == -1 and err().startswith(name) and msg in err(), (i, v, err())
    for i in (0, 4):
        a = list(ok)
        a[i] = ctypes.c_void_p(68)
        assert lib.vtp_mmd_poly_part(*a) == -1 and err().startswith(name) and b"aligned" in err(), i
    # a list needs the rows of its matrix; P problems and two tiles size the buffer
    a = list(ok)
    a[3], a[2] = p, 0
    assert lib.vtp_mmd_poly_part(*a) == -1 and err().startswith(name) and b"q_rows" in err()
    a = list(ok)
    a[11], a[13], a[17] = 129, 3, 3 * 2 * 2 * 8 - 1
    assert lib.vtp_mmd_poly_part(*a) == -1 and err().startswith(name) and b"part" in err()
    # fold: part rowsum B tiles P stream; total: rowsum B P total stream
    for args, msg in (((None, p, 2, 1, 1, None), b"null"), ((p, None, 2, 1, 1, None), b"null"), ((p, p, 0, 1, 1, None), b"B"),
                      ((p, p, 2, 0, 1, None), b"tiles"), ((p, p, 2, 1, 0, None), b"P")):
        assert lib.vtp_mmd_fold(*args) == -1 and err().startswith(b"vtp_mmd_fold") and msg in err(), args
    for args, msg in (((None, 2, 1, p, None), b"null"), ((p, 2, 1, None, None), b"null"), ((p, 0, 1, p, None), b"B"),
                      ((p, 2097153, 1, p, None), b"B"), ((p, 2, 0, p, None), b"P")):
        assert lib.vtp_mmd_total(*args) == -1 and err().startswith(b"vtp_mmd_total") and msg in err(), args
    for args in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1 << 20, 1 << 20, 1)):
        assert lib.vtp_mmd_workspace_bytes(*args) == -1 and err().startswith(b"vtp_mmd_workspace_bytes"), args


def test_workspace_bytes_and_wrapper_checks(lib):
    from vtp_amd import ops
    assert ops.mmd_workspace_bytes(67, 129, 3) == 3 * 2 * 67 * 8
    assert ops.mmd_workspace_bytes(1, 1) == 8 and ops.mmd_workspace_bytes(1024, 1 << 16) == 512 * 1024 * 8
    assert ops.mmd_workspace_bytes(1000, 1000, 100) == 100 * 8 * 1000 * 8  # the standard protocol: 6.4 MB
    for args, msg in (((0, 1, 1), "B"), ((1 << 20, 1 << 20, 1), "2 GiB")):
        with pytest.raises(ValueError, match=msg):
            ops.mmd_workspace_bytes(*args)
    q, x = torch.zeros(2, 8), torch.zeros(16, 8)
    part, rowsum, total = torch.zeros(1, 1, 2, dtype=F64), torch.zeros(1, 2, dtype=F64), torch.zeros(1, dtype=F64)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mmd_poly_part(q, x, part, 0.125)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mmd_fold(part, rowsum)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mmd_total(rowsum, total)
    with pytest.raises(ValueError, match="float32"):
        ops.mmd_poly_part(q.double(), x, part, 0.125)
    with pytest.raises(ValueError, match="float64"):
        ops.mmd_poly_part(q, x, part.float(), 0.125)
    with pytest.raises(ValueError, match=r"part must be \[P, 1, 2\]"):
        ops.mmd_poly_part(q, x, torch.zeros(1, 2, 2, dtype=F64), 0.125)
    with pytest.raises(ValueError, match="int32"):
        ops.mmd_poly_part(q, x, part, 0.125, qi=torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="one list per problem"):
        ops.mmd_poly_part(q, x, part, 0.125, xi=torch.zeros(2, 16, dtype=torch.int32))
    with pytest.raises(ValueError, match="unit column stride"):
        ops.mmd_poly_part(q, torch.zeros(8, 16).t(), part, 0.125)
    with pytest.raises(ValueError, match="rowsum must be"):
        ops.mmd_fold(part, torch.zeros(1, 3, dtype=F64))
    with pytest.raises(ValueError, match="total must be"):
        ops.mmd_total(rowsum, torch.zeros(2, dtype=F64))


def test_export_and_constructor_validation():
    import vtp_amd
    from vtp_amd import kid, ops
    assert vtp_amd.KID is kid.KID and ops.MMD_TILE == M.TILE == 128
    for kw, msg in ((dict(subsets=-1), "subsets"), (dict(subset_size=1), "subset_size"), (dict(degree=0), "degree"), (dict(degree=9), "degree"),
                    (dict(chunk_rows=0), "positive"), (dict(query_rows=0), "positive"), (dict(capacity=0), "positive"),
                    (dict(banks=object()), "PrecisionRecall")):
        with pytest.raises(ValueError, match=msg):  # ahead of the GPU check
            kid.KID(**kw)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="MI355X"):
            kid.KID()


def test_result_keys_with_kid_and_their_defaults():
    from vtp_amd.gen_eval import result_keys
    # the defaults leave every key set as it was
    assert result_keys(True, True, True, 5) == ("fid", "sfid", "is", "is_std", "precision", "recall")
    assert result_keys(False, False, False, 0) == ()
    assert result_keys(True, True, True, 5, kid=True) == ("fid", "sfid", "is", "is_std", "precision", "recall", "kid", "kid_std")
    assert result_keys(False, True, False, 5, precision_recall=False, kid=True, kid_subsets=False) == ("fid", "sfid", "kid")
    assert result_keys(False, True, False, 0, kid=True) == ("fid",)  # no real rows: no KID
    assert result_keys(False, False, False, 1, precision_recall=False, kid=True) == ("kid", "kid_std")


def test_mmd_kernels_do_not_spill(lib):
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    obj = os.path.join(ROOT, "vtp_amd", "lib", "mmd.o")
    rows = {name: (vs, scr) for name, vs, _, scr, *_ in sr.report_built(obj)}
    for k in ("vtp::mmd_poly_part_kernel", "vtp::mmd_fold_kernel", "vtp::mmd_total_kernel"):
        hit = [n for n in rows if n.startswith(k + "(")]
        assert hit, f"kernel {k} not in {obj}: {sorted(rows)}"
        assert rows[hit[0]] == (0, 0), f"{k}: {rows[hit[0]]} (spilled VGPRs, scratch bytes)"
    assert len(rows) == 3, sorted(rows)
