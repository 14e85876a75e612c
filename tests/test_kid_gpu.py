"""GPU: the Kernel Inception Distance kernels (csrc/mmd.hip: vtp_mmd_poly_part / vtp_mmd_fold / vtp_mmd_total), vtp_amd.KID and
GenEval(kid=...).

part, rowsum and total are compared with EQUALITY of bits.  The oracle is tests/mmd_ref.py::oracle_part: the pair value in torch fp64
on the host from the fp32 products that ops.gemm_nt_f32 formed (pr_ref.gemm_parts), summed in the order the kernel's header states.
Against the fp64 restatement kid_64 the distance is held to the a-priori bound of mmd_ref.bound, which tests/test_kid_host.py shows
to be below 1 % of |KID| on every case (asserted here again).  The ratio |kid - kid_64| / bound is printed for the kernels and for
the oracle (built from the GEMM products, not from the kernels under test)."""
import functools
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

import mmd_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
NAN = float("nan")
NCASE = len(M.CASES)
SETS = ("real", "fake")
PASSES = (("real", "real"), ("fake", "fake"), ("real", "fake"))


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.contiguous().view(I64 if t.dtype == F64 else I32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def sliced(x, pad=8, off=4):
    """x on the GPU as a column slice (offset `off`, row stride D + pad) of a wider NaN-poisoned matrix"""
    wide = torch.full((x.shape[0], x.shape[1] + pad), NAN, dtype=F32)
    wide[:, off:off + x.shape[1]] = x
    return wide.to(DEV)[:, off:off + x.shape[1]]


def sets_of(i):
    return dict(zip(SETS, M.case(i)))


@functools.lru_cache(maxsize=None)
def products(i, qs, xs):
    """S f32 [B, N] on the CPU: the products of case i's set qs with its set xs, formed once by ops.gemm_nt_f32"""
    s = sets_of(i)
    return M.gemm_parts(s[qs], s[xs])[0]


@functools.lru_cache(maxsize=None)
def on_device(i, s):
    return sets_of(i)[s].to(DEV)


def gamma_of(i):
    return 1.0 / M.CASES[i][1][2]


def run(q, x, P, B, N, gamma, degree=3, query_base=-1, index_base=0, qi=None, xi=None, rowsum=None):
    """one chunk through the three kernels -> (part, rowsum, total) on the CPU; the buffers are NaN-poisoned past their ends"""
    from vtp_amd import ops
    tiles = (N + 127) // 128
    buf = torch.full((P * tiles * B + 3,), NAN, device=DEV, dtype=F64)
    part = buf[:P * tiles * B].view(P, tiles, B)
    ops.mmd_poly_part(q, x, part, gamma, 1.0, degree, query_base=query_base, index_base=index_base, qi=qi, xi=xi)
    rowsum = torch.zeros(P, B, device=DEV, dtype=F64) if rowsum is None else rowsum.to(DEV)
    ops.mmd_fold(part, rowsum)
    total = torch.full((P + 1,), NAN, device=DEV, dtype=F64)
    ops.mmd_total(rowsum, total[:P])
    assert bool(buf[P * tiles * B:].isnan().all()) and bool(total[P:].isnan().all())
    return part.cpu(), rowsum.cpu(), total[:P].cpu()


# ---------------------------------------------------------------------------------------------------------------- 1. the oracle, exact
@pytest.mark.parametrize("i", range(NCASE), ids=M.IDS)
def test_part_rowsum_and_total_equal_the_oracle(i):
    _gpu()
    for qs, xs in PASSES:
        S = products(i, qs, xs)
        B, N = S.shape
        base = 0 if qs == xs else -1
        for degree in (2, 3):
            want = M.oracle_part(S, gamma_of(i), 1.0, degree, query_base=base)
            want_r = M.oracle_fold(want)
            want_t = M.oracle_total(want_r)
            for q, x in ((on_device(i, qs), on_device(i, xs)), (sliced(sets_of(i)[qs]), sliced(sets_of(i)[xs]))):
                part, rowsum, total = run(q, x, 1, B, N, gamma_of(i), degree, query_base=base)
                assert same_bits(part[0], want), (qs, xs, degree)
                assert same_bits(rowsum[0], want_r), (qs, xs, degree)
                assert same_bits(total[0], want_t), (qs, xs, degree)
        # the diagonal matters: without exclusion the self pass differs
        if base == 0:
            assert not same_bits(run(on_device(i, qs), on_device(i, xs), 1, B, N, gamma_of(i))[1][0], want_r)


@pytest.mark.parametrize("i", M.SUBSET_CASES, ids=[M.IDS[i] for i in M.SUBSET_CASES])
def test_index_lists_equal_the_oracle_on_the_gathered_rows(i):
    """P = 3 shuffled subsets of 129 rows as the problems of one launch, against the oracle on the products of the gathered rows; and
    the identity written out as a list"""
    _gpu()
    s = sets_of(i)
    P, m = M.SUBSETS, M.SUBSET_SIZE
    tab = dict(zip(SETS, M.draws(s["real"].shape[0], s["fake"].shape[0], P, m, i)))
    dtab = {k: v.to(I32).to(DEV) for k, v in tab.items()}
    for qs, xs in PASSES:
        base = 0 if qs == xs else -1
        S = torch.stack([M.gemm_parts(s[qs][tab[qs][p]], s[xs][tab[xs][p]])[0] for p in range(P)])
        want = M.oracle_part(S, gamma_of(i), 1.0, 3, query_base=base)
        want_r = M.oracle_fold(want)
        want_t = M.oracle_total(want_r)
        for q, x in ((on_device(i, qs), on_device(i, xs)), (sliced(s[qs]), sliced(s[xs]))):
            part, rowsum, total = run(q, x, P, m, m, gamma_of(i), 3, query_base=base, qi=dtab[qs], xi=dtab[xs])
            assert same_bits(part, want) and same_bits(rowsum, want_r) and same_bits(total, want_t), (qs, xs)
        assert not torch.equal(want_r[0], want_r[1]) and not torch.equal(want_r[1], want_r[2])  # the problems differ
    # one list and one identity side; the identity as a list; an index outside the matrix reads a row of zeros: k = coef0^3 = 1
    S = products(i, "real", "fake")
    B, N = S.shape
    want = M.oracle_part(S, gamma_of(i))
    ident = {k: torch.arange(v.shape[0], dtype=I32, device=DEV)[None] for k, v in s.items()}
    q, x = on_device(i, "real"), on_device(i, "fake")
    for kw in (dict(qi=ident["real"]), dict(xi=ident["fake"]), dict(qi=ident["real"], xi=ident["fake"])):
        assert same_bits(run(q, x, 1, B, N, gamma_of(i), **kw)[0][0], want), kw
    out = torch.tensor([[-1, N, 2 ** 31 - 1]], dtype=I32, device=DEV)
    assert run(q, x, 1, B, 3, gamma_of(i), xi=out)[1][0].tolist() == [3.0] * B


# ---------------------------------------------------------------------------------------------------------------- 2. chunks and the diagonal
def test_a_self_pass_in_two_chunks_excludes_exactly_the_diagonal():
    """index_base = 128: the second chunk's tiles cover the same absolute rows as tiles 1 .. of the whole, and its excluded pairs lie
    on the shifted diagonal; query passes move query_base"""
    _gpu()
    for i, s in ((0, "real"), (2, "fake")):
        S = products(i, s, s)
        n = S.shape[0]
        want = M.oracle_part(S, gamma_of(i), query_base=0)
        want_r = M.oracle_fold(want)
        x = on_device(i, s)
        for cut in (128, 256) if n > 256 else (128,):
            p0, r0, _ = run(x, x[:cut], 1, n, cut, gamma_of(i), query_base=0, index_base=0)
            p1, r1, t1 = run(x, x[cut:], 1, n, n - cut, gamma_of(i), query_base=0, index_base=cut, rowsum=r0)
            assert same_bits(torch.cat([p0, p1], 1)[0], want), (i, cut)
            assert same_bits(p1[0], M.oracle_part(S[:, cut:].contiguous(), gamma_of(i), query_base=0, index_base=cut))
            assert same_bits(r1[0], want_r) and same_bits(t1[0], M.oracle_total(want_r)), (i, cut)
        # queries in passes of 50 against the bank in chunks of 128
        rows = []
        for b0 in range(0, n, 50):
            b1, r = min(n, b0 + 50), None
            for n0 in range(0, n, 128):
                r = run(x[b0:b1], x[n0:n0 + 128], 1, b1 - b0, min(n, n0 + 128) - n0, gamma_of(i), query_base=b0, index_base=n0, rowsum=r)[1]
            rows.append(r[0])
        assert same_bits(torch.cat(rows), want_r), i
        # bases that name no pair of the call exclude nothing
        assert same_bits(run(x[:50], x, 1, 50, n, gamma_of(i), query_base=5000)[1][0], M.oracle_fold(M.oracle_part(S[:50].contiguous(), gamma_of(i))))


def test_the_total_is_the_neighbour_tree_at_every_block_edge():
    """B around the 512-element blocks of vtp_mmd_total, values whose sum depends on the order"""
    _gpu()
    from vtp_amd import ops
    g = torch.Generator().manual_seed(0)
    for B in (1, 2, 3, 511, 512, 513, 1025, 5000):
        r = (torch.randn(2, B, generator=g, dtype=F64) * torch.logspace(-8, 8, B, dtype=F64)[torch.randperm(B, generator=g)])
        total = torch.empty(2, device=DEV, dtype=F64)
        ops.mmd_total(r.to(DEV), total)
        assert same_bits(total.cpu(), M.oracle_total(r)), B


# ---------------------------------------------------------------------------------------------------------------- 3. the class
def oracle_kid(i, subsets=0):
    """what KID must return on case i, bit for bit: the oracle's totals through the host's finish"""
    s = sets_of(i)
    if not subsets:
        t = [float(M.oracle_total(M.oracle_fold(M.oracle_part(products(i, qs, xs), gamma_of(i), query_base=0 if qs == xs else -1))))
             for qs, xs in PASSES]
        return {"kid": M.estimate(*t, s["real"].shape[0], s["fake"].shape[0])}
    m = M.SUBSET_SIZE
    tab = dict(zip(SETS, M.draws(s["real"].shape[0], s["fake"].shape[0], subsets, m, i)))
    t = []
    for qs, xs in PASSES:
        S = torch.stack([M.gemm_parts(s[qs][tab[qs][p]], s[xs][tab[xs][p]])[0] for p in range(subsets)])
        t.append(M.oracle_total(M.oracle_fold(M.oracle_part(S, gamma_of(i), query_base=0 if qs == xs else -1))).tolist())
    mean, std = M.mean_std([M.estimate(a, b, c, m, m) for a, b, c in zip(*t)])
    return {"kid": mean, "kid_std": std}


def feed(kid, i, ragged):
    real, fake = on_device(i, "real"), on_device(i, "fake")
    if ragged:
        for a, b in ((0, 1), (1, 8), (8, 130), (130, real.shape[0])):
            if a < real.shape[0]:
                kid.add_real_features(real[a:b])
        for a, b in ((0, 100), (100, 101), (101, fake.shape[0])):
            kid.add_fake_features(sliced(fake[a:b].cpu()))
    else:
        kid.add_real_features(real)
        kid.add_fake_features(fake)
    return kid


def test_the_result_repeats_bit_for_bit_whatever_the_chunking_the_batching_and_the_banks():
    _gpu()
    from vtp_amd import KID, PrecisionRecall
    i = 0
    for subsets in (0, M.SUBSETS):
        want = oracle_kid(i, subsets)
        kw = dict(subsets=subsets, subset_size=M.SUBSET_SIZE, seed=i)
        seen = []
        for chunk_rows in (128, 256, 65536):
            for query_rows in (40, 128, 1024):
                kid = feed(KID(chunk_rows=chunk_rows, query_rows=query_rows, **kw), i, ragged=(chunk_rows + query_rows) % 3 == 0)
                seen.append(kid.result())
                assert kid.result() == seen[-1]
        pr = PrecisionRecall(k=3, chunk_rows=100)
        feed(pr, i, ragged=True)
        shared = KID(banks=pr, chunk_rows=200, **kw)  # 200 rounds up to 256
        assert shared.chunk_rows == 256 and shared.rows("real").data_ptr() == pr.rows("real").data_ptr()
        seen.append(shared.result())
        assert pr.result()["precision"] > 0  # the shared banks still serve their owner
        with pytest.raises(RuntimeError, match="add the rows there"):
            shared.add_real_features(on_device(i, "real"))
        assert all(out == want for out in seen), (subsets, want, seen)
        assert set(want) == ({"kid", "kid_std"} if subsets else {"kid"})
    # the full-set row sums: per-sample scores, the oracle's bits
    kid = feed(KID(subsets=0, query_rows=77), i, ragged=False)
    with pytest.raises(RuntimeError, match="after result"):
        kid.row_sums()
    kid.result()
    rs = kid.row_sums()
    for qs, xs in PASSES:
        want_r = M.oracle_fold(M.oracle_part(products(i, qs, xs), gamma_of(i), query_base=0 if qs == xs else -1))
        assert rs[f"{qs}_{xs}"].is_cuda and same_bits(rs[f"{qs}_{xs}"].cpu(), want_r), (qs, xs)
    # other kernel parameters and seeds change the value; errors
    assert feed(KID(subsets=0, degree=2), i, False).result() != kid.result()
    assert feed(KID(subsets=0, gamma=0.5), i, False).result() != kid.result()
    a = feed(KID(subsets=3, subset_size=129, seed=1), i, False)
    assert a.result() != oracle_kid(i, 3) and a.result() == a.result()
    # the kept tables are redrawn when the row counts change: what a fresh object returns
    b = feed(KID(subsets=3, subset_size=129, seed=1), i, False)
    for k in (a, b):
        k.add_fake_features(on_device(i, "real")[:7])
    assert a.result() == b.result()
    with pytest.raises(ValueError, match="exceeds the smaller set"):
        feed(KID(subsets=2, subset_size=258), i, False).result()
    with pytest.raises(ValueError, match="no CPU path"):
        a.add_real_features(torch.zeros(4, 64))
    with pytest.raises(ValueError, match="like the real bank"):
        a.add_fake_features(torch.zeros(4, 8, device=DEV))
    a.reset()
    with pytest.raises(RuntimeError, match="empty"):
        a.result()
    a.add_real_features(on_device(i, "real")[:1])
    a.add_fake_features(on_device(i, "fake")[:5])
    a.subsets = 0
    with pytest.raises(ValueError, match="at least 2 rows"):
        a.result()


# ---------------------------------------------------------------------------------------------------------------- 4. against fp64
@pytest.mark.parametrize("i", range(NCASE), ids=M.IDS)
def test_the_distance_is_within_the_a_priori_bound_of_fp64(i):
    _gpu()
    from vtp_amd import KID
    kid64, bnd = M.case_64(i)
    got = feed(KID(subsets=0), i, False).result()["kid"]
    orc = oracle_kid(i)["kid"]
    print(f"KID {M.IDS[i]} full: kid {got:.9f} fp64 {kid64:.9f}  |err| / bound: kernels {abs(got - kid64) / bnd:.3e}, oracle "
          f"{abs(orc - kid64) / bnd:.3e}  (bound {bnd:.3e} = {bnd / abs(kid64):.2e} of |kid|)")
    assert bnd <= 0.01 * abs(kid64)
    assert abs(orc - kid64) <= bnd  # the oracle is built from the GEMM products: were this to fail, the bound would be wrong
    assert abs(got - kid64) <= bnd
    if i in M.SUBSET_CASES:
        ref, bnds = M.subset_case_64(i)
        out = feed(KID(subsets=M.SUBSETS, subset_size=M.SUBSET_SIZE, seed=i), i, False).result()
        mean_b, max_b = sum(bnds) / len(bnds), max(bnds)
        print(f"KID {M.IDS[i]} subsets: kid {out['kid']:.9f} fp64 {ref['kid']:.9f} |err| / bound {abs(out['kid'] - ref['kid']) / mean_b:.3e}; "
              f"kid_std {out['kid_std']:.9f} fp64 {ref['kid_std']:.9f} |err| / bound {abs(out['kid_std'] - ref['kid_std']) / max_b:.3e}")
        assert all(b <= 0.01 * abs(v) for b, v in zip(bnds, ref["values"]))
        # the mean moves by at most the mean of the subsets' bounds; the standard deviation is the norm of the centred values over
        # sqrt(P), so it moves by at most the largest of them
        assert abs(out["kid"] - ref["kid"]) <= mean_b and abs(out["kid_std"] - ref["kid_std"]) <= max_b


# ---------------------------------------------------------------------------------------------------------------- 5. NaN
def test_a_nan_row_gives_a_nan_result_and_nothing_else():
    _gpu()
    from vtp_amd import KID
    i = 2
    real = on_device(i, "real").clone()
    real[7, 3] = NAN
    for kw in (dict(subsets=0), dict(subsets=1, subset_size=130)):
        kid = KID(**kw)
        kid.add_real_features(real)
        kid.add_fake_features(on_device(i, "fake"))
        out = kid.result()
        assert out["kid"] != out["kid"], kw
    # the row sums tell which row it was: row 7 and, through the products with it, every other real row; the fake set stays finite
    kid = KID(subsets=0)
    kid.add_real_features(real)
    kid.add_fake_features(on_device(i, "fake"))
    kid.result()
    rs = kid.row_sums()
    assert bool(rs["real_real"].isnan().all()) and bool(rs["fake_fake"].isfinite().all())
    assert rs["real_fake"].isnan().nonzero().flatten().tolist() == [7]


# ---------------------------------------------------------------------------------------------------------------- 6. GenEval
def test_gen_eval_reports_kid_on_the_rows_it_feeds(monkeypatch):
    """the feature path and the Frechet distance are stubbed (they have their own tests): rows of case 4 stand in for the pool
    features of the byte images"""
    _gpu()
    from vtp_amd import FrechetStats, GenEval, InceptionFeatures, KID, gen_eval
    i = 4
    real, fake = on_device(i, "real"), on_device(i, "fake")
    monkeypatch.setattr(gen_eval, "frechet_distance", lambda *a, **k: 0.0)
    inc = InceptionFeatures("pytorch_fid").to(DEV)

    def make(**kw):
        ge = GenEval(inc, **kw)
        ge._spatial = {s: FrechetStats(16, ge.device) for s in ("real", "generated")}  # what the first pass would make
        ge._pass = lambda rows: (rows, rows[:, :16].contiguous())
        for a, b in ((0, 7), (7, 40)):
            ge.add_real(real[a:b])
        for a, b in ((0, 200), (200, 257)):
            ge.add_generated(fake[a:b])
        return ge

    args = dict(subsets=3, subset_size=30, seed=2)
    want = feed(KID(**args), i, False).result()
    shared = make(k=3, kid=args)
    assert all(shared.kid.rows(s).data_ptr() == shared.pr.rows(s).data_ptr() for s in ("real", "fake"))  # one copy of the rows
    out = shared.results("eig")
    assert set(out) == {"fid", "sfid", "precision", "recall", "kid", "kid_std"}
    assert {k: out[k] for k in ("kid", "kid_std")} == want
    own = make(k=None, kid=dict(subsets=0))
    out = own.results("eig")
    assert set(out) == {"fid", "sfid", "kid"} and out["kid"] == oracle_kid(i)["kid"]
    assert make(k=None, kid=True).kid.subsets == 100  # True: the defaults of KID
    assert set(make(k=3).results("eig")) == {"fid", "sfid", "precision", "recall"}  # the defaults: as before
    own.reset()
    with pytest.raises(RuntimeError, match="add_generated"):
        own.results()
    with pytest.raises(RuntimeError, match="empty"):
        own.kid.result()


# ---------------------------------------------------------------------------------------------------------------- 7. two ranks
SHARDS = {"real": (100, 300), "fake": (200, 257)}  # rank 0 holds rows [0, first), rank 1 the rest: uneven shards


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from vtp_amd import KID
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    real, fake = M.case(0)
    cut = {s: (0, SHARDS[s][0]) if rank == 0 else SHARDS[s] for s in SETS}
    res = []
    for kw in (dict(subsets=0, query_rows=100), dict(subsets=M.SUBSETS, subset_size=M.SUBSET_SIZE, seed=0)):
        kid = KID(group=dist.group.WORLD, **kw)
        kid.add_real_features(real[cut["real"][0]:cut["real"][1]].to(DEV))
        kid.add_fake_features(fake[cut["fake"][0]:cut["fake"][1]].to(DEV))
        res.append(kid.result())
    out[rank] = res
    dist.destroy_process_group()


def test_two_ranks_equal_the_single_process_on_the_concatenation():
    _gpu()
    one = [oracle_kid(0), oracle_kid(0, M.SUBSETS)]
    torch.cuda.empty_cache()
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        assert out[r] == one, (r, out[r], one)
