"""GPU: the precision / recall kernels (csrc/precision_recall.hip: vtp_pr_sqnorm / vtp_pr_knn_dist / vtp_pr_cover) and
vtp_amd.PrecisionRecall.

Distances, lists and hit counts are compared with EQUALITY.  The oracle is tests/pr_ref.py::oracle32: the kernels' formula evaluated
on the host in torch fp32 from the products and norms that ops.gemm_nt_f32 formed (the bank zero-padded to a multiple of 8 rows, the
pad columns dropped); the expected lists are the 8 smallest per row of a host sort, the expected hits a host compare.

Against the fp64 restatement (direct ((a - b)^2).sum() distances) decisions are compared: a row is left out when one of its
distances is within tau * (|q|^2 + |x|^2) of the radius it is compared with, tau = 4 x the largest error of oracle32 (the GEMM-built
oracle, not the kernels under test) relative to |q|^2 + |x|^2 over all cases: x 2 because the radius carries the same error as the
distance, x 2 for other draws.  Measured on an MI355X (the test prints it): the error is 4.6e-7, 3.6e-7, 2.2e-7, 5.2e-7 and 2.64e-6
for the five cases in order -- the D = 2048 case sets it: one fmaf chain of 2048 terms against torch's blocked sums, and still a
hundredth of the a-priori bound 2 (D + 2) 2^-24 = 2.4e-4 -- so tau = 1.056e-5.  With it at most 2 of 129 rows (1.6 %, k = 8) are
left out, no decision and no hit count outside them differs, and the radii are within 3.4e-6 x 2 |x|^2 of fp64."""
import functools
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

import pr_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
NAN, INF = float("nan"), float("inf")
SPLITS = [0, 1, 3, 64]
NCASE = len(R.CASES)
SETS = ("real", "fake")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.contiguous().view(I32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sliced(x, pad=8, off=4):
    """x on the GPU as a column slice (offset `off`, row stride D + pad) of a wider NaN-poisoned matrix"""
    wide = torch.full((x.shape[0], x.shape[1] + pad), NAN, dtype=F32)
    wide[:, off:off + x.shape[1]] = x
    return wide.to(DEV)[:, off:off + x.shape[1]]


@functools.lru_cache(maxsize=None)
def oracle(i, qs, xs):
    """case i, queries from set qs against the bank xs ("real" / "fake"): (d2 of oracle32, qn, xn) on the CPU, computed once"""
    sets = dict(zip(SETS, R.case(i)))
    S, qn, xn = R.gemm_parts(sets[qs], sets[xs])
    return R.oracle32(S, qn, xn), qn, xn


def oracle_radii(i, s, k):
    """the squared radii of set s of case i: column k - 1 of the oracle's lists of the set against itself"""
    return R.lists32(oracle(i, s, s)[0], query_base=0)[:, k - 1].contiguous()


@functools.lru_cache(maxsize=None)
def on_device(i, s):
    return dict(zip(SETS, R.case(i)))[s].to(DEV)


def run_knn(q, qn, chunks, query_base=-1, splits=0, d2_out=None):
    """q [B, D], qn [B] on the device and chunks = [(bank rows, norms, index_base), ...] -> the lists on the CPU"""
    from vtp_amd import ops
    B = q.shape[0]
    dist = torch.full((B, 8), INF, device=DEV)
    ws = torch.empty(ops.pr_workspace_bytes(B, splits), device=DEV, dtype=torch.uint8)
    for x, xn, base in chunks:
        ops.pr_knn_dist(q, qn, x, xn, dist, ws, query_base=query_base, index_base=base, splits=splits, d2_out=d2_out)
    return dist.cpu()


def run_cover(q, qn, chunks, splits=0, start=0):
    """chunks = [(bank rows, norms, radii), ...] -> the hit counts on the CPU"""
    from vtp_amd import ops
    hits = torch.full((q.shape[0],), start, device=DEV, dtype=I32)
    for x, xn, r2 in chunks:
        ops.pr_cover(q, qn, x, xn, r2, hits, splits=splits)
    return hits.cpu()


def cuts_of(n, step):
    return [(a, min(n, a + step)) for a in range(0, n, step)]


# ---------------------------------------------------------------------------------------------------------------- 1. norms
@pytest.mark.parametrize("D", [8, 24, 64, 136, 2048])
def test_sqnorm_has_the_bits_of_the_gemm_diagonal(D):
    _gpu()
    from vtp_amd import ops
    g = torch.Generator().manual_seed(D)
    for N in (1, 129):
        x = torch.randn(N, D, generator=g) * 3
        want = R.gemm_parts(x, x)[2]
        for xd in (x.to(DEV), sliced(x)):
            out = torch.full((N + 2,), NAN, device=DEV)
            ops.pr_sqnorm(xd, out[:N])
            assert same_bits(out[:N].cpu(), want), (N, D)
            assert bool(out[N:].isnan().all())


# ---------------------------------------------------------------------------------------------------------------- 2. distances and lists, exact
@pytest.mark.parametrize("i", range(NCASE), ids=R.IDS)
def test_distances_and_lists_equal_the_oracle(i):
    _gpu()
    for qs in SETS:
        for xs in SETS:
            d2, qn, xn = oracle(i, qs, xs)
            B, N = d2.shape
            base = 0 if qs == xs else -1  # a set against itself: self-exclusion on
            want = R.lists32(d2, query_base=base)
            q, x, qnd, xnd = on_device(i, qs), on_device(i, xs), qn.to(DEV), xn.to(DEV)
            for splits in SPLITS:
                dump = torch.full((B, N + 3), NAN, device=DEV)
                got = run_knn(q, qnd, [(x, xnd, 0)], base, splits, dump[:, :N])
                assert same_bits(got, want), (qs, xs, splits)
                assert same_bits(dump[:, :N].cpu(), d2) and bool(dump[:, N:].isnan().all()), (qs, xs, splits)


def test_a_five_row_set_gives_lists_that_end_in_inf():
    _gpu()
    d2, _, xn = oracle(0, "real", "real")
    x, xnd = on_device(0, "real")[:5], xn[:5].to(DEV)
    want = R.lists32(d2[:5, :5], query_base=0)
    assert bool(want[:, :4].isfinite().all()) and bool((want[:, 4:] == INF).all())
    for splits in SPLITS:
        assert same_bits(run_knn(x, xnd, [(x, xnd, 0)], 0, splits), want), splits


# ---------------------------------------------------------------------------------------------------------------- 3. chunking and layout
def test_chunks_layouts_and_passes_give_the_same_lists():
    _gpu()
    i, s = 0, "real"
    d2, _, xn = oracle(i, s, s)
    N = d2.shape[0]
    want = R.lists32(d2, query_base=0)
    x, xnd = on_device(i, s), xn.to(DEV)
    assert same_bits(run_knn(x, xnd, [(x, xnd, 0)], 0), want)
    for step in (1, 127, 128, 129, N):
        chunks = [(x[a:b], xnd[a:b], a) for a, b in cuts_of(N, step)]
        assert same_bits(run_knn(x, xnd, chunks, 0), want), step
    # query passes of 50, the bank in chunks of 127, every index moved by 1000: the excluded pair of a late pass lies in a later chunk
    for step in (127, N):
        got = torch.cat([run_knn(x[a:b], xnd[a:b], [(x[c:d], xnd[c:d], 1000 + c) for c, d in cuts_of(N, step)], 1000 + a)
                         for a, b in cuts_of(N, 50)])
        assert same_bits(got, want), step
    # bases that name no pair of the call exclude nothing; equal bases exclude the diagonal
    assert same_bits(run_knn(x[:50], xnd[:50], [(x, xnd, 0)], 5000), R.lists32(d2[:50]))
    # column slices of wider NaN-poisoned matrices
    xs = sliced(R.case(i)[0])
    assert same_bits(run_knn(xs, xnd, [(xs[a:b], xnd[a:b], a) for a, b in cuts_of(N, 129)], 0, 3), want)
    # without exclusion a row finds itself at exactly 0
    got = run_knn(x, xnd, [(x, xnd, 0)], -1)
    assert same_bits(got, R.lists32(d2)) and bool((got[:, 0] == 0).all())


def test_a_self_pass_across_the_tile_edge():
    """130 x 130: rows 128 and 129 are excluded in the second tile, chunked so that the pair moves between tiles"""
    _gpu()
    i = 2
    for s in SETS:
        d2, _, xn = oracle(i, s, s)
        want = R.lists32(d2, query_base=0)
        x, xnd = on_device(i, s), xn.to(DEV)
        for step in (1, 64, 129, 130):
            assert same_bits(run_knn(x, xnd, [(x[a:b], xnd[a:b], a) for a, b in cuts_of(130, step)], 0), want), (s, step)


# ---------------------------------------------------------------------------------------------------------------- 4. exact ties and duplicates
@functools.lru_cache(maxsize=None)
def dyadic_case(B=70, N=200, D=64, seed=0):
    """entries m / 8, |m| <= 4: every product is a multiple of 1 / 64 and every partial sum stays below 64 / 4 = 16 in magnitude, so
    products, norms and distances are exact in fp32 whatever the order, and equal distances are frequent.  Bank rows 7 and 150 are
    twins of row 3; queries 0 .. 4 are copies of bank rows 0 .. 4.  Returns (q, x) f32 and the integer distances in units of 1 / 64."""
    g = torch.Generator().manual_seed(seed)
    mq = torch.randint(-4, 5, (B, D), generator=g)
    mx = torch.randint(-4, 5, (N, D), generator=g)
    mx[7] = mx[3]
    mx[150] = mx[3]
    mq[:5] = mx[:5]
    dqx = ((mq[:, None, :] - mx[None, :, :]) ** 2).sum(-1)
    dxx = ((mx[:, None, :] - mx[None, :, :]) ** 2).sum(-1)
    return mq.to(F32) / 8, mx.to(F32) / 8, dqx, dxx


def test_exact_ties_and_duplicates_equal_integer_arithmetic():
    _gpu()
    from vtp_amd import ops
    q, x, dqx, dxx = dyadic_case()
    B, N = dqx.shape
    qd, xd = q.to(DEV), x.to(DEV)
    qn, xn = torch.empty(B, device=DEV), torch.empty(N, device=DEV)
    ops.pr_sqnorm(qd, qn)
    ops.pr_sqnorm(xd, xn)
    assert torch.equal(qn.cpu(), (q * q).sum(1)) and torch.equal(xn.cpu(), (x * x).sum(1))
    # lists: the integer sort, ties and all
    want = R.lists32(dqx.to(F32) / 64)
    want_self = R.lists32(dxx.to(F32) / 64, query_base=0)
    assert sum(len(set(row)) < 8 for row in want.tolist()) > 0  # equal distances do occur among the 8 smallest
    for splits in SPLITS:
        dump = torch.full((B, N), NAN, device=DEV)
        assert torch.equal(run_knn(qd, qn, [(xd, xn, 0)], -1, splits, dump), want), splits
        assert torch.equal(dump.cpu() * 64, dqx.to(F32))
        assert torch.equal(run_knn(xd, xn, [(xd[a:b], xn[a:b], a) for a, b in cuts_of(N, 77)], 0, splits), want_self), splits
    # the twins of row 3 are at exactly 0 from it and counted: two zeros lead the lists of rows 3, 7 and 150
    assert want_self[[3, 7, 150], :2].eq(0).all() and want_self[3, 2] > 0 and want_self[0, 0] > 0
    # hits: r2[n] = the distance of query 9 to bank row n, so query 9 hits every row on the boundary d2 == r2
    r2i = dqx[9].clone()
    want_hits = (dqx <= r2i[None, :]).sum(1).to(I32)
    assert int(want_hits[9]) == N and 0 < int(want_hits.min()) < N
    r2 = (r2i.to(F32) / 64).to(DEV)
    for splits in SPLITS:
        assert torch.equal(run_cover(qd, qn, [(xd, xn, r2)], splits), want_hits), splits
    # r2 = 0 hits exact duplicates alone: queries 0 .. 4 are bank rows 0 .. 4, and row 3 has two twins
    zero = torch.zeros(N, device=DEV)
    got = run_cover(qd, qn, [(xd[a:b], xn[a:b], zero[a:b]) for a, b in cuts_of(N, 130)])
    assert torch.equal(got, (dqx == 0).sum(1).to(I32)) and got[:5].tolist() == [1, 1, 1, 3, 1] and int(got[5:].sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- 5. hits, exact
@pytest.mark.parametrize("i", range(NCASE), ids=R.IDS)
def test_hits_equal_the_oracle(i):
    _gpu()
    for k in R.ks_of(i):
        for qs, xs in (("fake", "real"), ("real", "fake")):
            d2, qn, xn = oracle(i, qs, xs)
            r2 = oracle_radii(i, xs, k)
            want = R.hits32(d2, r2)
            N = d2.shape[1]
            q, x, qnd, xnd, r2d = on_device(i, qs), on_device(i, xs), qn.to(DEV), xn.to(DEV), r2.to(DEV)
            for splits in SPLITS:
                assert torch.equal(run_cover(q, qnd, [(x, xnd, r2d)], splits), want), (k, qs, splits)
            # the bank in chunks, accumulated across calls into a buffer that starts at 5
            for step in (1, 127, 129):
                got = run_cover(q, qnd, [(x[a:b], xnd[a:b], r2d[a:b]) for a, b in cuts_of(N, step)], 0, start=5)
                assert torch.equal(got, want + 5), (k, qs, step)
            # query passes of 50 on column slices
            xs_ = sliced(x.cpu())
            got = torch.cat([run_cover(q[a:b], qnd[a:b], [(xs_, xnd, r2d)], 3) for a, b in cuts_of(q.shape[0], 50)])
            assert torch.equal(got, want), (k, qs)


# ---------------------------------------------------------------------------------------------------------------- 6. against fp64
@functools.lru_cache(maxsize=None)
def oracle_error():
    """per case the largest |oracle32 - d2_64| / (|q|^2 + |x|^2) over the four directions, and tau = 4 x the largest of them"""
    errs = []
    for i in range(NCASE):
        sets = dict(zip(SETS, R.case(i)))
        e = 0.0
        for qs in SETS:
            for xs in SETS:
                q64, x64 = sets[qs].to(F64), sets[xs].to(F64)
                scale = (q64 * q64).sum(1)[:, None] + (x64 * x64).sum(1)[None, :]
                e = max(e, float(((oracle(i, qs, xs)[0].to(F64) - R.d2_64(q64, x64)).abs() / scale).max()))
        errs.append(e)
    return errs, 4 * max(errs)


def test_oracle_error_is_below_the_a_priori_bound():
    _gpu()
    errs, tau = oracle_error()
    print(f"PR oracle32 error relative to |q|^2 + |x|^2 per case: {['%.3e' % e for e in errs]}; tau = {tau:.3e}")
    for i, e in enumerate(errs):
        D = R.CASES[i][1][2]
        assert e < 2 * (D + 2) * 2.0 ** -24, (R.IDS[i], e)


@pytest.mark.parametrize("i", range(NCASE), ids=R.IDS)
def test_decisions_agree_with_fp64(i):
    _gpu()
    errs, tau = oracle_error()
    sets = dict(zip(SETS, R.case(i)))
    n64 = {s: (sets[s].to(F64) ** 2).sum(1) for s in SETS}
    for k in R.ks_of(i):
        ref = R.case_64(i, k)
        assert min(ref["counts"]) >= R.FLOOR
        # the kernels' radii
        r2 = {}
        for s in SETS:
            xn = oracle(i, s, s)[1].to(DEV)
            r2[s] = run_knn(on_device(i, s), xn, [(on_device(i, s), xn, 0)], 0)[:, k - 1].contiguous()
            dev = (r2[s].to(F64) - ref["radii_" + s]).abs()
            print(f"PR {R.IDS[i]} k={k} {s} radii: largest |r2 - r2_64| / (2 |x|^2) = {float((dev / (2 * n64[s])).max()):.3e} (tau {tau:.3e})")
            assert bool((dev <= tau * 2 * n64[s]).all()), (k, s)
        shares = {}
        for name, qs, xs in (("precision", "fake", "real"), ("recall", "real", "fake")):
            _, qn, xn = oracle(i, qs, xs)
            hits = run_cover(on_device(i, qs), qn.to(DEV), [(on_device(i, xs), xn.to(DEV), r2[xs].to(DEV))])
            want = ref["hits_" + qs]
            d64 = R.d2_64(sets[qs], sets[xs])
            near = ((d64 - ref["radii_" + xs][None, :]).abs() <= tau * (n64[qs][:, None] + n64[xs][None, :])).any(1)
            wrong = ((hits > 0) != (want > 0))
            B = hits.shape[0]
            print(f"PR {R.IDS[i]} k={k} {name}: {int(near.sum())} of {B} rows left out, {int(wrong.sum())} decisions differ, "
                  f"{int((hits != want).sum())} hit counts differ")
            assert int(near.sum()) <= 0.02 * B, (k, name)
            assert not bool((wrong & ~near).any()), (k, name)
            shares[name] = int((hits > 0).sum()) / B
            assert abs(shares[name] - ref[name]) <= int(near.sum()) / B, (k, name)


# ---------------------------------------------------------------------------------------------------------------- 7. through the class
def test_through_the_class():
    _gpu()
    from vtp_amd import PrecisionRecall
    i = 0
    real, fake = on_device(i, "real"), on_device(i, "fake")
    Nr, Ng = real.shape[0], fake.shape[0]
    first = None
    for k in (1, 3):
        want_r = {s: oracle_radii(i, s, k) for s in SETS}
        want_h = {"fake": R.hits32(oracle(i, "fake", "real")[0], want_r["real"]), "real": R.hits32(oracle(i, "real", "fake")[0], want_r["fake"])}
        for kw in (dict(), dict(chunk_rows=100, query_rows=77), dict(capacity=1000, chunk_rows=1 << 20, query_rows=128)):
            pr = PrecisionRecall(k=k, **kw)
            # uneven calls; without capacity the banks start at one row and must grow several times
            for a, b in ((0, 1), (1, 8), (8, 130), (130, Nr)):
                pr.add_real_features(real[a:b])
            for a, b in ((0, 200), (200, 201), (201, Ng)):
                pr.add_fake_features(sliced(fake[a:b].cpu()))  # any layout is copied into the bank
            assert pr.rows("real").shape == (Nr, real.shape[1]) and torch.equal(pr.rows("fake"), fake)
            out = pr.result()
            for s in SETS:
                assert same_bits(pr.radii(s).cpu(), want_r[s]), (k, kw, s)
                assert pr.hits(s).dtype == I32 and torch.equal(pr.hits(s).cpu(), want_h[s]), (k, kw, s)
            cnt = pr.counts()
            pc, rc = int((want_h["fake"] > 0).sum()), int((want_h["real"] > 0).sum())
            assert cnt == {"precision": (pc, Ng), "recall": (rc, Nr)}
            assert out == {"precision": pc / Ng, "recall": rc / Nr} and pr.result() == out
        ref = R.case_64(i, k)
        print(f"PR class {R.IDS[i]} k={k}: {cnt}, fp64 {ref['counts']}")
        if k == 1:
            first = out
    assert first != out  # k matters
    # more rows change the result; reset empties the banks
    pr.add_fake_features(real[:50])
    assert pr.counts()["precision"][1] == Ng + 50
    pr.add_real_features(real[:1])  # the banks changed: the last result is forgotten
    with pytest.raises(RuntimeError, match="after result"):
        pr.radii("real")
    pr.reset()
    with pytest.raises(RuntimeError, match="empty"):
        pr.result()
    pr.add_real_features(real[:3])
    pr.add_fake_features(fake[:10])
    with pytest.raises(RuntimeError, match="fewer than k \\+ 1"):
        pr.result()
    with pytest.raises(ValueError, match="like the real bank"):
        pr.add_fake_features(torch.zeros(2, 8, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- 8. two ranks
SHARDS = {"real": (100, 300), "fake": (200, 257)}  # rank 0 holds rows [0, first), rank 1 the rest: uneven shards


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _summary(pr):
    return (pr.result(), pr.counts(), [int(bits(pr.radii(s)).sum()) for s in SETS], [int(pr.hits(s).sum()) for s in SETS])


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from vtp_amd import PrecisionRecall
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    real, fake = R.case(0)
    pr = PrecisionRecall(k=3, group=dist.group.WORLD, query_rows=100)
    cut = {s: (0, SHARDS[s][0]) if rank == 0 else SHARDS[s] for s in SETS}
    pr.add_real_features(real[cut["real"][0]:cut["real"][1]].to(DEV))
    pr.add_fake_features(fake[cut["fake"][0]:cut["fake"][1]].to(DEV))
    out[rank] = _summary(pr)
    dist.destroy_process_group()


def test_two_ranks_equal_the_single_process_on_the_concatenation():
    _gpu()
    from vtp_amd import PrecisionRecall
    pr = PrecisionRecall(k=3)
    pr.add_real_features(on_device(0, "real"))
    pr.add_fake_features(on_device(0, "fake"))
    one = _summary(pr)
    assert one[1]["precision"][1] == 257 and one[1]["recall"][1] == 300
    del pr
    torch.cuda.empty_cache()
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        assert out[r] == one
