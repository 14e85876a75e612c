"""GPU: the k-NN kernels (csrc/knn.hip: vtp_knn_topk / vtp_knn_vote) and vtp_amd.Knn.

Neighbours are compared with EQUALITY.  The oracle of the similarities is ops.gemm_nt_f32 (the bank zero-padded to a multiple of 8
rows, the pad columns dropped): vtp_knn_topk promises the bits of that kernel, and how far those are from fp64 is
tests/test_fp32_kernels_gpu.py's business.  The expected lists are the first K of a host sort of that matrix by (-s, index).

Votes are compared with tests/knn_ref.py, evaluated in fp64 on the fp32 lists the kernel itself returned.  The kernel's weights are
fp32: the argument (s_j - s_0) / T is up to 2 / 0.07 = 29 in magnitude, so a weight is off by about 29 * 2^-24 = 2e-6 relative, and
so is a sum of up to 200 of them (all positive).  Where the reference's first and second (for top-1) or fifth and sixth (for top-5)
class score are closer than 1e-4 relative to the larger one, the row is not compared; at most 2 rows per case and k may be left out
that way (the fp64 reference alone leaves out at most 1 for seeds 0-4 on the first three shapes).  Counters are compared with the
sums of the returned ranks, exactly, no row left out."""
import functools
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import knn_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
NAN = float("nan")
T = 0.07
# B, N, D, C, noise, seed
CASES = [(67, 3001, 64, 20, 4.0, 0), (33, 1000, 136, 7, 3.0, 0), (40, 777, 768, 1000, 4.0, 0), (1, 200, 64, 5, 4.0, 0),
         (1, 201, 64, 5, 4.0, 0)]
IDS = ["67x3001x64", "33x1000x136", "40x777x768", "1x200x64", "1x201x64"]
SPLITS = [0, 1, 3, 64]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _sliced(x, pad=8, off=4):
    """x on the GPU as a column slice (offset `off`, row stride D + pad) of a wider NaN-poisoned matrix"""
    wide = torch.full((x.shape[0], x.shape[1] + pad), NAN, dtype=F32)
    wide[:, off:off + x.shape[1]] = x
    return wide.to(DEV)[:, off:off + x.shape[1]]


@functools.lru_cache(maxsize=None)
def clustered_case(B, N, D, C, noise, seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(C, D, generator=g)
    labels = torch.randint(0, C, (N,), generator=g)
    targets = torch.randint(0, C, (B,), generator=g)
    bank = F.normalize(centres[labels] + noise * torch.randn(N, D, generator=g), dim=1)
    queries = F.normalize(centres[targets] + noise * torch.randn(B, D, generator=g), dim=1)
    return queries, bank, labels, targets


@functools.lru_cache(maxsize=None)
def dyadic_case(B, N, D, C, seed):
    """entries k / 8, |k| <= 4: every product is a multiple of 1 / 64 and every partial sum stays below 64 / 4 = 16 in magnitude, so a
    similarity is exact in fp32 whatever the order, and equal similarities are frequent"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-4, 5, (B, D), generator=g).to(F32) / 8
    x = torch.randint(-4, 5, (N, D), generator=g).to(F32) / 8
    return q, x, torch.randint(0, C, (N,), generator=g), torch.randint(0, C, (B,), generator=g)


def gemm_sims(q, x):
    """the oracle: ops.gemm_nt_f32(Q, X padded to a multiple of 8 rows), pad columns dropped; on the CPU"""
    from vtp_amd import ops
    N = x.shape[0]
    xp = torch.zeros(ops.pad8(N), x.shape[1], dtype=F32)
    xp[:N] = x
    out = torch.full((q.shape[0], xp.shape[0]), NAN, device=DEV)
    ops.gemm_nt_f32(q.to(DEV).contiguous(), xp.to(DEV), out)
    return out.cpu()[:, :N].contiguous()


@functools.lru_cache(maxsize=None)
def oracle(case):
    """(S, -S sorted: the order of every bank row per query) of a clustered case, computed once"""
    q, x, _, _ = clustered_case(*case)
    S = gemm_sims(q, x)
    return S, torch.sort(-S, dim=1, stable=True).indices


def empty_lists(B, K):
    return torch.full((B, K), -float("inf"), device=DEV), torch.full((B, K), -1, device=DEV, dtype=I64)


def run_topk(q, chunks, K, splits=0, sims_out=None):
    """q [B, D] and chunks = [(bank rows on the device, index_base), ...] -> the lists on the CPU"""
    from vtp_amd import ops
    B = q.shape[0]
    sims, idx = empty_lists(B, K)
    ws = torch.empty(ops.knn_workspace_bytes(B, K, splits), device=DEV, dtype=torch.uint8)
    for x, base in chunks:
        ops.knn_topk(q, x, base, K, sims, idx, ws, splits, sims_out)
    return sims.cpu(), idx.cpu()


def bits(t):
    return t.contiguous().view(I32)


def same(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------- 1. neighbours, exact
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_neighbours_equal_the_host_sort_of_the_gemm(case):
    _gpu()
    B, N = case[0], case[1]
    q, x, _, _ = clustered_case(*case)
    S, order = oracle(case)
    qd, xd = q.to(DEV), x.to(DEV)
    for K in sorted({min(k, N) for k in (1, 5, 200, 256)}):
        want = (torch.gather(S, 1, order[:, :K]), order[:, :K])
        for splits in SPLITS:
            dump = torch.full((B, N + 3), NAN, device=DEV)
            got = run_topk(qd, [(xd, 0)], K, splits, dump[:, :N])
            assert same(got, want), (K, splits)
            assert torch.equal(bits(dump[:, :N].cpu()), bits(S)) and bool(dump[:, N:].isnan().all()), (K, splits)


# ---------------------------------------------------------------------------------------------------------------- 2. chunking and layout
def test_chunks_layouts_and_batches_give_the_same_lists():
    _gpu()
    case = CASES[0]
    B, N, D = case[:3]
    q, x, _, _ = clustered_case(*case)
    S, order = oracle(case)
    K = 200
    want = (torch.gather(S, 1, order[:, :K]), order[:, :K])
    qd, xd = q.to(DEV), x.to(DEV)
    for cuts in ([0, 1000, N], [0, 130, 131, 900, 1411, 2000, 2999, N]):
        chunks = [(xd[a:b], a) for a, b in zip(cuts, cuts[1:])]
        for splits in (0, 3):
            assert same(run_topk(qd, chunks, K, splits), want), (cuts, splits)
        assert same(run_topk(qd, chunks[::-1], K, 1), want), cuts  # the order of the chunks does not matter either
    # a global index: the whole bank at a large base
    base = (1 << 33) + 5
    got = run_topk(qd, [(xd, base)], K)
    assert same((got[0], got[1] - base), want)
    # queries and bank as column slices of wider matrices
    assert same(run_topk(_sliced(q), [(_sliced(x, pad=12, off=8), 0)], K, 3), want)
    # 61 more queries appended: the first 67 rows do not change
    g = torch.Generator().manual_seed(1)
    q128 = torch.cat([q, F.normalize(torch.randn(128 - B, D, generator=g), dim=1)])
    for splits in (0, 3):
        s128, i128 = run_topk(q128.to(DEV), [(xd, 0)], K, splits)
        assert same((s128[:B], i128[:B]), want), splits


def test_a_split_without_a_tile_changes_nothing():
    """81 tiles in one row block: the heuristic (splits=0) takes 9 splits of 9 tiles -- it drops the split that 10 splits of 9 tiles
    leave without a tile -- and a forced count of 10 launches that empty split.  Both give the lists of a single split."""
    _gpu()
    case = (5, 10300, 8, 5, 4.0, 2)
    K = 10
    q, x, _, _ = clustered_case(*case)
    S, order = oracle(case)
    want = (torch.gather(S, 1, order[:, :K]), order[:, :K])
    qd, xd = q.to(DEV), x.to(DEV)
    for splits in (0, 1, 10):
        assert same(run_topk(qd, [(xd, 0)], K, splits), want), splits


# ---------------------------------------------------------------------------------------------------------------- 3. ties
def test_exact_ties_follow_the_bank_index():
    _gpu()
    B, N, D = 33, 1500, 64
    q, x, _, _ = dyadic_case(B, N, D, 10, 0)
    S64 = q.double() @ x.double().T
    S = gemm_sims(q, x)
    assert torch.equal(S.double(), S64)  # exact in fp32
    order = torch.sort(-S, dim=1, stable=True).indices
    qd, xd = q.to(DEV), x.to(DEV)
    for K in (10, 200):
        sorted_s = torch.gather(S, 1, order)
        tied = int((sorted_s[:, K - 1] == sorted_s[:, K]).sum())
        print(f"KNN ties: {tied} of {B} rows have equal similarities across the boundary at K = {K}")
        assert tied >= min(B, 2)
        want = (sorted_s[:, :K].contiguous(), order[:, :K])
        for splits in SPLITS:
            assert same(run_topk(qd, [(xd, 0)], K, splits), want), (K, splits)
        assert same(run_topk(qd, [(xd[:700], 0), (xd[700:], 700)], K, 3), want), K


# ---------------------------------------------------------------------------------------------------------------- 4. votes
def run_vote(sims, idx, labels, targets, ks, C, counts=None):
    from vtp_amd import ops
    B, nk = sims.shape[0], len(ks)
    counts = torch.zeros(nk, 3, device=DEV, dtype=I64) if counts is None else counts
    rank = torch.full((B, nk), -7, device=DEV, dtype=I32)
    pred = torch.full((B, nk, 5), -7, device=DEV, dtype=I32)
    ops.knn_vote(sims.to(DEV), idx.to(DEV), labels.to(DEV, I32), targets.to(DEV, I64), ks, 1.0 / T, C, counts, rank, pred)
    return counts, rank.cpu(), pred.cpu()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_votes_against_the_fp64_restatement(case):
    _gpu()
    B, N, D, C = case[:4]
    q, x, labels, targets = clustered_case(*case)
    ks = tuple(k for k in (10, 20, 100, 200) if k <= N)
    K = ks[-1]
    sims, idx = run_topk(q.to(DEV), [(x.to(DEV), 0)], K)
    counts, rank, pred = run_vote(sims, idx, labels, targets, ks, C)
    want_rank, want_pred, gap1, gap5 = R.vote(sims.double(), labels[idx], targets, ks, T, C)
    out1, out5 = R.close(gap1), R.close(gap5)
    for m, k in enumerate(ks):
        left_out = int((out1[:, m] | out5[:, m]).sum())
        print(f"KNN votes {IDS[CASES.index(case)]} k={k}: top-1 {int((rank[:, m] < 1).sum())} top-5 {int((rank[:, m] < 5).sum())} of {B}, "
              f"rows left out {left_out}, rank mismatches {int((rank[:, m] != want_rank[:, m]).sum())}")
        assert left_out <= 2, (k, left_out)
        keep1, keep5 = ~out1[:, m], ~out5[:, m]
        assert torch.equal((rank[:, m] < 1)[keep1], (want_rank[:, m] < 1)[keep1]), k
        assert torch.equal((rank[:, m] < 5)[keep5], (want_rank[:, m] < 5)[keep5]), k
        assert torch.equal(pred[:, m, 0][keep1], want_pred[:, m, 0][keep1]), k
    assert torch.equal(counts.cpu(), R.counts_of(rank))
    # a second call adds to the counters; the run repeats bit for bit
    counts2, rank2, pred2 = run_vote(sims, idx, labels, targets, ks, C, counts)
    assert counts2 is counts and torch.equal(counts.cpu(), 2 * R.counts_of(rank))
    assert torch.equal(rank2, rank) and torch.equal(pred2, pred)


def test_targets_out_of_range_are_misses_and_rows():
    _gpu()
    case = CASES[1]
    B, N, D, C = case[:4]
    q, x, labels, targets = clustered_case(*case)
    ks = (10, 20, 100, 200)
    sims, idx = run_topk(q.to(DEV), [(x.to(DEV), 0)], 200)
    _, rank, _ = run_vote(sims, idx, labels, targets, ks, C)
    t2 = targets.clone()
    t2[0], t2[1] = -1, C
    counts2, rank2, _ = run_vote(sims, idx, labels, t2, ks, C)
    assert rank2[:2].tolist() == [[C] * 4, [C] * 4] and torch.equal(rank2[2:], rank[2:])
    assert torch.equal(counts2.cpu(), R.counts_of(rank2)) and counts2[:, 2].tolist() == [B] * 4
    want_rank, _, _, _ = R.vote(sims.double(), labels[idx], t2, ks, T, C)
    assert want_rank[:2].tolist() == [[C] * 4, [C] * 4]


# ---------------------------------------------------------------------------------------------------------------- 5. exact vote ties
def test_exact_vote_ties_and_targets_without_a_neighbour():
    _gpu()
    C, ks = 9, (2, 4)
    sims = torch.tensor([[0.5, 0.5, 0.25, 0.25]] * 4, dtype=F32)
    idx = torch.tensor([[0, 1, 2, 3]] * 4, dtype=I64)
    labels = torch.tensor([6, 2, 6, 2])  # per class one neighbour at 0.5 and one at 0.25: equal scores at both k
    targets = torch.tensor([6, 2, 4, 8])
    counts, rank, pred = run_vote(sims, idx, labels, targets, ks, C)
    want_rank, want_pred, _, _ = R.vote(sims.double(), labels[idx], targets, ks, T, C)
    # the lower class index wins the tie; a target without a neighbour: (classes seen) + target - (classes seen below it)
    assert rank.tolist() == [[1, 1], [0, 0], [2 + 4 - 1, 2 + 4 - 1], [2 + 8 - 2, 2 + 8 - 2]]
    assert pred[0].tolist() == [[2, 6, 0, 1, 3], [2, 6, 0, 1, 3]]
    assert torch.equal(rank, want_rank) and torch.equal(pred, want_pred)
    assert counts.cpu().tolist() == [[1, 2, 4], [1, 2, 4]]


# ---------------------------------------------------------------------------------------------------------------- 6. through the class
def test_through_the_class():
    _gpu()
    from vtp_amd import Knn
    from vtp_amd.zeroshot import percent
    case = CASES[0]
    B, N, D, C = case[:4]
    q, x, labels, targets = clustered_case(*case)
    ks = (10, 20, 100, 200)
    sims, idx = run_topk(q.to(DEV), [(x.to(DEV), 0)], 200)
    _, rank, pred = run_vote(sims, idx, labels, targets, ks, C)
    want = {k: tuple(int(v) for v in row) for k, row in zip(ks, R.counts_of(rank))}
    # un-normalised rows in, three uneven calls, a buffer that has to grow twice, chunks and query passes that divide nothing
    g = torch.Generator().manual_seed(2)
    scale_x, scale_q = torch.rand(N, 1, generator=g) * 3 + 0.5, torch.rand(B, 1, generator=g) * 3 + 0.5
    xs, qs = (x * scale_x).to(DEV), (q * scale_q).to(DEV)
    knn = Knn(None, num_classes=C, ks=ks, temperature=T, capacity=1024, chunk_rows=777, query_rows=50)
    with pytest.raises(RuntimeError, match="nothing evaluated"):
        knn.accuracy()
    knn.add_bank_features(xs[:100], labels[:100].to(DEV))
    with pytest.raises(RuntimeError, match="fewer than max"):
        knn.update_features(qs, targets.to(DEV))
    knn.add_bank_features(xs[100:1901], labels[100:1901].to(DEV))
    knn.add_bank_features(xs[1901:], labels[1901:].to(DEV))
    assert knn.size == N and knn.bank.shape == (N, D) and knn.capacity == 4096
    ref = Knn(None, num_classes=C, ks=ks, temperature=T)
    ref.add_bank_features(F.normalize(xs, dim=1), labels.to(DEV))
    # a priori: a computed norm is within gamma_{D+2} of the true one and the division rounds once more, so normalising a normalised
    # row again moves an entry (below 1 in magnitude) by less than (D + 4) u, u = 2^-24
    bound = (D + 4) * 2.0 ** -24
    assert float((knn.bank - ref.bank).abs().max()) <= bound and torch.equal(knn.bank_labels.cpu(), labels.to(I32))
    assert float((knn.bank.double().norm(dim=1) - 1).abs().max()) <= bound
    so, io = torch.full((B, 200), NAN, device=DEV), torch.full((B, 200), -7, device=DEV, dtype=I64)
    ro, po = torch.full((B, 4), -7, device=DEV, dtype=I32), torch.full((B, 4, 5), -7, device=DEV, dtype=I32)
    assert knn.update_features(qs, targets.to(DEV), sims_out=so, idx_out=io, rank_out=ro, pred_out=po) is None
    ref.update_features(F.normalize(qs, dim=1), targets.to(DEV))
    assert knn.counts() == ref.counts()
    got = knn.counts()
    assert got == {k: tuple(int(v) for v in row) for k, row in zip(ks, R.counts_of(ro.cpu()))}
    assert knn.accuracy() == {k: (percent(c1, n), percent(c5, n)) for k, (c1, c5, n) in got.items()}
    # against the kernels driven by hand on the host-normalised rows: the device normalisation may differ from F.normalize on the CPU
    # in the last bit, so lists are compared by index where the similarities are well apart and the counters are printed
    print(f"KNN class counts {got} by hand {want}; lists differ in {int((io.cpu() != idx).sum())} of {idx.numel()} places")
    with pytest.raises(RuntimeError, match="reset"):
        knn.add_bank_features(xs[:8], labels[:8].to(DEV))
    knn.update_features(qs, targets.to(DEV))
    assert knn.counts() == {k: (2 * c1, 2 * c5, 2 * n) for k, (c1, c5, n) in got.items()}
    knn.reset()
    assert knn.counts() == {k: (0, 0, 0) for k in ks} and knn.size == N
    knn.update_features(qs, targets.to(DEV), splits=3)
    assert knn.counts() == got
    with pytest.raises(ValueError, match="no CPU path"):
        knn.update_features(qs.cpu(), targets.to(DEV))
    with pytest.raises(ValueError, match="integer class indices"):
        knn.update_features(qs, targets[:5].to(DEV))


# ---------------------------------------------------------------------------------------------------------------- 7. through the model
def test_through_the_model(golden_sd):
    _gpu()
    from oracle.ref_stubs import TINY
    from vtp_amd import Knn, VTPConfig, VTPModel
    model = VTPModel(VTPConfig(**TINY))
    model.load_state_dict(golden_sd, strict=True)
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    size, C, ks = TINY["image_size"], 5, (1, 5)
    bank_im, query_im = torch.randn(24, 3, size, size, generator=g).to(DEV), torch.randn(8, 3, size, size, generator=g).to(DEV)
    bank_y, query_y = torch.randint(0, C, (24,), generator=g).to(DEV), torch.randint(0, C, (8,), generator=g).to(DEV)
    knn = Knn(model, num_classes=C, ks=ks)
    knn.add_bank(bank_im[:10], bank_y[:10])
    knn.add_bank(bank_im[10:], bank_y[10:])
    knn.update(query_im[:3], query_y[:3])
    knn.update(query_im[3:], query_y[3:])
    by_model = knn.counts()
    assert [v[2] for v in by_model.values()] == [8, 8]
    feats = Knn(None, num_classes=C, ks=ks)
    with torch.no_grad():
        feats.add_bank_features(model.get_last_layer_feature(bank_im)["cls_token"], bank_y)
        feats.update_features(model.get_last_layer_feature(query_im)["cls_token"], query_y)
    assert feats.counts() == by_model
    # feature_fn replaces the class token
    pooled = Knn(model, num_classes=C, ks=ks, feature_fn=lambda m, im: m.get_last_layer_feature(im)["patch_tokens"].mean(1))
    pooled.add_bank(bank_im, bank_y)
    pooled.update(query_im, query_y)
    assert [v[2] for v in pooled.counts().values()] == [8, 8]
    with pytest.raises(ValueError, match="MI355X"):
        knn.update(query_im.cpu(), query_y)


# ---------------------------------------------------------------------------------------------------------------- 8. two ranks
TWO = (66, 1000, 64, 10, 0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from vtp_amd import Knn
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    q, x, labels, targets = dyadic_case(*TWO)
    knn = Knn(None, num_classes=TWO[3], ks=(10, 100), group=dist.group.WORLD)
    knn.add_bank_features(x.to(DEV), labels.to(DEV))  # every rank holds the whole bank
    half = TWO[0] // world
    sl = slice(rank * half, (rank + 1) * half)
    knn.update_features(q[sl].to(DEV), targets[sl].to(DEV))
    out[rank] = (knn.counts(), knn.accuracy())
    dist.destroy_process_group()


def test_two_ranks_sum_to_the_single_process_counts():
    _gpu()
    from vtp_amd import Knn
    q, x, labels, targets = dyadic_case(*TWO)
    knn = Knn(None, num_classes=TWO[3], ks=(10, 100))
    knn.add_bank_features(x.to(DEV), labels.to(DEV))
    knn.update_features(q.to(DEV), targets.to(DEV))
    one, acc = knn.counts(), knn.accuracy()
    assert [v[2] for v in one.values()] == [TWO[0]] * 2
    del knn
    torch.cuda.empty_cache()
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        assert out[r] == (one, acc)
