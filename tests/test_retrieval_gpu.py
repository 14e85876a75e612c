"""GPU: the retrieval kernels (csrc/retrieval.hip: vtp_retr_best / vtp_retr_rank / vtp_retr_count) and vtp_amd.Retrieval.

Every comparison is integer or bitwise; there are no tolerances.  The oracle of the similarities is ops.gemm_nt_f32 (the gallery
zero-padded to a multiple of 8 rows, the pad columns dropped): the kernels promise the bits of that kernel.  Ranks are compared with
tests/retrieval_ref.py evaluated on exactly those values.

The kernel cases use entries that are multiples of 2^-2 (so of 2^-6) in [-1, 1]: every product is a multiple of 2^-4, every chain of
up to 768 terms is exact in fp32 whatever the order, and equal similarities are common.  Gallery rows 150 and 299 are copies of row
3, row 128 of row 127; queries 0 .. 4 are gallery rows 0 .. 4 and query 130 is gallery row 200."""
import functools
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

import retrieval_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
NAN, NEG = float("nan"), float("-inf")
DS, BS, NS, SPLITS = [8, 24, 40, 768], [1, 127, 129, 260], [1, 127, 129, 300], [1, 3, 0]
LENS = [0, 1, 5, 17]
KS = (1, 5, 10)


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
def case(D):
    """(queries f32 [260, D], gallery f32 [300, D]) on the CPU; the sub-cases take the leading rows"""
    g = torch.Generator().manual_seed(D)
    x = R.dyadic((300, D), g)
    q = R.dyadic((260, D), g)
    x[150] = x[3]
    x[299] = x[3]
    x[128] = x[127]
    q[:5] = x[:5]
    q[130] = x[200]
    return q, x


@functools.lru_cache(maxsize=None)
def on_device(D):
    q, x = case(D)
    return q.to(DEV), x.to(DEV)


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
def oracle(D):
    """the [260, 300] similarities of the case, computed once; every sub-case is a corner of it (an element of the GEMM does not
    depend on the other rows) and is exact, so it equals the integer arithmetic as well"""
    q, x = case(D)
    S = gemm_sims(q, x)
    assert torch.equal(S.to(F64), R.sims_64(q, x))
    return S


@functools.lru_cache(maxsize=None)
def lists_of(B, N, seed=0):
    """ground-truth lists of length 0, 1, 5, 17 in turn: rows of [0, N) and, now and then, an index outside it"""
    g = torch.Generator().manual_seed(1000 * B + N + seed)
    out = []
    for b in range(B):
        l = torch.randint(0, N, (LENS[(b + 1) % 4],), generator=g).tolist()
        if b % 7 == 3 and l:
            l[len(l) // 2] = N + b % 3   # past the end
            l.append(-1 - b % 2)         # negative
        out.append(l)
    if B > 8 and N == 300:
        out[5] = [299, 150, 3]                      # equal ground-truth rows: the lower index is the best
        out[6] = [N - 1]                            # the best row lies in the last chunk
        out[130 if B > 130 else 7] = [0, N - 1, N // 2]
    return out


def csr_on_device(lists):
    ptr, idx = R.csr(lists)
    return ptr.to(DEV), idx.to(DEV)


def run_best(q, x, lists):
    from vtp_amd import ops
    B = q.shape[0]
    ptr, idx = csr_on_device(lists)
    bs = torch.full((B + 2,), NAN, device=DEV)
    bj = torch.full((B + 2,), -7, device=DEV, dtype=I64)
    ops.retr_best(q, x, ptr, idx, bs[:B], bj[:B])
    assert bool(bs[B:].isnan().all()) and bj[B:].tolist() == [-7, -7]
    return bs[:B].contiguous(), bj[:B].contiguous()


def run_rank(q, chunks, bs, bj, splits=0, sims_out=None, start=0):
    """chunks = [(gallery rows on the device, index_base), ...] -> beats on the CPU"""
    from vtp_amd import ops
    beats = torch.full((q.shape[0],), start, device=DEV, dtype=I32)
    for x, base in chunks:
        ops.retr_rank(q, x, base, bs, bj, beats, splits, sims_out)
    return beats.cpu()


def steps_of(n, step):
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def cuts_of(n, parts):
    return steps_of(n, -(-n // parts))


# ---------------------------------------------------------------------------------------------------------------- 1. every shape
@pytest.mark.parametrize("D", DS)
def test_similarities_best_and_beats_at_every_shape(D):
    _gpu()
    S = oracle(D)
    qd, xd = on_device(D)
    for B in BS:
        for N in NS:
            lists = lists_of(B, N)
            want_s, want_j = R.best_of(S[:B, :N], lists)
            bs, bj = run_best(qd[:B], xd[:N], lists)
            assert same_bits(bs.cpu(), want_s) and torch.equal(bj.cpu(), want_j), (B, N)
            want = R.rank_by_sort(S[:B, :N], lists)
            for splits in SPLITS:
                dump = torch.full((B, N + 3), NAN, device=DEV)
                beats = run_rank(qd[:B], [(xd[:N], 0)], bs, bj, splits, dump[:, :N])
                got_S = dump[:, :N].cpu()
                assert same_bits(got_S, S[:B, :N]) and bool(dump[:, N:].isnan().all()), (B, N, splits)
                assert torch.equal(beats, R.rank_by_count(got_S, bs.cpu(), bj.cpu())), (B, N, splits)
                assert torch.equal(beats, want), (B, N, splits)
    # column slices of wider NaN-poisoned matrices
    q, x = case(D)
    lists = lists_of(129, 300)
    bs, bj = run_best(sliced(q[:129]), sliced(x), lists)
    assert torch.equal(run_rank(sliced(q[:129]), [(sliced(x), 0)], bs, bj, 3), R.rank_by_sort(S[:129], lists))


# ---------------------------------------------------------------------------------------------------------------- 2. the best ground truth
def test_best_on_long_lists_empty_lists_and_block_edges():
    """lists longer than a round of 64 pairs, lists that straddle the workgroups' ranges, runs of empty lists in front, in the middle
    and at the end, with the pair count an exact multiple of 64 (the trailing empty queries belong to a workgroup without pairs)"""
    _gpu()
    D = 40
    S = oracle(D)
    qd, xd = on_device(D)
    g = torch.Generator().manual_seed(5)
    rnd = lambda n: torch.randint(0, 300, (n,), generator=g).tolist()
    lists = [[], [], [], rnd(150), rnd(1), rnd(5), rnd(17), []] + [[] for _ in range(70)] + [rnd(63), rnd(65), rnd(19), [], [], []]
    # query 3 is gallery row 3, and row 150 is a copy of it: equal rows inside a long list, the lower index in a later round
    lists[3][10], lists[3][100] = 150, 3
    assert sum(len(l) for l in lists) == 320
    B = len(lists)
    want_s, want_j = R.best_of(S[:B], lists)
    bs, bj = run_best(qd[:B], xd, lists)
    assert same_bits(bs.cpu(), want_s) and torch.equal(bj.cpu(), want_j) and int(bj[3]) == 3
    assert (bj.cpu() < 0).tolist() == [not l for l in lists] and bool((bs.cpu()[bj.cpu() < 0] == NEG).all())
    # all empty: no pairs at all
    bs, bj = run_best(qd[:B], xd, [[] for _ in range(B)])
    assert bool((bs == NEG).all()) and bool((bj == -1).all())
    assert torch.equal(run_rank(qd[:B], [(xd, 0)], bs, bj), torch.full((B,), 300, dtype=I32))
    # one entry per query (every caption has one image) and the whole gallery per query
    one = [[(7 * b) % 300] for b in range(260)]
    bs, bj = run_best(qd, xd, one)
    assert torch.equal(bj.cpu(), torch.tensor([l[0] for l in one])) and same_bits(bs.cpu(), S[torch.arange(260), bj.cpu()])
    every = [list(range(299, -1, -1)) for _ in range(3)]
    bs, bj = run_best(qd[:3], xd, every)
    top = torch.sort(-S[:3], dim=1, stable=True).indices[:, 0]
    assert torch.equal(bj.cpu(), top) and torch.equal(run_rank(qd[:3], [(xd, 0)], bs, bj), torch.zeros(3, dtype=I32))


# ---------------------------------------------------------------------------------------------------------------- 3. chunks, passes, splits
def test_chunks_passes_and_splits_give_the_same_ranks():
    _gpu()
    D, B, N = 40, 260, 300
    S = oracle(D)
    qd, xd = on_device(D)
    lists = lists_of(B, N)
    want = R.rank_by_sort(S, lists)
    bs, bj = run_best(qd, xd, lists)
    assert int(bj[6]) == N - 1 and int(bj[5]) == 3  # a best row in the last chunk; equal ground-truth rows resolve to the lower index
    assert len(set(want.tolist())) > 10 and int((want == N).sum()) == sum(1 for l in lists if not [j for j in l if 0 <= j < N])
    for parts in (1, 2, 7):
        chunks = [(xd[a:b], a) for a, b in cuts_of(N, parts)]
        for rows in (64, 128, B):
            for splits in SPLITS:
                got = torch.cat([run_rank(qd[a:b], chunks, bs[a:b], bj[a:b], splits) for a, b in steps_of(B, rows)])
                assert torch.equal(got, want), (parts, rows, splits)
    # beats accumulates: a buffer that starts at 5, and the chunks in reverse order
    chunks = [(xd[a:b], a) for a, b in reversed(cuts_of(N, 7))]
    assert torch.equal(run_rank(qd, chunks, bs, bj, start=5), want + 5)
    # the global index decides ties: the same chunk under another index_base counts differently around the best row
    got = run_rank(qd[:5], [(xd, 1000)], bs[:5], bj[:5])
    assert torch.equal(got, R.rank_by_count(S[:5], bs[:5].cpu(), bj[:5].cpu(), index_base=1000))


# ---------------------------------------------------------------------------------------------------------------- 4. counters
def test_counts_match_the_host_and_the_rank_buffer_is_filled_at_an_offset():
    _gpu()
    from vtp_amd import ops
    D, B, N = 24, 260, 300
    S = oracle(D)
    qd, xd = on_device(D)
    lists = lists_of(B, N)
    want = R.rank_by_sort(S, lists)
    assert not lists[3] and int(want[3]) == N  # a query without ground truth: rank N, a row and a miss
    bs, bj = run_best(qd, xd, lists)
    beats = run_rank(qd, [(xd, 0)], bs, bj).to(DEV)
    for ks in (KS, (1,), (1, 2, 3, 5, 10, 50, 300, 301)):
        counts = torch.zeros(len(ks) + 1, device=DEV, dtype=I64)
        rank = torch.full((B + 10,), -7, device=DEV, dtype=I32)
        ops.retr_count(beats, ks, counts, rank, 4)
        assert torch.equal(counts.cpu(), R.counts_of(want, ks)), ks
        assert torch.equal(rank[4:4 + B].cpu(), want) and bool((rank[:4] == -7).all()) and bool((rank[4 + B:] == -7).all())
        # in two passes into the same counters and the same buffer, and without a buffer
        counts.zero_()
        rank.fill_(-7)
        ops.retr_count(beats[:129], ks, counts, rank, 0)
        ops.retr_count(beats[129:], ks, counts, rank, 129)
        assert torch.equal(counts.cpu(), R.counts_of(want, ks)) and torch.equal(rank[:B].cpu(), want)
        ops.retr_count(beats, ks, counts)
        assert torch.equal(counts.cpu(), 2 * R.counts_of(want, ks))
    c = R.counts_of(want, (1, 300, 301))
    assert c[1] < B and c[2] == B == c[3]  # rank N is a miss at K = N and a row


# ---------------------------------------------------------------------------------------------------------------- 5. through the class
N_IMG, PER = 12, 5


@functools.lru_cache(maxsize=None)
def captioned_set():
    """12 images with 5 captions each: image ids that are neither sorted nor contiguous, the captions shuffled"""
    from oracle.ref_stubs import TINY
    g = torch.Generator().manual_seed(11)
    images = torch.randn(N_IMG, 3, TINY["image_size"], TINY["image_size"], generator=g)
    tokens = torch.randint(1, TINY["text_vocab_size"] - 1, (N_IMG * PER, TINY["text_context_length"]), generator=g)
    img_ids = torch.tensor([901, 17, 4000000000, 3, 52, 77, 500, 12, 8, 1000, 41, 64])[torch.randperm(N_IMG, generator=g)]
    txt_ids = img_ids.repeat_interleave(PER)[torch.randperm(N_IMG * PER, generator=g)]
    return images, img_ids, tokens, txt_ids


def reference_on(img, img_ids, txt, txt_ids, ks=KS):
    """both directions by the sort statement, on the similarities of the GEMM oracle"""
    out, ranks = {}, {}
    for name, (q, qi, x, xi) in {"image_to_text": (img, img_ids, txt, txt_ids), "text_to_image": (txt, txt_ids, img, img_ids)}.items():
        ranks[name] = R.rank_by_sort(gemm_sims(q, x), R.gt_lists(qi, xi))
        out[name] = R.summary(ranks[name], ks)
    return out, ranks


def test_through_the_class_on_a_tiny_model(golden_sd):
    _gpu()
    from oracle.ref_stubs import TINY
    from vtp_amd import Retrieval, VTPConfig, VTPModel
    images, img_ids, tokens, txt_ids = captioned_set()
    model = VTPModel(VTPConfig(**TINY))
    model.load_state_dict(golden_sd, strict=True)
    model = model.to(DEV).eval()
    r = Retrieval(model, ks=KS)
    for a, b in ((0, 1), (1, 8), (8, N_IMG)):  # uneven calls; the banks start at one row and grow
        r.add_images(images[a:b].to(DEV), img_ids[a:b].to(DEV))
    for a, b in ((0, 33), (33, 34), (34, N_IMG * PER)):
        r.add_texts(tokens[a:b].to(DEV), txt_ids[a:b].to(DEV))
    out = r.result()
    img, txt = r.rows("image").cpu(), r.rows("text").cpu()
    assert img.shape[0] == N_IMG and txt.shape[0] == N_IMG * PER and img.shape[1] == txt.shape[1] and img.dtype == F32
    assert torch.equal(r.ids("image").cpu(), img_ids) and torch.equal(r.ids("text").cpu(), txt_ids)
    with torch.no_grad():
        assert same_bits(img[1:8], model.get_clip_image_feature(images[1:8].to(DEV), normalize=True).float().cpu())
        assert same_bits(txt[34:], model.get_clip_text_feature(tokens[34:].to(DEV), normalize=True).float().cpu())
    want, want_ranks = reference_on(img, img_ids, txt, txt_ids)
    assert out == want, (out, want)
    assert set(out) == {"image_to_text", "text_to_image"} and set(out["image_to_text"]) == {"R@1", "R@5", "R@10", "counts", "rows", "median_rank",
                                                                                         "mean_rank"}
    assert out["image_to_text"]["rows"] == N_IMG and out["text_to_image"]["rows"] == N_IMG * PER
    galleries = {"image_to_text": (img_ids, txt_ids), "text_to_image": (txt_ids, img_ids)}
    for name, (qi, xi) in galleries.items():
        ranks = r.ranks(name)
        assert ranks.dtype == I32 and ranks.is_cuda and torch.equal(ranks.cpu(), want_ranks[name]), name
        # rank < k exactly when the first k neighbours of the independent vtp_knn_topk hold a ground-truth row
        for k in (1, 5, 10, 12):
            top = r.top(name, k).cpu()
            assert top.shape == (qi.shape[0], k) and top.dtype == I64
            hit = (xi[top] == qi[:, None]).any(1)
            assert torch.equal(hit, ranks.cpu() < k), (name, k)
    # a second result() gives the same bits
    first = {name: r.ranks(name).clone() for name in galleries}
    assert r.result() == out and all(torch.equal(r.ranks(name), first[name]) for name in galleries)
    # cached features: the same result, whatever the chunking and the passes
    for kw in (dict(), dict(chunk_rows=7, query_rows=5), dict(capacity=100, chunk_rows=1, query_rows=64)):
        c = Retrieval(None, ks=KS, **kw)
        c.add_image_features(sliced(img), img_ids.to(DEV))  # any layout is copied into the bank
        c.add_text_features(txt[:20].to(DEV), txt_ids[:20].to(DEV))
        c.add_text_features(txt[20:].to(DEV).double(), txt_ids[20:].to(DEV))  # any float type is cast to f32
        assert c.result() == out, kw
        assert all(torch.equal(c.ranks(name), first[name]) for name in galleries), kw
    # rows may be added after result(): a caption of an image the image bank does not hold is a miss and a row, an image without
    # a caption likewise
    c.add_text_features(txt[:1].to(DEV), torch.tensor([123456], device=DEV))
    c.add_image_features(img[:1].to(DEV), torch.tensor([-5], device=DEV))
    with pytest.raises(RuntimeError, match="after result"):
        c.ranks("image_to_text")
    more = c.result()
    want_more, ranks_more = reference_on(torch.cat([img, img[:1]]), torch.cat([img_ids, torch.tensor([-5])]), torch.cat([txt, txt[:1]]),
                                         torch.cat([txt_ids, torch.tensor([123456])]))
    assert more == want_more and int(c.ranks("text_to_image")[-1]) == N_IMG + 1 and int(c.ranks("image_to_text")[-1]) == N_IMG * PER + 1
    assert more["text_to_image"]["rows"] == N_IMG * PER + 1
    # the error cases: before any launch
    with pytest.raises(ValueError, match="no CPU path"):
        r.add_images(images[:1], img_ids[:1].to(DEV))
    with pytest.raises(ValueError, match="no CPU path"):
        r.add_texts(tokens[:1].to(DEV), txt_ids[:1])
    with pytest.raises(ValueError, match="must be 2 integers"):
        r.add_images(images[:2].to(DEV), img_ids[:3].to(DEV))
    with pytest.raises(ValueError, match="must be 2 integers"):
        r.add_images(images[:2].to(DEV), img_ids[:2].to(DEV).float())
    with pytest.raises(ValueError, match="multiple of 8"):
        c.add_image_features(torch.zeros(2, 12, device=DEV), img_ids[:2].to(DEV))
    with pytest.raises(ValueError, match="like the image bank"):
        c.add_text_features(torch.zeros(2, img.shape[1] + 8, device=DEV), img_ids[:2].to(DEV))
    with pytest.raises(ValueError, match="k must be"):
        r.top("image_to_text", N_IMG * PER + 1)
    c.reset()
    with pytest.raises(RuntimeError, match="image bank is empty"):
        c.result()


# ---------------------------------------------------------------------------------------------------------------- 6. two ranks
SHARDS = {"image": 5, "text": 41}  # rank 0 holds the rows in front of the cut, rank 1 the rest: uneven shards


def _features():
    """the cached features of a run that needs no model: dyadic rows of width 24 under the ids of the captioned set"""
    _, img_ids, _, txt_ids = captioned_set()
    g = torch.Generator().manual_seed(3)
    return R.dyadic((N_IMG, 24), g), img_ids, R.dyadic((N_IMG * PER, 24), g), txt_ids


def _summary(r):
    out = r.result()
    return out, {name: r.ranks(name).cpu().tolist() for name in out}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from vtp_amd import Retrieval
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    img, img_ids, txt, txt_ids = _features()
    r = Retrieval(None, ks=KS, group=dist.group.WORLD, query_rows=7)
    cut = {s: slice(0, SHARDS[s]) if rank == 0 else slice(SHARDS[s], None) for s in SHARDS}
    r.add_image_features(img[cut["image"]].to(DEV), img_ids[cut["image"]].to(DEV))
    r.add_text_features(txt[cut["text"]].to(DEV), txt_ids[cut["text"]].to(DEV))
    out[rank] = _summary(r)
    dist.destroy_process_group()


def test_two_ranks_equal_the_single_process_on_the_concatenation():
    _gpu()
    from vtp_amd import Retrieval
    img, img_ids, txt, txt_ids = _features()
    r = Retrieval(None, ks=KS)
    r.add_image_features(img.to(DEV), img_ids.to(DEV))
    r.add_text_features(txt.to(DEV), txt_ids.to(DEV))
    one = _summary(r)
    want, want_ranks = R.evaluate(img, img_ids, txt, txt_ids, KS)  # exact data: fp64 is the oracle
    assert one[0] == want and one[1] == {name: t.tolist() for name, t in want_ranks.items()}
    del r
    torch.cuda.empty_cache()
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for k in range(world):
        assert out[k] == one
