"""The k-NN manifold precision / recall of vtp_amd.PrecisionRecall (csrc/precision_recall.hip) restated on the CPU.  Not a test module;
imported by tests/test_precision_recall_host.py and tests/test_precision_recall_gpu.py.

    d2_64, radii_64, hits_64 : the fp64 restatement, with direct ((a - b)^2).sum() distances.
        radius of row i of X for neighbourhood size k = the k-th smallest of { d2(x_i, x_j) : j != i } (the row is excluded by
        index, not by value: a duplicate of x_i elsewhere counts, at distance 0);
        hits of a query q against (X, r2) = #{ j : d2(q, x_j) <= r2[j] };
        precision = the share of generated rows with a hit against (real rows, real radii), recall the same with the sets swapped.
    oracle32 : the kernels' formula max((n(a) + n(b)) - 2 s(a, b), 0) in torch fp32 on the host, one rounding per operation, from
        the products S and the norms that ops.gemm_nt_f32 formed (gemm_parts, on the GPU): the bit-exact oracle.
    lists32 / hits32 : the 8 smallest per row by a host sort, and the hit counts, of an oracle32 matrix.
    clustered, lowrank : the seeded generators of the test cases."""
import functools
import math

import torch

F32, F64 = torch.float32, torch.float64
MAX_K = 8

# the cases: (generator, arguments) -- shapes chosen for what can break: 257 and 129 put one row into a second 128-tile, 130 x 130
# makes a self-against-self pass cross the tile edge, D = 24 ends on a partial 16-slab, D = 8 is half a slab, D = 2048 is the
# production width, 40 queries are a partial row block
CASES = [("clustered", (300, 257, 64, 5, 1.0, 0.9, 0)), ("clustered", (129, 400, 24, 3, 0.7, 0.8, 1)),
         ("clustered", (130, 130, 8, 2, 0.5, 0.7, 3)), ("lowrank", (300, 257, 64, 4, 0.8, 0.3, 0)),
         ("lowrank", (40, 257, 2048, 6, 0.8, 0.3, 6))]
IDS = ["clustered-300x257x64", "clustered-129x400x24", "clustered-130x130x8", "lowrank-300x257x64", "lowrank-40x257x2048"]
# the fp64 restatement's counts, evaluated once on the CPU: {k: (generated covered, not covered, real covered, not covered)}
TABLE = [{1: (26, 231, 266, 34), 3: (70, 187, 296, 4)}, {1: (80, 320, 104, 25), 3: (176, 224, 122, 7)},
         {1: (43, 87, 77, 53), 3: (94, 36, 122, 8)}, {1: (203, 54, 162, 138), 3: (254, 3, 230, 70)},
         {1: (172, 85, 22, 18), 3: (232, 25, 25, 15)}]
FLOOR = 3  # every decision of a case that is compared leaves at least this many rows on each side


def clustered(Nr, Ng, D, C, noise, shift, seed):
    g = torch.Generator().manual_seed(seed)
    cen = torch.randn(C, D, generator=g)
    real = cen[torch.randint(0, C, (Nr,), generator=g)] + noise * torch.randn(Nr, D, generator=g)
    fake = cen[torch.randint(0, C, (Ng,), generator=g)] * shift + 1.15 * noise * torch.randn(Ng, D, generator=g)
    return real.contiguous(), fake.contiguous()


def lowrank(Nr, Ng, D, L, spread, shift, seed):
    """a D-dimensional set with few intrinsic dimensions, like Inception features (isotropic noise in 2048-d gives precision 0)"""
    g = torch.Generator().manual_seed(seed)
    P = torch.randn(L, D, generator=g) / math.sqrt(L)
    zr = torch.randn(Nr, L, generator=g)
    zg = spread * torch.randn(Ng, L, generator=g) + shift
    real = zr @ P + 0.02 * torch.randn(Nr, D, generator=g)
    fake = zg @ P + 0.02 * torch.randn(Ng, D, generator=g)
    return real.contiguous(), fake.contiguous()


@functools.lru_cache(maxsize=None)
def case(i):
    """(real, fake) f32 on the CPU of case i, generated once"""
    kind, args = CASES[i]
    return (clustered if kind == "clustered" else lowrank)(*args)


# ------------------------------------------------------------------------------------------------------------------ fp64
def d2_64(q, x):
    """[B, N] f64: ((q_b - x_n)^2).sum(), directly"""
    q, x = q.to(F64), x.to(F64)
    return ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)


def kth_other(d2, k, query_base=0, index_base=0):
    """per row b the k-th smallest of { d2[b, n] : query_base + b != index_base + n }; +inf where fewer than k remain"""
    B, N = d2.shape
    d = d2.clone()
    same = (torch.arange(B)[:, None] + query_base) == (torch.arange(N)[None, :] + index_base)
    d[same] = float("inf")
    if N < k:
        return torch.full((B,), float("inf"), dtype=d2.dtype)
    return torch.sort(d, dim=1).values[:, k - 1]


def radii_64(x, k):
    return kth_other(d2_64(x, x), k)


def hits_64(q, x, r2):
    """int64 [B]: #{ n : d2(q_b, x_n) <= r2[n] }"""
    return (d2_64(q, x) <= r2.to(F64)[None, :]).sum(1)


def pr_64(real, fake, k):
    """dict of the fp64 restatement: radii and hits of both sets and the four counts of the table"""
    rr, rf = radii_64(real, k), radii_64(fake, k)
    hf, hr = hits_64(fake, real, rr), hits_64(real, fake, rf)
    pc, rc = int((hf > 0).sum()), int((hr > 0).sum())
    return dict(radii_real=rr, radii_fake=rf, hits_fake=hf, hits_real=hr, counts=(pc, fake.shape[0] - pc, rc, real.shape[0] - rc),
                precision=pc / fake.shape[0], recall=rc / real.shape[0])


@functools.lru_cache(maxsize=None)
def case_64(i, k):
    return pr_64(*case(i), k)


def ks_of(i):
    """the neighbourhood sizes case i is compared at: 1 and 3, and 8 where the floor still holds"""
    return [k for k in (1, 3, 8) if k != 8 or min(case_64(i, 8)["counts"]) >= FLOOR]


# ------------------------------------------------------------------------------------------------------------------ fp32, bit-exact
def oracle32(S, qn, xn):
    """S f32 [B, N] (the products), qn f32 [B], xn f32 [N] (the norms), on the CPU -> d2 f32 [B, N] with the kernels' roundings: the
    sum of the norms rounds once, 2 * S is exact, the difference rounds once, negatives become 0 (a NaN stays a NaN)"""
    assert S.dtype == F32 and qn.dtype == F32 and xn.dtype == F32 and not S.is_cuda
    return ((qn[:, None] + xn[None, :]) - 2.0 * S).clamp_min(0.0)


def gemm_parts(q, x):
    """(S, qn, xn) on the CPU from ops.gemm_nt_f32 on the GPU: S = Q X^T with the bank padded to a multiple of 8 rows (pad columns
    dropped), norms = the diagonals of Q Q^T and X X^T"""
    from vtp_amd import ops

    def nt(a, b):
        n = b.shape[0]
        bp = torch.zeros(ops.pad8(n), b.shape[1], dtype=F32)
        bp[:n] = b
        out = torch.full((a.shape[0], bp.shape[0]), float("nan"), device="cuda")
        ops.gemm_nt_f32(a.to("cuda").contiguous(), bp.to("cuda"), out)
        return out.cpu()[:, :n].contiguous()

    same = q is x
    xn = nt(x, x).diagonal().contiguous()
    return nt(q, x), (xn if same else nt(q, q).diagonal().contiguous()), xn


def lists32(d2, query_base=-1, index_base=0):
    """f32 [B, 8]: per row the 8 smallest of d2 by a host sort, ascending, +inf for an empty entry; query_base >= 0 leaves out the
    pair with query_base + b == index_base + n"""
    B, N = d2.shape
    d = d2.clone()
    if query_base >= 0:
        same = (torch.arange(B)[:, None] + query_base) == (torch.arange(N)[None, :] + index_base)
        d[same] = float("inf")
    d = torch.cat([d, torch.full((B, MAX_K), float("inf"), dtype=d.dtype)], 1)
    return torch.sort(d, dim=1).values[:, :MAX_K].contiguous()


def hits32(d2, r2):
    """int32 [B]: #{ n : d2[b, n] <= r2[n] }"""
    return (d2 <= r2[None, :]).sum(1).to(torch.int32)
