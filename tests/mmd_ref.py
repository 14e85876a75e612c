"""The Kernel Inception Distance of vtp_amd.KID (csrc/mmd.hip) restated on the CPU.  Not a test module; imported by
tests/test_kid_host.py and tests/test_kid_gpu.py.

    kid_64      : the fp64 restatement: k = (x.y gamma + coef0)^degree from fp64 products, the unbiased estimator
                  MMD^2_u = Sxx / (m (m - 1)) + Syy / (n (n - 1)) - 2 Sxy / (m n) (Sxx, Syy over the ordered pairs i != j), and the
                  subset protocol with the draws of draws().
    oracle_part : the bit-exact oracle of vtp_mmd_poly_part from the fp32 products S that ops.gemm_nt_f32 formed on the GPU
                  (pr_ref.gemm_parts): the pair value in torch fp64 on the CPU, one rounding per operation, and the tile sums in the
                  order the kernel's header states -- TABLE maps (set, step) to the tile row -- by a loop over the 32 steps.
                  oracle_fold / oracle_total: the fold over tiles in ascending order and the neighbour-pair tree.
    bound       : the a-priori error bound of the fp32 chain against kid_64, evaluated in fp64.
    The cases and generators are those of pr_ref (imported, not copied)."""
import functools
import math

import torch

import pr_ref as R
from pr_ref import CASES, IDS, case, gemm_parts  # noqa: F401

F32, F64 = torch.float32, torch.float64
TILE = 128
U32, U64 = 2.0 ** -24, 2.0 ** -53
SUBSETS, SUBSET_SIZE = 3, 129      # the subset protocol of the tests
SUBSET_CASES = [0, 1, 2, 3]        # the cases whose two sets both hold 129 rows (case 4 has 40 real rows)


# ------------------------------------------------------------------------------------------------------------------ fp64
def draws(n_real, n_fake, subsets, subset_size, seed):
    """(real, fake) int64 [subsets, subset_size]: randperm(n)[:subset_size] from one generator, real then fake, subset by subset"""
    g = torch.Generator().manual_seed(seed)
    ri, fi = [], []
    for _ in range(subsets):
        ri.append(torch.randperm(n_real, generator=g)[:subset_size])
        fi.append(torch.randperm(n_fake, generator=g)[:subset_size])
    return torch.stack(ri), torch.stack(fi)


def kernel_64(a, b, gamma, coef0, degree):
    return ((a.to(F64) @ b.to(F64).T) * gamma + coef0) ** degree


def mmd2_64(x, y, gamma=None, coef0=1.0, degree=3):
    """the unbiased MMD^2 of the rows of x and y, a python float"""
    m, n = x.shape[0], y.shape[0]
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    kxx, kyy = kernel_64(x, x, gamma, coef0, degree), kernel_64(y, y, gamma, coef0, degree)
    kxx.fill_diagonal_(0.0)
    kyy.fill_diagonal_(0.0)
    kxy = kernel_64(x, y, gamma, coef0, degree)
    return float(kxx.sum() / (m * (m - 1)) + kyy.sum() / (n * (n - 1)) - 2.0 * kxy.sum() / (m * n))


def mean_std(vals):
    mean = math.fsum(vals) / len(vals)
    return mean, math.sqrt(math.fsum((v - mean) ** 2 for v in vals) / len(vals))


def kid_64(x, y, subsets=0, subset_size=1000, seed=0, gamma=None, coef0=1.0, degree=3):
    """{"kid"} of the whole sets (subsets = 0), or {"kid", "kid_std", "values"}: mean, population standard deviation and the
    per-subset values of the protocol"""
    if not subsets:
        return {"kid": mmd2_64(x, y, gamma, coef0, degree)}
    ri, fi = draws(x.shape[0], y.shape[0], subsets, subset_size, seed)
    vals = [mmd2_64(x[ri[p]], y[fi[p]], gamma, coef0, degree) for p in range(subsets)]
    mean, std = mean_std(vals)
    return {"kid": mean, "kid_std": std, "values": vals}


# ------------------------------------------------------------------------------------------------------------------ bit-exact
def acc_row(r, half):
    return (r & 3) + 8 * (r >> 2) + 4 * half


def _table():
    """int64 [4, 32]: the tile row that set = wm * 2 + half adds at step = u * 16 + r (csrc/mmd.hip, ORDER OF THE SUMS)"""
    t = torch.empty(4, 32, dtype=torch.int64)
    for wm in range(2):
        for half in range(2):
            for u in range(2):
                for r in range(16):
                    t[wm * 2 + half, u * 16 + r] = wm * 64 + u * 32 + acc_row(r, half)
    return t


TABLE = _table()
NATURAL = torch.arange(TILE).view(4, 32)


def pair_values(S, gamma, coef0, degree):
    """f64, the shape of S: t = S * gamma + coef0 with two roundings, k = t times t a further degree - 1 times, left to right"""
    assert S.dtype == F32 and not S.is_cuda
    t = S.to(F64) * gamma
    t = t + coef0
    k = t
    for _ in range(degree - 1):
        k = k * t
    return k


def oracle_part(S, gamma, coef0=1.0, degree=3, query_base=-1, index_base=0, table=TABLE):
    """S f32 [..., B, N] on the CPU -> part f64 [..., tiles, B]: per tile of 128 columns and per row of S the sum of the pair values,
    the pair with query_base + b == index_base + n left out (query_base >= 0).  Every set starts at +0.0 and adds its rows in step
    order; the sets are added as ((0 + 1) + 2) + 3.  A skipped pair is skipped (torch.where), not added as zero."""
    assert index_base % TILE == 0
    B, N = S.shape[-2:]
    tiles = (N + TILE - 1) // TILE
    k = pair_values(S, gamma, coef0, degree)
    valid = torch.ones(B, N, dtype=torch.bool)
    if query_base >= 0:
        valid &= (torch.arange(B)[:, None] + query_base) != (torch.arange(N)[None, :] + index_base)
    pad = tiles * TILE - N
    k = torch.cat([k, torch.full(k.shape[:-1] + (pad,), float("nan"), dtype=F64)], -1).reshape(k.shape[:-1] + (tiles, TILE))
    valid = torch.cat([valid, torch.zeros(B, pad, dtype=torch.bool)], -1).reshape(B, tiles, TILE)
    acc = torch.zeros(k.shape[:-1] + (4,), dtype=F64)
    for step in range(32):
        rows = table[:, step]
        acc = torch.where(valid[..., rows], acc + k[..., rows], acc)
    part = ((acc[..., 0] + acc[..., 1]) + acc[..., 2]) + acc[..., 3]
    return part.transpose(-1, -2).contiguous()


def oracle_fold(part, rowsum=None):
    """rowsum f64 [..., B] (zeros when None) plus part [..., tiles, B], tile by tile in ascending order"""
    rowsum = torch.zeros(part.shape[:-2] + part.shape[-1:], dtype=F64) if rowsum is None else rowsum.clone()
    for t in range(part.shape[-2]):
        rowsum = rowsum + part[..., t, :]
    return rowsum


def oracle_total(rowsum):
    """[...]: neighbours paired level by level, an odd last element moves up unchanged"""
    v = rowsum
    while v.shape[-1] > 1:
        n = v.shape[-1]
        nxt = v[..., 0:n - (n % 2):2] + v[..., 1::2]
        v = torch.cat([nxt, v[..., n - 1:]], -1) if n % 2 else nxt
    return v[..., 0]


def estimate(sxx, syy, sxy, m, n):
    """the host's finish of vtp_amd.KID from the three totals, python floats"""
    return sxx / (m * (m - 1)) + syy / (n * (n - 1)) - 2.0 * sxy / (m * n)


# ------------------------------------------------------------------------------------------------------------------ the bound
def bound(x, y, gamma=None, coef0=1.0, degree=3):
    """An a-priori bound of |KID - kid_64| for the rows x, y (the full-set estimator; a subset is bounded by its own rows).
    The fp32 chain of a product s = sum_k a_k b_k of D terms: |s^ - s| <= g_D sum_k |a_k b_k|, g_D = D u / (1 - D u), u = 2^-24.
    t = s gamma + coef0 moves by at most delta = gamma g_D sum_k |a_k b_k|, and k = t^degree by at most
    max(|k(t + delta) - k(t)|, |k(t - delta) - k(t)|): t^degree is monotone (odd degree) or convex (even degree), so its largest
    deviation over [t - delta, t + delta] is at an end.  These are summed over the pairs with the estimator's weights.  The fp64
    work -- degree + 1 operations per value, a sum of `pairs` terms in some order, the host's finish -- adds at most
    (pairs + degree + 6) 2^-53 sum |k| per block, weighted the same way."""
    D = x.shape[1]
    gamma = 1.0 / D if gamma is None else gamma
    g_D = D * U32 / (1 - D * U32)
    m, n = x.shape[0], y.shape[0]
    total = 0.0
    for a, b, w, own in ((x, x, 1.0 / (m * (m - 1)), True), (y, y, 1.0 / (n * (n - 1)), True), (x, y, 2.0 / (m * n), False)):
        a, b = a.to(F64), b.to(F64)
        t = (a @ b.T) * gamma + coef0
        delta = gamma * g_D * (a.abs() @ b.abs().T)
        k = t ** degree
        dk = torch.maximum(((t + delta) ** degree - k).abs(), ((t - delta) ** degree - k).abs())
        if own:
            dk.fill_diagonal_(0.0)
            k.fill_diagonal_(0.0)
        pairs = a.shape[0] * (b.shape[0] - (1 if own else 0))
        total += w * (float(dk.sum()) + (pairs + degree + 6) * U64 * float(k.abs().sum()))
    return total


@functools.lru_cache(maxsize=None)
def case_64(i):
    """(kid_64, bound) of the full-set estimator on case i"""
    x, y = case(i)
    return kid_64(x, y)["kid"], bound(x, y)


@functools.lru_cache(maxsize=None)
def subset_case_64(i):
    """kid_64 of the subset protocol of the tests on case i, and the per-subset bounds"""
    x, y = case(i)
    out = kid_64(x, y, SUBSETS, SUBSET_SIZE, seed=i)
    ri, fi = draws(x.shape[0], y.shape[0], SUBSETS, SUBSET_SIZE, i)
    return out, [bound(x[ri[p]], y[fi[p]]) for p in range(SUBSETS)]
