"""Image-text retrieval of vtp_amd.Retrieval (csrc/retrieval.hip) restated on the CPU.  Not a test module; imported by
tests/test_retrieval_host.py and tests/test_retrieval_gpu.py.

For a query i, a gallery of N rows and similarities S[i, j] (compared exactly, whatever the float type):
    G(i)       = the gallery rows that share the query's image id.
    order      = gallery rows by (similarity descending, gallery index ascending), a total order.
    (s*, j*)   = the first element of G(i) under that order.
    rank[i]    = the number of gallery rows strictly before (s*, j*); N for an empty G(i).
    R@K        = #{rank < K} / rows.
The rank is stated twice, independently: rank_by_count is the counting formula #{s > s*} + #{j < j* : s == s*} around best_of;
rank_by_sort is a stable sort by -s and the position of the first ground-truth row in it.  A NaN is never chosen as s* and never
counted (inputs are finite by contract; rank_by_sort does not take NaNs)."""
import torch

F64, I32, I64 = torch.float64, torch.int32, torch.int64
NEG = float("-inf")


def sims_64(q, x):
    return q.to(F64) @ x.to(F64).T


def gt_lists(query_ids, gallery_ids):
    """per query the gallery rows with its id, ascending"""
    where = {}
    for j, g in enumerate(gallery_ids.tolist()):
        where.setdefault(g, []).append(j)
    return [where.get(i, []) for i in query_ids.tolist()]


def csr(lists):
    """lists of gallery rows -> (gt_ptr int32 [B + 1], gt_idx int64 [nnz])"""
    ptr = [0]
    for l in lists:
        ptr.append(ptr[-1] + len(l))
    return torch.tensor(ptr, dtype=I32), torch.tensor([j for l in lists for j in l], dtype=I64)


def best_of(S, lists, index_base=0):
    """S [B, N]: the gallery rows index_base .. index_base + N - 1; lists hold GLOBAL rows, those outside the chunk are ignored.
    -> (best_s of S's dtype [B], best_j int64 [B], global): the first list entry under (s descending, row ascending); (-inf, -1)
    for none"""
    B, N = S.shape
    rows = S.tolist()  # python floats hold every f32 / f64 exactly
    bs, bj = [NEG] * B, [-1] * B
    for b, l in enumerate(lists):
        for j in l:
            c = j - index_base
            if not 0 <= c < N:
                continue
            s = rows[b][c]
            if s > bs[b] or (s == bs[b] and j < bj[b]):
                bs[b], bj[b] = s, j
    return torch.tensor(bs, dtype=S.dtype), torch.tensor(bj, dtype=I64)


def rank_by_count(S, best_s, best_j, index_base=0):
    """the counting formula on the chunk S [B, N] whose row 0 is the global row index_base: int32 [B].  best_j == -1: every row"""
    B, N = S.shape
    j = torch.arange(N, dtype=I64)[None, :] + index_base
    s = best_s.to(S.dtype)[:, None]
    before = (S > s) | ((S == s) & (j < best_j[:, None]))
    before |= (best_j < 0)[:, None]
    return before.sum(1).to(I32)


def rank_by_sort(S, lists):
    """stable sort by -s and the position of the first ground-truth row: int32 [B]; N for an empty list"""
    B, N = S.shape
    order = torch.sort(-S, dim=1, stable=True).indices
    out = torch.full((B,), N, dtype=I32)
    for b, l in enumerate(lists):
        members = set(j for j in l if 0 <= j < N)
        if not members:
            continue
        for pos, j in enumerate(order[b].tolist()):
            if j in members:
                out[b] = pos
                break
    return out


def counts_of(rank, ks):
    """rank [B] -> int64 [nk + 1]: #{rank < k} per k, and the rows"""
    return torch.tensor([int((rank < k).sum()) for k in ks] + [rank.shape[0]], dtype=I64)


def summary(rank, ks):
    """what Retrieval.result() reports for one direction, from the ranks"""
    r = rank.to(F64) + 1
    n = rank.shape[0]
    out = {f"R@{k}": int((rank < k).sum()) / n * 100 for k in ks}
    out["counts"] = {k: int((rank < k).sum()) for k in ks}
    out["rows"] = n
    out["median_rank"] = float(r.median()) if n % 2 else float(r.sort().values[n // 2 - 1:n // 2 + 1].mean())
    out["mean_rank"] = float(r.mean())
    return out


def evaluate(img, img_ids, txt, txt_ids, ks):
    """both directions on f32 / f64 features: {"image_to_text": summary, "text_to_image": summary} and the ranks"""
    out, ranks = {}, {}
    for name, (q, qi, x, xi) in {"image_to_text": (img, img_ids, txt, txt_ids), "text_to_image": (txt, txt_ids, img, img_ids)}.items():
        S = sims_64(q, x)
        lists = gt_lists(qi, xi)
        ranks[name] = rank_by_sort(S, lists)
        out[name] = summary(ranks[name], ks)
    return out, ranks


def dyadic(shape, gen, step=16):
    """f32 entries m * step / 64 with m * step in [-64, 64]: multiples of 2^-6 in [-1, 1] (of step * 2^-6: a coarse step makes equal
    similarities frequent).  Every product is a multiple of 2^-12 of magnitude <= 1, so a chain of up to 2^11 terms is exact in fp32
    whatever the order."""
    lim = 64 // step
    return torch.randint(-lim, lim + 1, shape, generator=gen).to(torch.float32) * (step / 64)
