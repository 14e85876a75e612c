"""The weighted k-NN classifier of vtp_amd.Knn (csrc/knn.hip) restated in fp64 on the CPU: the DINO / DINOv2 protocol as the papers
describe it.  Not a test module; imported by tests/test_knn_host.py and tests/test_knn_gpu.py.

    neighbours : the first K bank rows under (similarity descending, bank index ascending) -- a stable sort by -s.
    vote       : w_j = exp((s_j - s_0) / T); the score of class c at k is the sum of w_j over the first k neighbours with label c,
                 added in neighbour order; classes are ranked by (score descending, class index ascending) and a class without a
                 neighbour has score 0.  Only the classes that occur are held: a target with score 0 is ranked behind every class
                 that is before it among those that occur, and behind every class of lower index that does not occur --
                 rank = #{occurring classes before the target} + target - #{occurring classes with a lower index}.
"""
import math

import torch


def neighbours(S: torch.Tensor, K: int, index_base: int = 0):
    """S [B, N] (any float type, compared exactly) -> (sims [B, K], idx int64 [B, K])"""
    order = torch.sort(-S, dim=1, stable=True).indices[:, :K]
    return torch.gather(S, 1, order), order + index_base


def _before(a, b):
    """(score, class) a strictly before b"""
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


def vote_row(sims, labels, target, ks, T, C):
    """one query: sims (K floats, the list order) and labels (K ints) of its neighbours.  Per k of ks: dict(rank, pred, gap1, gap5) --
    rank = the number of classes ranked before the target (C for a target outside [0, C)), pred = the five best classes, gap1 /
    gap5 = (first, second) and (fifth, sixth) score of the ranking, the pairs whose order decides top-1 and top-5."""
    s = [float(x) for x in sims]
    w = [math.exp((x - s[0]) / T) for x in s]
    out, scores, done = [], {}, 0
    for k in ks:
        for j in range(done, k):  # neighbour order: the scores at k are prefixes of one sum per class
            c = int(labels[j])
            if 0 <= c < C:
                scores[c] = scores.get(c, 0.0) + w[j]
        done = k
        t = int(target)
        if 0 <= t < C:
            me = (scores.get(t, 0.0), t)
            rank = sum(1 for c, v in scores.items() if _before((v, c), me))
            if me[0] == 0.0:
                rank += t - sum(1 for c in scores if c < t)
        else:
            rank = C
        unseen = [c for c in range(min(C, len(scores) + 6)) if c not in scores][:6]
        order = sorted([(v, c) for c, v in scores.items()] + [(0.0, c) for c in unseen], key=lambda e: (-e[0], e[1]))
        top = [e[0] for e in order[:6]] + [0.0] * 6
        out.append(dict(rank=rank, pred=[e[1] for e in order[:5]], gap1=(top[0], top[1]), gap5=(top[4], top[5])))
    return out


def vote(sims, labels, targets, ks, T, C):
    """sims [B, K], labels [B, K] (the labels of the neighbours), targets [B] -> rank int32 [B, nk], pred int32 [B, nk, 5],
    gap1 / gap5 f64 [B, nk, 2]"""
    B, nk = sims.shape[0], len(ks)
    rank = torch.zeros(B, nk, dtype=torch.int32)
    pred = torch.zeros(B, nk, 5, dtype=torch.int32)
    gap1 = torch.zeros(B, nk, 2, dtype=torch.float64)
    gap5 = torch.zeros(B, nk, 2, dtype=torch.float64)
    sl, ll, tl = sims.tolist(), labels.tolist(), targets.tolist()
    for b in range(B):
        for m, r in enumerate(vote_row(sl[b], ll[b], tl[b], ks, T, C)):
            rank[b, m] = r["rank"]
            pred[b, m] = torch.tensor(r["pred"], dtype=torch.int32)
            gap1[b, m] = torch.tensor(r["gap1"], dtype=torch.float64)
            gap5[b, m] = torch.tensor(r["gap5"], dtype=torch.float64)
    return rank, pred, gap1, gap5


def close(gap, rel=1e-4):
    """gap [..., 2] = (larger, smaller): the pair is closer than rel relative to the larger score (two zeros are not close: their
    order is decided by the class index, exactly)"""
    return (gap[..., 0] - gap[..., 1]) < rel * gap[..., 0]


def counts_of(rank):
    """rank [B, nk] -> int64 [nk, 3]: top-1 hits, top-5 hits, rows"""
    return torch.stack([(rank < 1).sum(0), (rank < 5).sum(0), torch.full((rank.shape[1],), rank.shape[0])], 1).to(torch.int64)
