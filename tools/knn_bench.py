#!/usr/bin/env python3
"""k-NN evaluation at ImageNet size: vtp_amd.Knn.update_features for 5 000 queries in batches of 256 and of 1 024 against banks of
1 281 167 and 100 000 rows (D = 768, K = 200, ks = 10, 20, 100, 200), next to the torch formulation a user runs today, in fp32 on
the same GPU in the same process: matmul over bank chunks of 131 072 rows, topk, merge by cat + topk, softmax, one_hot weighted
prefix sums per k, topk(5).  That side is rocBLAS + topk in several passes over a [B, chunk] matrix in memory against one fused
pass -- a comparison of two ways to get the number, not kernel against kernel.

    python tools/knn_bench.py [--queries 5000] [--banks 1281167 100000] [--batches 256 1024] [--reps 3] [--out profiles/knn.log]

Device events around whole passes over the queries, one warm-up pass, `reps` timed passes per side, alternating; the figure of record
is the median.  Also recorded: that two fused runs give identical counters, that splits = 0 and a forced split count give
identical neighbour lists, the vote kernel alone, and vtp_knn_topk at the heuristic's largest split count on a chunk of one row
(list initialisation and the merge kernels: what a call costs beyond its tiles) and of 128 rows (one tile of which every row
survives: four buffer merges on top of that)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=5000)
    ap.add_argument("--banks", type=int, nargs="+", default=[1281167, 100000])
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=131072)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_bench: needs the GPU (no CPU timing)")
    from vtp_amd import ops
    from vtp_amd.knn import Knn
    dev = "cuda"
    D, C, Q = a.dim, a.classes, a.queries
    ks, T = (10, 20, 100, 200), 0.07
    K = ks[-1]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)  # ms

    say(f"# k-NN evaluation: queries={Q} D={D} classes={C} ks={ks} T={T} device={torch.cuda.get_device_name(0)}")
    g = torch.Generator(device=dev).manual_seed(0)
    centres = torch.randn(C, D, device=dev, generator=g)
    y = torch.randint(0, C, (Q,), device=dev, generator=g)
    q = F.normalize(centres[y] + 4.0 * torch.randn(Q, D, device=dev, generator=g), dim=1)
    for N in a.banks:
        labels = torch.randint(0, C, (N,), device=dev, generator=g)
        knn = Knn(None, num_classes=C, ks=ks, temperature=T, capacity=N)
        for n0 in range(0, N, 1 << 17):  # clustered rows, made and added piece by piece
            lab = labels[n0:n0 + (1 << 17)]
            knn.add_bank_features(centres[lab] + 4.0 * torch.randn(lab.shape[0], D, device=dev, generator=g), lab)
        bank, lab64 = knn.bank, labels.to(torch.int64)
        say(f"## bank N={N} ({N * D * 4 / 1e9:.2f} GB)")
        for B in a.batches:
            tcounts = torch.zeros(len(ks), 3, device=dev, dtype=torch.int64)

            def fused_pass():
                for b0 in range(0, Q, B):
                    knn.update_features(q[b0:b0 + B], y[b0:b0 + B])

            def torch_pass():
                for b0 in range(0, Q, B):
                    qb, yb = q[b0:b0 + B], y[b0:b0 + B]
                    best_s = best_i = None
                    for n0 in range(0, N, a.torch_chunk):
                        s = qb @ bank[n0:n0 + a.torch_chunk].T
                        cs, ci = s.topk(min(K, s.shape[1]), dim=1)
                        ci = ci + n0
                        if best_s is None:
                            best_s, best_i = cs, ci
                        else:
                            ms, mi = torch.cat([best_s, cs], 1), torch.cat([best_i, ci], 1)
                            best_s, o = ms.topk(K, dim=1)
                            best_i = mi.gather(1, o)
                    w = torch.softmax(best_s / T, dim=1)
                    votes = F.one_hot(lab64[best_i], C).to(torch.float32) * w[:, :, None]
                    for m, k in enumerate(ks):
                        top5 = votes[:, :k].sum(1).topk(5, dim=1).indices
                        hit = top5 == yb[:, None]
                        tcounts[m, 0] += hit[:, 0].sum()
                        tcounts[m, 1] += hit.any(1).sum()
                        tcounts[m, 2] += qb.shape[0]

            knn.reset()
            fused_pass()
            first = knn.counts()
            tcounts.zero_()
            torch_pass()
            tc = tcounts.cpu()
            t_f, t_t = [], []
            for r in range(a.reps):
                knn.reset()
                t_f.append(timed(fused_pass))
                again = knn.counts()
                t_t.append(timed(torch_pass))
                say(f"N={N} B={B} pass {r}: fused {t_f[-1]:9.1f} ms   torch {t_t[-1]:9.1f} ms   counters identical to the first fused run: {again == first}")
            mf, mt = statistics.median(t_f), statistics.median(t_t)
            flop = 2.0 * Q * N * D
            say(f"N={N} B={B} fused  median {mf:9.1f} ms  {Q / mf * 1e3:9.0f} queries/s  {flop / mf / 1e9:6.1f} TFLOP/s of the similarity product over the "
                f"whole pass (fid.hip reaches 62.1 on the same instruction)")
            say(f"N={N} B={B} torch  median {mt:9.1f} ms  {Q / mt * 1e3:9.0f} queries/s")
            say(f"N={N} B={B} torch / fused = {mt / mf:.2f}" + ("" if mt >= mf else "   ** the torch formulation is FASTER here **"))
            say(f"N={N} B={B} accuracy fused {({k: tuple(round(v, 2) for v in p) for k, p in knn.accuracy().items()})}  torch counts "
                f"{({k: tuple(int(v) for v in tc[m]) for m, k in enumerate(ks)})} fused counts {first}")

            # the pieces, device events over back-to-back launches
            qb = q[:B].contiguous()
            yb = y[:B].contiguous()
            sims = torch.full((B, K), -float("inf"), device=dev)
            idx = torch.full((B, K), -1, device=dev, dtype=torch.int64)
            ws = torch.empty(ops.knn_workspace_bytes(B, K, 0), device=dev, dtype=torch.uint8)
            chunk = bank[:min(N, knn.chunk_rows)]
            most = ws.numel() // (B * K * 12)  # the largest split count the heuristic takes at this B
            counts = torch.zeros(len(ks), 3, device=dev, dtype=torch.int64)
            pieces = (("vtp_knn_topk, one call on %d rows" % chunk.shape[0], lambda: ops.knn_topk(qb, chunk, 0, K, sims, idx, ws), 3),
                      ("vtp_knn_topk, 128-row chunk (every row survives)", lambda: ops.knn_topk(qb, bank[:128], 0, K, sims, idx, ws, most), 10),
                      ("vtp_knn_topk, 1-row chunk (list init + merge)", lambda: ops.knn_topk(qb, bank[:1], 0, K, sims, idx, ws, most), 10),
                      ("vtp_knn_vote", lambda: ops.knn_vote(sims, idx, knn.bank_labels, yb, ks, 1.0 / T, C, counts), 10))
            for name, call, reps in pieces:
                call()
                ms = timed(lambda: [call() for _ in range(reps)]) / reps
                extra = f"  {2.0 * B * chunk.shape[0] * D / ms / 1e9:6.1f} TFLOP/s" if name.startswith("vtp_knn_topk, one call") else ""
                say(f"  B={B}: {name:48s} {ms * 1e3:10.1f} us{extra}")
        if N == min(a.banks):
            # splits = 0 against a forced split count: identical lists
            B = a.batches[0]
            outs = []
            for splits in (0, 7):
                so, io = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev, dtype=torch.int64)
                knn.update_features(q[:B], y[:B], sims_out=so, idx_out=io, splits=splits)
                outs.append((so, io))
            same = torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1])
            say(f"N={N} B={B}: splits = 0 and splits = 7 give identical lists: {same}")
        del knn, bank
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
