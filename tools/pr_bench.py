#!/usr/bin/env python3
"""k-NN manifold precision / recall at the ADM protocol sizes: vtp_amd.PrecisionRecall.result() for 10 000 real and 50 000 generated
rows (D = 2048, k = 3, seeded synthetic features with few intrinsic dimensions), next to the torch formulation a user runs today, in
fp32 on the same GPU in the same process: per chunk of 1 024 queries |a|^2 + |b|^2 - 2 a @ b^T with matmul over bank chunks,
topk(k + 1, largest=False) for the radii (the row itself included, as ADM), compare + any for the cover.  That side is a rocBLAS
GEMM plus several passes over a [1024, chunk] matrix in memory against one fused pass -- a comparison of two ways to get the
number, not kernel against kernel.

    python tools/pr_bench.py [--real 10000] [--fake 50000] [--dim 2048] [--k 3] [--reps 3] [--out profiles/precision_recall.log]

One warm-up run of each side, then `reps` timed runs per side, alternating, a host clock around a synchronise (result() ends in a
copy to the host); the figure of record is the median.  TFLOP/s counts the distance products alone, 2 D (Nr^2 + Ng^2 + 2 Nr Ng).
Also recorded: the number of rows whose covered / not covered decision differs between the two sides (torch's distances are not
the fmaf chain's bits, so near-ties may flip), that two fused runs and a run with other chunk sizes give identical radii and hits,
and the two tile kernels alone on one pass of 1 024 queries (device events over back-to-back launches)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--real", type=int, default=10000)
    ap.add_argument("--fake", type=int, default=50000)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--latent", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--query-rows", type=int, default=1024)
    ap.add_argument("--torch-chunk", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pr_bench: needs the GPU (no CPU timing)")
    from vtp_amd import ops
    from vtp_amd.precision_recall import PrecisionRecall
    dev = "cuda"
    Nr, Ng, D, k, L = a.real, a.fake, a.dim, a.k, a.latent
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out  # ms

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)  # ms

    say(f"# precision / recall: real={Nr} fake={Ng} D={D} k={k} latent={L} device={torch.cuda.get_device_name(0)}")
    g = torch.Generator(device=dev).manual_seed(0)
    P = torch.randn(L, D, device=dev, generator=g) / L ** 0.5
    real = torch.randn(Nr, L, device=dev, generator=g) @ P + 0.02 * torch.randn(Nr, D, device=dev, generator=g)
    fake = (0.9 * torch.randn(Ng, L, device=dev, generator=g) + 0.2) @ P + 0.02 * torch.randn(Ng, D, device=dev, generator=g)
    flop = 2.0 * D * (float(Nr) ** 2 + float(Ng) ** 2 + 2.0 * Nr * Ng)

    pr = PrecisionRecall(k=k, capacity=max(Nr, Ng), query_rows=a.query_rows)
    pr.add_real_features(real)
    pr.add_fake_features(fake)

    def fused():
        out = pr.result()
        return out, pr.hits("fake") > 0, pr.hits("real") > 0

    def torch_dist(q, nq, x, nx, b0, b1, n0, n1):
        return nq[b0:b1, None] + nx[None, n0:n1] - 2.0 * (q[b0:b1] @ x[n0:n1].T)

    def torch_radii(x, nx):
        N = x.shape[0]
        out = torch.empty(N, device=dev)
        for b0 in range(0, N, a.query_rows):
            b1 = min(N, b0 + a.query_rows)
            best = None
            for n0 in range(0, N, a.torch_chunk):
                n1 = min(N, n0 + a.torch_chunk)
                d = torch_dist(x, nx, x, nx, b0, b1, n0, n1)
                c = d.topk(min(k + 1, n1 - n0), dim=1, largest=False).values
                best = c if best is None else torch.cat([best, c], 1).topk(k + 1, dim=1, largest=False).values
            out[b0:b1] = best[:, k]  # the (k + 1)-th smallest, the row itself included
        return out

    def torch_cover(q, nq, x, nx, r2):
        B, N = q.shape[0], x.shape[0]
        out = torch.zeros(B, device=dev, dtype=torch.bool)
        for b0 in range(0, B, a.query_rows):
            b1 = min(B, b0 + a.query_rows)
            for n0 in range(0, N, a.torch_chunk):
                n1 = min(N, n0 + a.torch_chunk)
                out[b0:b1] |= (torch_dist(q, nq, x, nx, b0, b1, n0, n1) <= r2[None, n0:n1]).any(1)
        return out

    def torch_side():
        nr, ng = (real * real).sum(1), (fake * fake).sum(1)
        rr, rg = torch_radii(real, nr), torch_radii(fake, ng)
        cf, cr = torch_cover(fake, ng, real, nr, rr), torch_cover(real, nr, fake, ng, rg)
        return {"precision": int(cf.sum()) / Ng, "recall": int(cr.sum()) / Nr}, cf, cr

    # warm every shape of both sides
    first, ff, fr = fused()
    radii0 = {s: pr.radii(s).clone() for s in ("real", "fake")}
    hits0 = {s: pr.hits(s).clone() for s in ("real", "fake")}
    tout, tf, tr = torch_side()
    say(f"fused {first}   torch {tout}")
    say(f"decisions that differ between the two sides: {int((ff != tf).sum())} of {Ng} generated rows, {int((fr != tr).sum())} of {Nr} real rows")
    t_f, t_t = [], []
    for r in range(a.reps):
        ms, (out, _, _) = wall(fused)
        t_f.append(ms)
        same = out == first and all(torch.equal(pr.radii(s).view(torch.int32), radii0[s].view(torch.int32)) and torch.equal(pr.hits(s), hits0[s])
                                    for s in ("real", "fake"))
        ms, _ = wall(torch_side)
        t_t.append(ms)
        say(f"run {r}: fused {t_f[-1]:9.1f} ms   torch {t_t[-1]:9.1f} ms   radii and hits identical to the first fused run: {same}")
    mf, mt = statistics.median(t_f), statistics.median(t_t)
    say(f"fused  median {mf / 1e3:8.4f} s per result()  {flop / mf / 1e9:6.1f} TFLOP/s of the distance products ({flop / 1e12:.2f} TFLOP)")
    say(f"torch  median {mt / 1e3:8.4f} s per result()  {flop / mt / 1e9:6.1f} TFLOP/s")
    say(f"torch / fused = {mt / mf:.2f}" + ("" if mt >= mf else "   ** the torch formulation is FASTER here **"))

    # other chunk sizes: the same bits
    other = PrecisionRecall(k=k, capacity=max(Nr, Ng), chunk_rows=7001, query_rows=640)
    other.add_real_features(real)
    other.add_fake_features(fake)
    o = other.result()
    same = o == first and all(torch.equal(other.radii(s).view(torch.int32), radii0[s].view(torch.int32)) and torch.equal(other.hits(s), hits0[s])
                              for s in ("real", "fake"))
    say(f"chunk_rows = 7001, query_rows = 640 give identical radii and hits: {same}")
    del other

    # the pieces: one pass of query_rows queries over a whole bank, device events over back-to-back launches
    B = min(a.query_rows, Ng, Nr)
    nr, ng = torch.empty(Nr, device=dev), torch.empty(Ng, device=dev)
    ops.pr_sqnorm(real, nr)
    ops.pr_sqnorm(fake, ng)
    dist = torch.full((B, ops.PR_MAX_K), float("inf"), device=dev)
    ws = torch.empty(ops.pr_workspace_bytes(B), device=dev, dtype=torch.uint8)
    hits = torch.zeros(B, device=dev, dtype=torch.int32)
    pieces = ((f"vtp_pr_sqnorm, {Ng} rows", lambda: ops.pr_sqnorm(fake, ng), 0.0),
              (f"vtp_pr_knn_dist, {B} queries x {Ng} rows (self-exclusion on)", lambda: ops.pr_knn_dist(fake[:B], ng[:B], fake, ng, dist, ws, 0, 0),
               2.0 * B * Ng * D),
              (f"vtp_pr_knn_dist, {B} queries x {Nr} rows", lambda: ops.pr_knn_dist(real[:B], nr[:B], real, nr, dist, ws, 0, 0), 2.0 * B * Nr * D),
              (f"vtp_pr_cover, {B} queries x {Nr} rows", lambda: ops.pr_cover(fake[:B], ng[:B], real, nr, radii0["real"], hits), 2.0 * B * Nr * D),
              (f"vtp_pr_cover, {B} queries x {Ng} rows", lambda: ops.pr_cover(real[:B], nr[:B], fake, ng, radii0["fake"], hits), 2.0 * B * Ng * D),
              (f"torch matmul alone, {B} x {Ng} x {D}", lambda: fake[:B] @ fake.T, 2.0 * B * Ng * D))
    for name, call, fl in pieces:
        call()
        ms = events(lambda: [call() for _ in range(5)]) / 5
        say(f"  {name:64s} {ms * 1e3:10.1f} us" + (f"  {fl / ms / 1e9:6.1f} TFLOP/s" if fl else ""))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
