#!/usr/bin/env python3
"""Kernel Inception Distance at the sizes it is reported at: vtp_amd.KID.result() for 10 000 real and 50 000 generated rows (D = 2048,
seeded synthetic features with few intrinsic dimensions) -- the standard protocol (100 subsets of 1 000 rows) and the full-set
estimator -- next to the torch formulation a user runs today, in fp32 on the same GPU in the same process: per subset (or per chunk
of 1 024 queries over bank chunks) a matmul, (s * gamma + coef0).pow(3) and a sum with the diagonal masked, the sums kept in fp64.
That side is a rocBLAS GEMM plus several passes over a [1024, chunk] matrix in memory against one fused pass whose pair values are
formed in fp64 -- a comparison of two ways to get the number, not kernel against kernel.

    python tools/kid_bench.py [--real 10000] [--fake 50000] [--dim 2048] [--reps 5] [--out profiles/kid.log]

One warm-up run of each side, then `reps` timed runs per side, alternating, a host clock around a synchronise (result() ends in a
copy to the host); the figure of record is the best, the median beside it.  The subset draws on the host are outside the windows on
both sides -- KID keeps its tables for the next result() on the same row counts, the torch side is handed them -- and are timed on
their own: a first result() pays them once.  TFLOP/s counts the products alone.  Also recorded: how many leading digits of the two
sides' KID agree, that repeated fused runs and a run with other chunk sizes give identical bits, and the tile kernel alone (device
events over back-to-back launches)."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def digits(a, b):
    """leading decimal digits on which a and b agree"""
    if a == b:
        return 17
    return max(0, int(math.floor(-math.log10(abs(a - b) / max(abs(a), abs(b))))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--real", type=int, default=10000)
    ap.add_argument("--fake", type=int, default=50000)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--latent", type=int, default=16)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--query-rows", type=int, default=1024)
    ap.add_argument("--torch-chunk", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kid_bench: needs the GPU (no CPU timing)")
    from vtp_amd import ops
    from vtp_amd.kid import KID, subset_tables
    dev = "cuda"
    Nr, Ng, D, L, P, m = a.real, a.fake, a.dim, a.latent, a.subsets, a.subset_size
    gamma, F64 = 1.0 / D, torch.float64
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

    say(f"# KID: real={Nr} fake={Ng} D={D} latent={L} subsets={P} x {m} device={torch.cuda.get_device_name(0)}")
    g = torch.Generator(device=dev).manual_seed(0)
    proj = torch.randn(L, D, device=dev, generator=g) / L ** 0.5
    real = torch.randn(Nr, L, device=dev, generator=g) @ proj + 0.02 * torch.randn(Nr, D, device=dev, generator=g)
    fake = (0.9 * torch.randn(Ng, L, device=dev, generator=g) + 0.2) @ proj + 0.02 * torch.randn(Ng, D, device=dev, generator=g)

    def make(**kw):
        kid = KID(capacity=max(Nr, Ng), **kw)
        kid.add_real_features(real)
        kid.add_fake_features(fake)
        return kid

    def torch_block(q, x, own):
        """the fp64 sum of the kernel values of q against x (the diagonal masked when own) from fp32 matmul and pow"""
        k = (q @ x.T * gamma + 1.0).pow(3)
        if own:
            k.fill_diagonal_(0.0)
        return k.sum(dtype=F64)

    torch.randperm(8)  # the first call's set-up is not the draws
    t0 = time.perf_counter()
    tab = subset_tables(Nr, Ng, P, m, 0)
    say(f"the subset draws on the host ({P} x 2 randperm; both sides keep their tables, so the timed runs below do not hold them): "
        f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
    ri, fi = tab["real"].to(dev).long(), tab["fake"].to(dev).long()

    def torch_subsets():
        vals = []
        for p in range(P):
            x, y = real[ri[p]], fake[fi[p]]
            vals.append(torch_block(x, x, True) / (m * (m - 1)) + torch_block(y, y, True) / (m * (m - 1)) - 2.0 * torch_block(x, y, False) / (m * m))
        v = torch.stack(vals).cpu()
        return {"kid": float(v.mean()), "kid_std": float(v.std(unbiased=False))}

    def torch_sum(q, x, own):
        total = torch.zeros((), device=dev, dtype=F64)
        for b0 in range(0, q.shape[0], a.query_rows):
            b1 = min(q.shape[0], b0 + a.query_rows)
            for n0 in range(0, x.shape[0], a.torch_chunk):
                n1 = min(x.shape[0], n0 + a.torch_chunk)
                k = (q[b0:b1] @ x[n0:n1].T * gamma + 1.0).pow(3)
                if own:
                    lo, hi = max(b0, n0), min(b1, n1)
                    if lo < hi:
                        k[lo - b0:hi - b0, lo - n0:hi - n0].fill_diagonal_(0.0)
                total += k.sum(dtype=F64)
        return total

    def torch_full():
        t = torch.stack([torch_sum(real, real, True), torch_sum(fake, fake, True), torch_sum(real, fake, False)]).cpu().tolist()
        return {"kid": t[0] / (Nr * (Nr - 1)) + t[1] / (Ng * (Ng - 1)) - 2.0 * t[2] / (Nr * Ng)}

    sides = (("standard protocol", make(subsets=P, subset_size=m, query_rows=a.query_rows), torch_subsets, 2.0 * D * 3 * P * float(m) ** 2),
             ("full-set estimator", make(subsets=0, query_rows=a.query_rows), torch_full,
              2.0 * D * (float(Nr) ** 2 + float(Ng) ** 2 + float(Nr) * Ng)))
    for name, kid, torch_side, flop in sides:
        say(f"## {name}")
        first, tout = kid.result(), torch_side()  # warm every shape of both sides
        say(f"fused {first}")
        say(f"torch {tout}")
        say(f"leading digits of kid on which the two sides agree: {digits(first['kid'], tout['kid'])}"
            + (f"; of kid_std: {digits(first['kid_std'], tout['kid_std'])}" if "kid_std" in first else ""))
        t_f, t_t, same = [], [], True
        for r in range(a.reps):
            ms, out = wall(kid.result)
            t_f.append(ms)
            same = same and out == first
            ms, _ = wall(torch_side)
            t_t.append(ms)
            say(f"run {r}: fused {t_f[-1]:9.1f} ms   torch {t_t[-1]:9.1f} ms")
        say(f"every fused run returned the bits of the first: {same}")
        bf, bt = min(t_f), min(t_t)
        say(f"fused  best {bf / 1e3:8.4f} s (median {statistics.median(t_f) / 1e3:8.4f} s) per result()  {flop / bf / 1e9:6.1f} TFLOP/s of the products "
            f"({flop / 1e12:.2f} TFLOP)")
        say(f"torch  best {bt / 1e3:8.4f} s (median {statistics.median(t_t) / 1e3:8.4f} s) per result()  {flop / bt / 1e9:6.1f} TFLOP/s")
        say(f"torch / fused = {bt / bf:.2f}" + ("" if bt >= bf else "   ** the torch formulation is FASTER here **"))
    other = make(subsets=0, chunk_rows=7001, query_rows=640)
    say(f"chunk_rows = 7001 (-> {other.chunk_rows}), query_rows = 640 give the identical full-set result: {other.result() == sides[1][1].result()}")
    del other

    # the piece: one pass of query_rows queries over a whole bank, device events over back-to-back launches
    B = min(a.query_rows, Ng, Nr)
    part = torch.empty(ops.mmd_workspace_bytes(B, Ng) // 8, device=dev, dtype=F64).view(1, -1, B)
    rowsum = torch.zeros(1, B, device=dev, dtype=F64)
    pieces = ((f"vtp_mmd_poly_part, {B} queries x {Ng} rows (diagonal excluded)", lambda: ops.mmd_poly_part(fake[:B], fake, part, gamma, query_base=0),
               2.0 * B * Ng * D),
              (f"vtp_mmd_fold, {part.shape[1]} tiles x {B} queries", lambda: ops.mmd_fold(part, rowsum), 0.0),
              (f"torch matmul alone, {B} x {Ng} x {D}", lambda: fake[:B] @ fake.T, 2.0 * B * Ng * D))
    for name, call, fl in pieces:
        call()
        ms = events(lambda: [call() for _ in range(5)]) / 5
        say(f"  {name:64s} {ms * 1e3:10.1f} us" + (f"  {fl / ms / 1e9:6.1f} TFLOP/s" if fl else ""))
    say("# caveats: synthetic features; the torch side is a rocBLAS GEMM plus passes over a block of products (pair values in fp32), the")
    say("# fused side one pass with pair values in fp64 -- two ways to get the number, not kernel against kernel; the subset draws on the")
    say("# host are outside both sides' windows and timed on their own (a first result() pays them); parity with other KID programs is unpinned (their subset draws differ); no counters, no trace")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
