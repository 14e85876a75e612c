#!/usr/bin/env python3
"""Image-text retrieval at the sizes it is run at: vtp_amd.Retrieval.result() for MSCOCO-5k (5 000 images, 25 000 captions) and for
a 100 000 x 500 000 set, at the CLIP width of the model (768), both directions, seeded synthetic unit features (images with few
intrinsic dimensions, a caption is its image's feature plus noise), next to the torch formulation a user runs today, in fp32 on the
same GPU in the same process: per 1 024 queries S = q @ x^T with matmul over gallery chunks into a [1024, gallery] block, the best
ground-truth similarity by a masked max over it, rank = (S > s*) summed.  That side is a rocBLAS GEMM plus several passes over a
block of similarities in memory against one fused pass that never writes it -- a comparison of two ways to get the number, not
kernel against kernel.

    python tools/retrieval_bench.py [--cases 5000x5 100000x5] [--dim 768] [--reps 5] [--out profiles/retrieval.log]

Each case is timed whole: result() (ground-truth lists, both directions, counters, the copy of the ranks to the host) against the
torch side doing the same, a host clock around work that ends in a copy to the host, one warm-up run of each side and `reps`
alternating runs, the median on record.  TFLOP/s counts the similarities alone, 2 D x images x captions x 2 directions.  Also
recorded: how many ranks differ between the two sides (torch's similarities are not the fmaf chain's bits and its count has no tie
rule), that fused runs repeat bit for bit and that other chunk sizes change nothing, and the pieces alone on one pass of 4 096
queries (device events over back-to-back launches)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-rows", type=int, default=1024, help="queries per [queries, gallery] block of the torch side")
    ap.add_argument("--torch-chunk", type=int, default=65536)
    ap.add_argument("--cases", nargs="+", default=["5000x5", "100000x5"], help="images x captions per image")
    ap.add_argument("--latent", type=int, default=6, help="intrinsic dimensions of the synthetic image features")
    ap.add_argument("--noise", type=float, default=1.5, help="norm of the noise a caption adds to its image's unit feature")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retrieval_bench: needs the GPU (no CPU timing)")
    from vtp_amd import ops
    from vtp_amd.retrieval import DIRECTIONS, Retrieval
    dev, D, KS = "cuda", a.dim, (1, 5, 10)
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

    def make(n_img, per, seed):
        """unit image features with `latent` intrinsic dimensions (so that images have near neighbours and recall is not trivial),
        `per` captions per image = the image's feature plus full-width noise, ids and captions shuffled"""
        g = torch.Generator(device=dev).manual_seed(seed)
        P = torch.randn(a.latent, D, device=dev, generator=g)
        img = torch.nn.functional.normalize(torch.randn(n_img, a.latent, device=dev, generator=g) @ P, dim=1)
        img_ids = torch.randperm(n_img, device=dev, generator=g) * 3 + 7
        order = torch.randperm(n_img * per, device=dev, generator=g) // per  # the image of every caption
        noise = a.noise / D ** 0.5 * torch.randn(n_img * per, D, device=dev, generator=g)
        txt = torch.nn.functional.normalize(img[order] + noise, dim=1)
        return {"image": img, "text": txt}, {"image": img_ids, "text": img_ids[order].contiguous()}

    def torch_direction(q, q_ids, x, x_ids):
        """-> (rank int64 [B], counts) the way it is written with torch today"""
        B, N = q.shape[0], x.shape[0]
        rank = torch.empty(B, device=dev, dtype=torch.int64)
        for b0 in range(0, B, a.torch_rows):
            b1 = min(B, b0 + a.torch_rows)
            S = torch.empty(b1 - b0, N, device=dev)
            for n0 in range(0, N, a.torch_chunk):
                n1 = min(N, n0 + a.torch_chunk)
                torch.matmul(q[b0:b1], x[n0:n1].T, out=S[:, n0:n1])
            best = S.masked_fill(q_ids[b0:b1, None] != x_ids[None, :], float("-inf")).max(1).values
            rank[b0:b1] = (S > best[:, None]).sum(1)
        return rank, torch.stack([(rank < k).sum() for k in KS])

    def torch_side(feats, ids):
        out, ranks = {}, {}
        for name, (qs, xs) in DIRECTIONS.items():
            ranks[name], c = torch_direction(feats[qs], ids[qs], feats[xs], ids[xs])
            c, r = c.cpu(), ranks[name].cpu().double() + 1
            out[name] = {f"R@{k}": int(c[m]) / r.shape[0] * 100 for m, k in enumerate(KS)}
            out[name]["median_rank"], out[name]["mean_rank"] = float(r.median()), float(r.mean())
        return out, ranks

    def brief(out):
        return "  ".join(f"{n}: " + " ".join(f"R@{k} {d[f'R@{k}']:.2f}" for k in KS) + f" mean rank {d['mean_rank']:.2f}" for n, d in out.items())

    say(f"# retrieval: D={D} ks={KS} latent={a.latent} noise={a.noise} device={torch.cuda.get_device_name(0)}")
    for seed, case in enumerate(a.cases):
        n_img, per = (int(v) for v in case.split("x"))
        feats, ids = make(n_img, per, seed)
        flop = 2.0 * D * n_img * n_img * per * 2
        r = Retrieval(None, ks=KS, capacity=n_img * per)
        r.add_image_features(feats["image"], ids["image"])
        r.add_text_features(feats["text"], ids["text"])
        first = r.result()
        ranks0 = {n: r.ranks(n).clone() for n in DIRECTIONS}
        tout, tranks = torch_side(feats, ids)
        say(f"## {n_img} images x {n_img * per} captions, both directions ({flop / 1e12:.3f} TFLOP of similarities)")
        say(f"fused {brief(first)}")
        say(f"torch {brief(tout)}")
        say("ranks that differ between the two sides: "
            + ", ".join(f"{int((ranks0[n] != tranks[n]).sum())} of {ranks0[n].shape[0]} ({n})" for n in DIRECTIONS))
        del tranks
        t_f, t_t = [], []
        for i in range(a.reps):
            ms, out = wall(r.result)
            t_f.append(ms)
            same = out == first and all(torch.equal(r.ranks(n), ranks0[n]) for n in DIRECTIONS)
            ms, _ = wall(lambda: torch_side(feats, ids))
            t_t.append(ms)
            say(f"run {i}: fused {t_f[-1]:9.2f} ms   torch {t_t[-1]:9.2f} ms   ranks identical to the first fused run: {same}")
        mf, mt = statistics.median(t_f), statistics.median(t_t)
        say(f"fused  median {mf:9.2f} ms per result()  {flop / mf / 1e9:6.1f} TFLOP/s of the similarities")
        say(f"torch  median {mt:9.2f} ms              {flop / mt / 1e9:6.1f} TFLOP/s")
        say(f"torch / fused = {mt / mf:.2f}" + ("" if mt >= mf else "   ** the torch formulation is FASTER here **"))
        other = Retrieval(None, ks=KS, chunk_rows=7001, query_rows=640)
        other.add_image_features(feats["image"], ids["image"])
        other.add_text_features(feats["text"], ids["text"])
        same = other.result() == first and all(torch.equal(other.ranks(n), ranks0[n]) for n in DIRECTIONS)
        say(f"chunk_rows = 7001, query_rows = 640 give identical ranks: {same}")
        del other
        # the pieces: one pass of 4 096 queries over the whole gallery, device events over back-to-back launches
        for name, (qs, xs) in DIRECTIONS.items():
            q, x = feats[qs], feats[xs]
            B = min(4096, q.shape[0])
            gt_ptr, gt_idx = r.ground_truth(ids[qs], ids[xs])
            bs, bj = torch.empty(q.shape[0], device=dev), torch.empty(q.shape[0], device=dev, dtype=torch.int64)
            beats = torch.zeros(B, device=dev, dtype=torch.int32)
            pieces = ((f"{name}: ground-truth lists, {q.shape[0]} queries, {gt_idx.shape[0]} entries (torch sort + searchsorted, reads nnz)",
                       lambda: r.ground_truth(ids[qs], ids[xs]), 0.0),
                      (f"{name}: vtp_retr_best, {q.shape[0]} queries, {gt_idx.shape[0]} pairs",
                       lambda: ops.retr_best(q, x, gt_ptr, gt_idx, bs, bj), 0.0),
                      (f"{name}: vtp_retr_rank, {B} queries x {x.shape[0]} rows", lambda: ops.retr_rank(q[:B], x, 0, bs[:B], bj[:B], beats),
                       2.0 * B * x.shape[0] * D),
                      (f"{name}: torch matmul alone, {B} x {x.shape[0]} x {D}", lambda: q[:B] @ x.T, 2.0 * B * x.shape[0] * D))
            for what, call, fl in pieces:
                call()
                ms = events(lambda: [call() for _ in range(5)]) / 5
                say(f"  {what:108s} {ms * 1e3:10.1f} us" + (f"  {fl / ms / 1e9:6.1f} TFLOP/s" if fl else ""))
        del r, feats, ids
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
