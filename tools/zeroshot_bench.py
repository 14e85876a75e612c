#!/usr/bin/env python3
"""Zero-shot evaluation step at the reference tool's shape (B = 128 and 256 images, D = 768, 1000 classes), features and classifier
given: vtp_amd.ZeroShot.update_features against the torch formulation a user of the tool runs today (logits = 100.0 * f @ W,
accuracy(logits, targets, (1, 5)) with its two host copies per batch -- oracle/tools_oracle.py:62-66, :96-99), plus the two kernels
alone.

    python tools/zeroshot_bench.py [--steps 20] [--rounds 5] [--out profiles/zeroshot_step.log]

Both loops get their inputs ready-made and are timed in alternating windows of `steps` batches, each closed by reading the
accumulated accuracy on the host (which is when the fused path synchronises at all); the figure of record is the median window."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--templates", type=int, default=80)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("zeroshot_bench: needs the GPU (no CPU timing)")
    from oracle.tools_oracle import accuracy  # the tool's accuracy() as the oracle restates it
    from vtp_amd import ops
    from vtp_amd.zeroshot import ZeroShot
    dev = "cuda"
    D, C = a.dim, a.classes
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# zero-shot step: D={D} classes={C} device={torch.cuda.get_device_name(0)}")
    torch.manual_seed(0)
    W = torch.nn.functional.normalize(torch.randn(C, D, device=dev), dim=1).T  # [D, C] as the tool builds it (a transposed view)
    zs = ZeroShot(None)
    zs.set_classifier(W)
    for B in a.batches:
        f = torch.nn.functional.normalize(torch.randn(B, D, device=dev), dim=1)
        y = torch.randint(0, C, (B,), device=dev)

        def torch_window():
            top1 = top5 = n = 0.0
            for _ in range(a.steps):
                logits = 100.0 * f @ W
                a1, a5 = accuracy(logits, y, topk=(1, 5))
                top1, top5, n = top1 + a1, top5 + a5, n + B
            return top1 / n * 100, top5 / n * 100

        def ours_window():
            zs.reset()
            for _ in range(a.steps):
                zs.update_features(f, y)
            return zs.accuracy()

        def window(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps * 1e6, acc

        for fn in (ours_window, torch_window):  # warm-up: code objects, library algorithm choice
            fn()
        t_ours, t_torch = [], []
        for r in range(a.rounds):
            to, ao = window(ours_window)
            tt, at = window(torch_window)
            t_ours.append(to)
            t_torch.append(tt)
            say(f"B={B} round {r}: fused {to:8.1f} us/batch (top-1 {ao[0]:.3f} top-5 {ao[1]:.3f})   torch {tt:8.1f} us/batch (top-1 {at[0]:.3f} top-5 {at[1]:.3f})")
        mo, mt = statistics.median(t_ours), statistics.median(t_torch)
        say(f"B={B} update_features median {mo:8.1f} us  min {min(t_ours):8.1f}  max {max(t_ours):8.1f}")
        say(f"B={B} torch loop      median {mt:8.1f} us  min {min(t_torch):8.1f}  max {max(t_torch):8.1f}")
        say(f"B={B} torch / fused = {mt / mo:.2f}  (medians of {a.rounds} alternating windows of {a.steps} batches, host clock)")

        # the scoring kernel alone (device events over `reps` back-to-back launches), without and with every optional output
        reps = 20
        counts = torch.zeros(3, device=dev, dtype=torch.int64)
        per_class = torch.zeros(2, C, device=dev, dtype=torch.int32)
        rank = torch.empty(B, device=dev, dtype=torch.int32)
        pred = torch.empty(B, 5, device=dev, dtype=torch.int32)
        logits = torch.empty(B, C, device=dev)
        for name, call in (("vtp_zs_topk (counts, per_class)", lambda: ops.zs_topk(f, zs.Wt, y, 100.0, B, C, D, counts, per_class)),
                           ("vtp_zs_topk (+ rank, pred, logits)", lambda: ops.zs_topk(f, zs.Wt, y, 100.0, B, C, D, counts, per_class, rank,
                                                                                        pred, logits))):
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / reps * 1e3
            say(f"  B={B}: {name:36s} {us:9.1f} us  {2.0 * B * C * D / us / 1e6:6.2f} TFLOP/s fp32 on {(B + 31) // 32} workgroups")

    # the classifier kernel alone: one class batch of the tool (10 classes x 80 templates) and all classes at once
    T = a.templates
    for nb in (10, C):
        feat = torch.randn(nb * T, D, device=dev)
        wt = torch.empty(nb, D, device=dev)
        call = lambda: ops.zs_class_mean(feat, wt, nb, T, D, 1e-12)
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            call()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 20 * 1e3
        say(f"  vtp_zs_class_mean {nb:5d} classes x {T} templates: {us:9.1f} us  {4.0 * nb * T * D / us / 1e6:6.3f} TB/s of its {4.0 * nb * T * D / 1e6:.1f} MB")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
