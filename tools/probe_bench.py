#!/usr/bin/env python3
"""Linear-probe step at the reference tool's default shape (B = 128, D = 768, the 2 x 13 sweep -> 2 x 12 heads, 1000 classes), features
given: vtp_amd.LinearProbe.step_features against the torch loop a user of the tool runs today (nn.Linear heads, CrossEntropyLoss,
torch.optim.SGD with momentum, CosineAnnealingLR -- the loop oracle/tools_oracle.py:176-190 restates), plus the three kernels alone
with their achieved bytes/s (logits: 4 N K bytes of weights, sgd: 16 N K bytes -- W and mW read and written once).

    python tools/probe_bench.py [--steps 20] [--rounds 5] [--out profiles/probe_step.log]

Both loops get their inputs ready-made (X_all for ours, one contiguous input per feature group for torch) and are timed in
alternating windows of `steps` steps, each closed by a device synchronise; the figure of record is the median window."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_bench: needs the GPU (no CPU timing)")
    from vtp_amd import ops
    from vtp_amd.probe import LinearProbe
    dev = "cuda"
    B, D, C = a.batch, a.dim, a.classes
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    probe = LinearProbe.from_sweep(None, batch_size=B, num_classes=C, max_iter=100000, embed_dim=D)
    x_all = torch.randn(B, (probe.n_max + 1) * D, device=dev)
    labels = torch.randint(0, C, (B,), device=dev)
    n_par = sum(g.weight.numel() + g.bias.numel() for g in probe.groups)
    say(f"# probe step: B={B} D={D} classes={C} heads={len(probe.keys)} groups={[(g.H, g.K) for g in probe.groups]} parameters={n_par / 1e6:.1f} M "
        f"device={torch.cuda.get_device_name(0)}")

    # the torch loop: one nn.Linear per head with the same initial weights, one optimizer parameter group per head
    heads, params = [], []
    lrs = probe.learning_rates(0)
    for g in probe.groups:
        xin = x_all[:, g.col0:g.col0 + g.K].contiguous()
        for i, k in enumerate(g.keys):
            lin = torch.nn.Linear(g.K, C).to(dev)
            with torch.no_grad():
                lin.weight.copy_(g.weight[i])
                lin.bias.copy_(g.bias[i])
            heads.append((lin, xin))
            params.append({"params": lin.parameters(), "lr": lrs[k]})
    opt = torch.optim.SGD(params, momentum=0.9, weight_decay=0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 100000, eta_min=0)
    crit = torch.nn.CrossEntropyLoss()

    def torch_step():
        loss = sum(crit(lin(xin), labels) for lin, xin in heads)
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        return loss

    def ours_step():
        return probe.step_features(x_all, labels).sum()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3, float(out.detach())

    for fn in (ours_step, torch_step):  # warm-up: code objects, library algorithm choice, optimizer state
        for _ in range(3):
            fn()
    t_ours, t_torch = [], []
    for r in range(a.rounds):
        to, lo = window(ours_step)
        tt, lt = window(torch_step)
        t_ours.append(to)
        t_torch.append(tt)
        say(f"round {r}: fused {to:8.3f} ms/step (loss sum {lo:.4f})   torch {tt:8.3f} ms/step (loss sum {lt:.4f})")
    mo, mt = statistics.median(t_ours), statistics.median(t_torch)
    say(f"step_features   median {mo:8.3f} ms  min {min(t_ours):8.3f} ms  max {max(t_ours):8.3f} ms")
    say(f"torch loop      median {mt:8.3f} ms  min {min(t_torch):8.3f} ms  max {max(t_torch):8.3f} ms")
    say(f"torch / fused = {mt / mo:.2f}  (medians of {a.rounds} alternating windows of {a.steps} steps, host clock around a device synchronise)")

    # the kernels alone (device events over `reps` back-to-back launches; learning rates 0 so that the weights stay put)
    reps = 20
    for g in probe.groups:
        N = g.H * C
        logits, dlogits, _ = probe._bufs(g, B)
        xs = x_all[:, g.col0:g.col0 + g.K]
        g.lr.zero_()
        loss = torch.zeros(g.H, device=dev)
        calls = (("vtp_probe_logits", 4.0 * N * g.K, lambda: ops.probe_logits(xs, g.weight, g.bias, logits, B, N, g.K)),
                 ("vtp_probe_ce", None, lambda: ops.probe_ce(logits, labels, B, g.H, C, 1.0 / B, loss, None, dlogits)),
                 ("vtp_probe_sgd", 16.0 * N * g.K, lambda: ops.probe_sgd(g.weight, g.bias, g.m_weight, g.m_bias, dlogits, xs, g.lr, B, g.H, C,
                                                                          g.K, 0.9)))
        for name, nbytes, call in calls:
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / reps * 1e3
            rate = f"{nbytes / us / 1e6:7.2f} TB/s of its {nbytes / 1e6:.0f} MB" if nbytes else "(L2-resident)"
            flops = 2.0 * B * N * g.K
            tf = f"  {flops / us / 1e6:6.1f} TFLOP/s fp32" if nbytes else ""
            say(f"  group N={N} K={g.K}: {name:17s} {us:9.1f} us  {rate}{tf}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
