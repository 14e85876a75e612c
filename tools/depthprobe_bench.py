#!/usr/bin/env python3
"""Depth-probe step and evaluation at the NYUv2-like shape (B = 16, 32 x 32 cells, K = 768, 256 bins, 512 x 512 labels) for H = 1
and H = 4 heads, features given: vtp_amd.DepthProbe.step_features / evaluate_features next to the torch formulation a user runs
today, in fp32 on the same GPU: matmul, F.interpolate(bilinear), relu + 0.1, the normalised bin expectation, the scale-invariant
log loss, autograd and a hand SGD step with momentum (evaluation: the nine metric sums).  That side is several passes over
[B, 256, 512, 512] tensors in memory against one fused pass that never stores them -- a comparison of two ways to get the number,
not kernel against kernel.

    python tools/depthprobe_bench.py [--heads 1 4] [--reps 20] [--limit 240] [--out profiles/depthprobe.log]

Every (side, H) measurement runs in a child process of its own under its own time limit, one after the other; the first child that
fails or runs out of time ends the bench (nothing else is started on the device) and the log says so.  A child warms up twice, then
times `reps` steps and `reps` evaluations with device events (median, with the smallest and largest of the record), the fused
kernels one by one, and reads the rise of torch.cuda.max_memory_allocated() over one step."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, HW, K, C, HL, MOMENTUM, LR, LO, HI, LAM = 16, 32, 768, 256, 512, 0.9, 0.01, 0.001, 10.0, 0.85


def _inputs(torch, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B * HW * HW, K, device=dev, generator=g)
    y = LO + (HI - LO) * torch.rand(B, HL, HL, device=dev, generator=g)
    y[torch.rand(B, HL, HL, device=dev, generator=g) < 0.1] = 0.0
    return x, y


def _times_ms(torch, fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return [statistics.median(out), min(out), max(out)]


def _peak_rise(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def child_fused(H, reps):
    import torch
    from vtp_amd import DepthProbe, ops
    dev = "cuda"
    x, y = _inputs(torch, dev)
    torch.manual_seed(0)
    probe = DepthProbe(None, [(f"h{i}", 1, LR) for i in range(H)], LO, HI, C, LAM, MOMENTUM, embed_dim=K)
    hw = (HW, HW)
    step, evaluate = (lambda: probe.step_features(x, hw, y)), (lambda: probe.evaluate_features(x, hw, y))
    for fn in (step, evaluate):
        fn(), fn()
    res = dict(side="fused", H=H, step_ms=_times_ms(torch, step, reps), eval_ms=_times_ms(torch, evaluate, reps),
               step_peak=_peak_rise(torch, step), eval_peak=_peak_rise(torch, evaluate), loss=float(step()[0]))
    # the kernels one by one, on buffers of their own (learning rate 0: the weights stay put)
    g = probe.groups[0]
    M, N = B * HW * HW, H * C
    f32 = dict(device=dev, dtype=torch.float32)
    z, grad = torch.empty(M, N, **f32), torch.empty(M, N, **f32)
    loss, stats = torch.zeros(H, **f32), torch.zeros(H, 4, device=dev, dtype=torch.float64)
    counts, sums = torch.zeros(H, 4, device=dev, dtype=torch.int64), torch.zeros(H, 6, device=dev, dtype=torch.float64)
    ws = torch.empty(ops.depth_pix_workspace_bytes(B, HW, HW, HL, HL, H, C), device=dev, dtype=torch.uint8)
    aux = torch.empty(ops.depth_pix_workspace_bytes(B, HW, HW, HL, HL, H, C, aux=True), device=dev, dtype=torch.uint8)
    n_sgd = max(1, min(H, probe._head_chunk(g, M)))
    ws_sgd = torch.empty(ops.depth_sgd_workspace_bytes(M, n_sgd * C, K), device=dev, dtype=torch.uint8)
    lr0 = torch.zeros(H, **f32)
    rng = (LO, HI, LAM)
    calls = (("vtp_probe_logits", lambda: ops.probe_logits(x, g.weight, g.bias, z, M, N, K)),
             ("vtp_depth_pix (training: aux)", lambda: ops.depth_pix(z, y, hw, H, C, *rng, aux=aux, loss=loss, stats=stats, workspace=ws)),
             ("vtp_depth_pix (evaluation: counters)", lambda: ops.depth_pix(z, y, hw, H, C, *rng, loss=loss, stats=stats, workspace=ws,
                                                                           eval_counts=counts, eval_sums=sums)),
             ("vtp_depth_dlogits", lambda: ops.depth_dlogits(z, (B, HL, HL), hw, H, C, *rng, aux, stats, grad)),
             (f"vtp_depth_sgd ({n_sgd} of {H} heads)", lambda: ops.depth_sgd(g.weight[:n_sgd], g.bias[:n_sgd], g.m_weight[:n_sgd],
                                                                          g.m_bias[:n_sgd], grad, x, lr0, M, n_sgd, C, K, MOMENTUM, ws_sgd)))
    res["kernels_us"] = {}
    for name, call in calls:
        call()
        res["kernels_us"][name] = _times_ms(torch, call, reps)[0] * 1e3
    print("RESULT " + json.dumps(res), flush=True)


def child_torch(H, reps):
    import math
    import torch
    import torch.nn.functional as F
    dev = "cuda"
    x, y = _inputs(torch, dev)
    ok = (y > 0) & (y <= HI)
    n = ok.sum()
    logy = torch.where(ok, y, torch.ones_like(y)).log()
    e = torch.linspace(LO, HI, C, device=dev).view(1, C, 1, 1)
    torch.manual_seed(0)
    Ws = [torch.empty(C, K).normal_(0, 0.01).to(dev).requires_grad_(True) for _ in range(H)]
    bs = [torch.zeros(C, device=dev, requires_grad=True) for _ in range(H)]
    moms = [torch.zeros_like(p) for p in Ws + bs]
    acc = torch.zeros(H, 9, device=dev, dtype=torch.float64)

    def depth(W, b):
        z = (x @ W.T + b).view(B, HW, HW, C).permute(0, 3, 1, 2)
        a = F.relu(F.interpolate(z, size=(HL, HL), mode="bilinear", align_corners=False)) + 0.1
        return (a * e).sum(1) / a.sum(1)

    def silog(d):
        g = (d.log() - logy) * ok
        return torch.sqrt(((g * g).sum() / n - LAM * (g.sum() / n) ** 2).clamp_min(0.0)), g

    def step():
        losses = [silog(depth(W, b))[0] for W, b in zip(Ws, bs)]
        grads = torch.autograd.grad(sum(losses), Ws + bs)
        with torch.no_grad():
            for p, m, g in zip(Ws + bs, moms, grads):
                m.mul_(MOMENTUM).add_(g)
                p.sub_(LR * m)
        return torch.stack(losses).detach()

    def evaluate():
        with torch.no_grad():
            out = []
            for i, (W, b) in enumerate(zip(Ws, bs)):
                d = depth(W, b)
                loss, g = silog(d)
                out.append(loss)
                dd, tt, gg = d[ok].double(), y[ok].double(), g[ok].double()
                ratio = torch.maximum(dd / tt, tt / dd)
                diff = dd - tt
                acc[i] += torch.stack([gg.sum(), (gg * gg).sum(), (diff.abs() / tt).sum(), (diff * diff / tt).sum(), (diff * diff).sum(),
                                       gg.abs().sum() / math.log(10.0), (ratio < 1.25).sum(), (ratio < 1.25 ** 2).sum(),
                                       (ratio < 1.25 ** 3).sum()])
            return torch.stack(out)

    for fn in (step, evaluate):
        fn(), fn()
    res = dict(side="torch", H=H, step_ms=_times_ms(torch, step, reps), eval_ms=_times_ms(torch, evaluate, reps),
               step_peak=_peak_rise(torch, step), eval_peak=_peak_rise(torch, evaluate), loss=float(step()[0]))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, metavar=("SIDE", "H"), default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("depthprobe_bench: needs the GPU (no CPU timing)")
    if a.child:
        (child_fused if a.child[0] == "fused" else child_torch)(int(a.child[1]), a.reps)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish(code):
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        sys.exit(code)

    say(f"# depth probe: B={B} cells={HW}x{HW} K={K} bins={C} labels={HL}x{HL} (10 % invalid) device={torch.cuda.get_device_name(0)}; "
        f"one [B, {C}, {HL}, {HL}] fp32 tensor = {B * C * HL * HL * 4 / 1e9:.2f} GB; medians of {a.reps} after 2 warm-up calls "
        f"(device events; min .. max of the record in brackets)")
    for H in a.heads:
        got = {}
        for side in ("fused", "torch"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", side, str(H), "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                say(f"H={H} {side}: no result within {a.limit} s -- stopped here, nothing else was started")
                finish(1)
            hit = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not hit:
                say(f"H={H} {side}: child failed (exit {r.returncode}) -- stopped here, nothing else was started\n{r.stderr[-1500:]}")
                finish(1)
            got[side] = json.loads(hit[-1][7:])
        f, t = got["fused"], got["torch"]
        for what, key in (("step_features", "step"), ("evaluate_features", "eval")):
            (mf, f0, f1), (mt, t0, t1) = f[key + "_ms"], t[key + "_ms"]
            say(f"H={H} {what:17s} fused {mf:9.3f} ms [{f0:.3f} .. {f1:.3f}]  peak +{f[key + '_peak'] / 1e6:9.1f} MB   "
                f"torch {mt:9.3f} ms [{t0:.3f} .. {t1:.3f}]  peak +{t[key + '_peak'] / 1e6:9.1f} MB   "
                f"torch / fused = {mt / mf:.2f}" + ("" if mt >= mf else "   ** the torch formulation is FASTER here **"))
        say(f"H={H} loss after the timed steps: fused {f['loss']:.4f}  torch {t['loss']:.4f}")
        for name, us in f["kernels_us"].items():
            say(f"  H={H}: {name:40s} {us:10.1f} us")
    finish(0)


if __name__ == "__main__":
    main()
