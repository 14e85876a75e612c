#!/usr/bin/env python3
"""Segmentation-probe step and evaluation at the ADE20k shape (B = 16, 32 x 32 cells, K = 768, C = 150, 512 x 512 labels) for H = 1
and H = 4 heads, features given: vtp_amd.SegProbe.step_features / evaluate_features next to the torch formulation a user runs
today, in fp32 on the same GPU: matmul, F.interpolate(bilinear), F.cross_entropy(ignore_index=255), autograd and a hand SGD step
with momentum (evaluation: argmax + bincount).  That side is several passes over [B, C, 512, 512] tensors in memory against one
fused pass that never stores them -- a comparison of two ways to get the number, not kernel against kernel.

    python tools/segprobe_bench.py [--heads 1 4] [--reps 5] [--limit 180] [--out profiles/segprobe.log]

Every (side, H) measurement runs in a child process of its own under its own time limit, one after the other; the first child that
fails or runs out of time ends the bench (nothing else is started on the device) and the log says so.  A child warms up twice, then
times `reps` steps and `reps` evaluations with device events (median of record), the fused kernels one by one, and reads the rise
of torch.cuda.max_memory_allocated() over one step."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, HW, K, C, HL, IGNORE, MOMENTUM, LR = 16, 32, 768, 150, 512, 255, 0.9, 0.01


def _inputs(torch, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B * HW * HW, K, device=dev, generator=g)
    y = torch.randint(0, C, (B, HL, HL), device=dev, generator=g, dtype=torch.uint8)
    y[torch.rand(B, HL, HL, device=dev, generator=g) < 0.1] = IGNORE
    return x, y


def _median_ms(torch, fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def _peak_rise(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def child_fused(H, reps):
    import torch
    from vtp_amd import SegProbe, ops
    dev = "cuda"
    x, y = _inputs(torch, dev)
    torch.manual_seed(0)
    probe = SegProbe(None, [(f"h{i}", 1, LR) for i in range(H)], C, embed_dim=K)
    hw = (HW, HW)
    step, evaluate = (lambda: probe.step_features(x, hw, y)), (lambda: probe.evaluate_features(x, hw, y))
    for fn in (step, evaluate):
        fn(), fn()
    res = dict(side="fused", H=H, step_ms=_median_ms(torch, step, reps), eval_ms=_median_ms(torch, evaluate, reps),
               step_peak=_peak_rise(torch, step), eval_peak=_peak_rise(torch, evaluate), loss=float(step()[0]))
    # the kernels one by one, on buffers of their own (learning rate 0: the weights stay put)
    g = probe.groups[0]
    M, N = B * HW * HW, H * C
    f32 = dict(device=dev, dtype=torch.float32)
    z, grad, lse = torch.empty(M, N, **f32), torch.empty(M, N, **f32), torch.empty(H, B, HL, HL, **f32)
    loss, cc = torch.zeros(H, **f32), torch.zeros(2, device=dev, dtype=torch.int32)
    conf = torch.zeros(H, C, C, device=dev, dtype=torch.int64)
    ws_ce = torch.empty(ops.seg_ce_workspace_bytes(B, HW, HW, HL, HL, H, C), device=dev, dtype=torch.uint8)
    n_sgd = max(1, min(H, probe._head_chunk(g, M)))
    ws_sgd = torch.empty(ops.seg_sgd_workspace_bytes(M, n_sgd * C, K), device=dev, dtype=torch.uint8)
    lr0 = torch.zeros(H, **f32)
    calls = (("vtp_probe_logits", lambda: ops.probe_logits(x, g.weight, g.bias, z, M, N, K)),
             ("vtp_seg_ce (training: lse)", lambda: ops.seg_ce(z, y, hw, H, C, IGNORE, loss, cc, ws_ce, lse=lse)),
             ("vtp_seg_ce (evaluation: confusion)", lambda: ops.seg_ce(z, y, hw, H, C, IGNORE, loss, cc, ws_ce, conf=conf)),
             ("vtp_seg_dlogits", lambda: ops.seg_dlogits(z, y, hw, H, C, IGNORE, lse, cc, grad)),
             (f"vtp_seg_sgd ({n_sgd} of {H} heads)", lambda: ops.seg_sgd(g.weight[:n_sgd], g.bias[:n_sgd], g.m_weight[:n_sgd], g.m_bias[:n_sgd],
                                                                      grad, x, lr0, M, n_sgd, C, K, MOMENTUM, ws_sgd)))
    res["kernels_us"] = {}
    for name, call in calls:
        call()
        res["kernels_us"][name] = _median_ms(torch, call, reps) * 1e3
    print("RESULT " + json.dumps(res), flush=True)


def child_torch(H, reps):
    import torch
    import torch.nn.functional as F
    dev = "cuda"
    x, y = _inputs(torch, dev)
    y64 = y.long()
    torch.manual_seed(0)
    Ws = [torch.empty(C, K).normal_(0, 0.01).to(dev).requires_grad_(True) for _ in range(H)]
    bs = [torch.zeros(C, device=dev, requires_grad=True) for _ in range(H)]
    moms = [torch.zeros_like(p) for p in Ws + bs]
    conf = torch.zeros(H, C * C, device=dev, dtype=torch.int64)

    def up(W, b):
        z = (x @ W.T + b).view(B, HW, HW, C).permute(0, 3, 1, 2)
        return F.interpolate(z, size=(HL, HL), mode="bilinear", align_corners=False)

    def step():
        losses = [F.cross_entropy(up(W, b), y64, ignore_index=IGNORE) for W, b in zip(Ws, bs)]
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
                u = up(W, b)
                out.append(F.cross_entropy(u, y64, ignore_index=IGNORE))
                ok = y64 != IGNORE
                conf[i] += torch.bincount(y64[ok] * C + u.argmax(1)[ok], minlength=C * C)
            return torch.stack(out)

    for fn in (step, evaluate):
        fn(), fn()
    res = dict(side="torch", H=H, step_ms=_median_ms(torch, step, reps), eval_ms=_median_ms(torch, evaluate, reps),
               step_peak=_peak_rise(torch, step), eval_peak=_peak_rise(torch, evaluate), loss=float(step()[0]))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=180, help="seconds a child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, metavar=("SIDE", "H"), default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("segprobe_bench: needs the GPU (no CPU timing)")
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

    say(f"# segmentation probe: B={B} cells={HW}x{HW} K={K} C={C} labels={HL}x{HL} (10 % ignored) device={torch.cuda.get_device_name(0)}; "
        f"one [B, C, {HL}, {HL}] fp32 tensor = {B * C * HL * HL * 4 / 1e9:.2f} GB; medians of {a.reps} (device events)")
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
            mf, mt = f[key + "_ms"], t[key + "_ms"]
            say(f"H={H} {what:17s} fused {mf:9.3f} ms  peak +{f[key + '_peak'] / 1e6:9.1f} MB   torch {mt:9.3f} ms  peak +{t[key + '_peak'] / 1e6:9.1f} MB   "
                f"torch / fused = {mt / mf:.2f}" + ("" if mt >= mf else "   ** the torch formulation is FASTER here **"))
        say(f"H={H} loss after the timed steps: fused {f['loss']:.4f}  torch {t['loss']:.4f}")
        for name, us in f["kernels_us"].items():
            say(f"  H={H}: {name:40s} {us:10.1f} us")
    finish(0)


if __name__ == "__main__":
    main()
