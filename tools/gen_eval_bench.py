#!/usr/bin/env python
"""Times what GenEval adds to the FID path on one MI355X at the tool's batch (B = 50, 299 x 299), seeded weights and inputs:

    forward        InceptionFeatures.forward (the pool features alone)
    forward_taps   the same pass with the sFID tap (one more vtp_conv2d_f32 launch, Cout = 7)
    is_update      InceptionScore.update on [50, 2048] features, C = 1000: vtp_gemm_nt_f32 + vtp_is_rows + vtp_is_accum
    is_torch       a torch restatement of that update on the same GPU: fp32 matmul + bias, fp64 softmax / log_softmax, the sums
                   added to an fp64 state

and prints the three ratios forward_taps / forward, is_update / forward, is_update / is_torch.  Every timing is a host clock
around work that ends in a device synchronise, after warm-up of the same shapes; --rounds windows of --iters calls each are
printed (median and min), so the spread is on the page.  The windows of the two sides of a ratio alternate."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _windows(fns, sync, iters, rounds, warmup):
    """per function the seconds per call of `rounds` windows; the functions take turns window by window"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    sync()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for fn, ts in zip(fns, out):
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            sync()
            ts.append((time.perf_counter() - t0) / iters)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", default="torchvision", choices=["torchvision", "pytorch_fid"])
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gen_eval_bench needs the MI355X: there is nothing to time on a CPU")
    from vtp_amd import InceptionFeatures, InceptionScore
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    B, C, D = a.batch, a.classes, 2048
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, 299, 299, generator=g).to(dev)
    f = torch.randn(B, D, generator=g).abs().to(dev)
    W = torch.randn(C, D, generator=g) * (6.0 / D ** 0.5)
    b = 0.1 * torch.randn(C, generator=g)
    inc = InceptionFeatures(a.variant).reset_parameters(0).to(dev)
    isc = InceptionScore(W, b, split_size=5000, device=dev)
    Wg, bg = W.to(dev), b.to(dev)
    state = torch.zeros(1, 1 + C, device=dev, dtype=torch.float64)

    def is_torch():
        lg = (f @ Wg.t() + bg).double()
        p, logp = torch.softmax(lg, 1), torch.log_softmax(lg, 1)
        state[0, 0] += (p * logp).sum()
        state[0, 1:] += p.sum(0)

    def is_update():
        if isc.n >= 5000 - B:  # stay inside one split: the state does not grow while the clock runs
            isc.reset()
        isc.update(f)

    lines = []

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    def stat(what, ts, **kw):
        res = {"what": what, "B": B, "iters": kw.pop("iters", a.iters), "rounds": a.rounds, "sec_per_call_median": statistics.median(ts),
               "sec_per_call_min": min(ts), "windows": [round(v, 7) for v in ts]}
        res.update(kw)
        emit(res)
        return res["sec_per_call_median"]

    t_fwd, t_taps = _windows([lambda: inc(x), lambda: inc.forward_taps(x)], sync, a.iters, a.rounds, a.warmup)
    m_fwd = stat("forward", t_fwd, variant=a.variant)
    m_taps = stat("forward_taps", t_taps, variant=a.variant)
    t_upd, t_torch = _windows([is_update, is_torch], sync, 10 * a.iters, a.rounds, a.warmup)
    m_upd = stat("is_update", t_upd, classes=C, iters=10 * a.iters)
    m_torch = stat("is_torch", t_torch, classes=C, iters=10 * a.iters)
    emit({"what": "ratios", "forward_taps_over_forward": m_taps / m_fwd, "is_update_over_forward": m_upd / m_fwd,
          "is_update_over_is_torch": m_upd / m_torch})
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
