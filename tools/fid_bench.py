#!/usr/bin/env python
"""Times the FID path on one MI355X at the tool's batch (B = 50, 299 x 299), seeded weights and images:

    ours   InceptionFeatures.forward (94 vtp_conv2d_f32 launches + pools), images/s and algorithmic TFLOP/s
    accum  FrechetStats.update on [50, 2048] features (vtp_fid_accum), us per call
    torch  the same network as tests/fid_ref.py writes it (F.conv2d + F.batch_norm + relu, fp32: torch / MIOpen), images/s

Without --what each of the three runs as a child process of its own under its own time limit, one after the other; the first
that fails ends the run.  Every timing is a host clock around work that ends in a device synchronise, after warm-up of the same
shapes; --rounds windows of --iters calls each are printed (median and min), so the spread is on the page."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _windows(fn, sync, iters, rounds, warmup):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / iters)
    return out


def run(what, B, iters, rounds, warmup, variant):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fid_bench needs the MI355X: there is nothing to time on a CPU")
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    x = torch.rand(B, 3, 299, 299, generator=torch.Generator().manual_seed(0)).to(dev)
    res = {"what": what, "B": B, "variant": variant, "iters": iters, "rounds": rounds}
    if what == "ours":
        from vtp_amd import InceptionFeatures
        from vtp_amd.fid import forward_gflop
        inc = InceptionFeatures(variant).reset_parameters(0).to(dev)
        t = _windows(lambda: inc(x), sync, iters, rounds, warmup)
        res["gflop_per_image"] = forward_gflop(299, 299)
    elif what == "torch":
        import fid_ref as R
        sd = {k: v.to(dev) for k, v in R.seeded_state_dict(0).items()}
        t = _windows(lambda: R.features(sd, x, variant), sync, iters, rounds, warmup)
        from vtp_amd.fid import forward_gflop
        res["gflop_per_image"] = forward_gflop(299, 299)
    elif what == "accum":
        from vtp_amd import FrechetStats
        st = FrechetStats(2048, dev)
        f = torch.randn(B, 2048, generator=torch.Generator().manual_seed(1)).to(dev)
        t = _windows(lambda: st.update(f), sync, iters * 10, rounds, warmup)
    else:
        raise SystemExit(f"unknown --what {what}")
    med, best = statistics.median(t), min(t)
    res.update(sec_per_call_median=med, sec_per_call_min=best, windows=[round(v, 6) for v in t])
    if what == "accum":
        res["us_per_call_median"] = med * 1e6
    else:
        res["images_per_s_median"] = B / med
        res["images_per_s_best"] = B / best
        res["tflops_median"] = B * res["gflop_per_image"] / med / 1e3
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=["ours", "accum", "torch"], default=None)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", default="torchvision", choices=["torchvision", "pytorch_fid"])
    ap.add_argument("--limit", type=int, default=180, help="seconds each child may take")
    a = ap.parse_args()
    if a.what is not None:
        run(a.what, a.batch, a.iters, a.rounds, a.warmup, a.variant)
        return 0
    for what in ("ours", "accum", "torch"):
        cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--batch", str(a.batch), "--iters", str(a.iters), "--rounds",
               str(a.rounds), "--warmup", str(a.warmup), "--variant", a.variant]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"fid_bench: {what} did not finish in {a.limit} s", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"fid_bench: {what} ended with status {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
