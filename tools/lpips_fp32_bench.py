#!/usr/bin/env python
"""Times LPIPS.enable_fp32_forward on one MI355X at the reconstruction tool's batch (B = 32, 256 x 256), seeded weights and images:

    fp32    LPIPS.forward with the switch on (chunks of FP32_CHUNK pairs), ms per call and algorithmic TFLOP/s of the 13 convolutions
    layers  each of the 13 vtp_conv2d_f32_blocked launches alone at the shape of one chunk: ms and TFLOP/s; conv1_1 with Cin = 3
            (scalar loads) and with Cin = 4 (a zero channel, 16-byte loads); the scale, max-pool and head launches in ms and GB/s
    layers1 the same with vtp_conv2d_f32 (one chain per output)
    bf16    LPIPS.forward as the trainer's kernel set computes it
    torch   oracle.lpips_oracle.lpips in fp32 on the same GPU (torch / MIOpen)

and prints the workspace bytes at the default chunk.  Without --what each runs as a child process of its own under its own time
limit, one after the other; the first that fails ends the run.  Every timing is a host clock around work that ends in a device
synchronise, after warm-up of the same shapes; --rounds windows of --iters calls each are printed (median and min)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def _layers(lp, dev, sync, chunk, H, W, iters, rounds, warmup, blocked=True):
    """every launch of one pass alone, on seeded data of its shape"""
    import torch
    from vtp_amd import ops
    from vtp_amd.lpips import CHNS, TAP_AFTER, VGG_CONVS
    op = lp._prep_fp32()
    nb = 2 * chunk
    g = torch.Generator().manual_seed(1)
    rows = []

    def timed(name, fn, flop=0.0, nbytes=0.0):
        t = _windows(fn, sync, iters, rounds, warmup)
        med = statistics.median(t)
        row = {"launch": name, "ms_median": med * 1e3, "ms_min": min(t) * 1e3}
        if flop:
            row["tflops"] = flop / med / 1e12
        if nbytes:
            row["gbytes_per_s"] = nbytes / med / 1e9
        rows.append(row)
        print(json.dumps(row), flush=True)

    img = (2 * torch.rand(chunk, 3, H, W, generator=g) - 1).to(dev)
    for cout in (3, 4):
        y = torch.empty(chunk, H, W, cout, device=dev)
        timed(f"scale_nhwc Cout={cout} [{chunk},3,{H},{W}]", lambda: ops.lpips_scale_nhwc_f32(img, y, op["shift"], op["scale"]),
              nbytes=4.0 * chunk * H * W * (3 + cout))
    h, w, cur, k = H, W, 1, 0
    for i, (sl, idx, cin, cout) in enumerate(VGG_CONVS):
        if sl != cur:
            x = torch.rand(nb, h, w, cin, generator=g).to(dev)
            y = torch.empty(nb, h // 2, w // 2, cin, device=dev)
            timed(f"maxpool2 [{nb},{h},{w},{cin}]", lambda: ops.maxpool2_f32(x, y), nbytes=4.0 * nb * h * w * cin * 1.25)
            h, w, cur = h // 2, w // 2, sl
        variants = [(cin, op["w"][i])]
        if i == 0:  # the first layer both ways, whichever the module uses
            w3 = op["w"][0][..., :3].contiguous()
            variants = [(3, w3), (4, torch.cat([w3, torch.zeros(cout, 3, 3, 1, device=dev)], 3).contiguous())]
        for ci, wt in variants:
            x = torch.rand(nb, h, w, ci, generator=g).to(dev)
            if ci == 4 and i == 0:
                x[..., 3] = 0
            y = torch.empty(nb, h, w, cout, device=dev)
            timed(f"conv{i:02d} slice{sl}.{idx} {ci}->{cout} [{nb},{h},{w}] K={9 * ci}",
                  lambda: ops.conv2d_f32(x, wt, op["b"][i], y, stride=1, pad=(1, 1), relu=True, blocked=blocked),
                  flop=2.0 * nb * h * w * 9 * cin * cout)
        if i == TAP_AFTER[k]:
            f = torch.rand(nb, h, w, cout, generator=g).to(dev)
            part = torch.empty(chunk, ops.lpips_head_segments(h * w), dtype=torch.float64, device=dev)
            timed(f"head tap{k} [{nb},{h},{w},{CHNS[k]}]", lambda: ops.lpips_head_f32(f, op["lin"][k], part),
                  nbytes=4.0 * nb * h * w * cout)
            k = min(k + 1, 4)
    return rows


def run(what, B, H, W, iters, rounds, warmup):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lpips_fp32_bench needs the MI355X: there is nothing to time on a CPU")
    from vtp_amd import LPIPS
    from vtp_amd.lpips import FP32_CHUNK
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    g = torch.Generator().manual_seed(0)
    x0 = 2 * torch.rand(B, 3, H, W, generator=g) - 1
    x1 = (x0 + 0.1 * torch.randn(B, 3, H, W, generator=g)).clamp(-1, 1)
    x0, x1 = x0.to(dev), x1.to(dev)
    lp = LPIPS().reset_parameters(0).to(dev)
    res = {"what": what, "B": B, "H": H, "W": W, "iters": iters, "rounds": rounds, "gflop_per_pair": 2 * LPIPS.forward_gflop(H, W)}
    if what in ("layers", "layers1"):
        chunk = min(FP32_CHUNK, B)
        res["chunk"] = chunk
        res["rows"] = _layers(lp, dev, sync, chunk, H, W, iters, rounds, warmup, blocked=what == "layers")
        conv = [r for r in res["rows"] if r["launch"].startswith("conv") and "3->64" not in r["launch"]]
        res["conv_ms_per_pass"] = sum(r["ms_median"] for r in conv)
        res["all_ms_per_pass"] = sum(r["ms_median"] for r in res["rows"]
                                     if "3->64" not in r["launch"] and "Cout=3" not in r["launch"])
        print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
        return
    if what == "fp32":
        lp.enable_fp32_forward()
        res["chunk"] = lp.fp32_chunk
        res["workspace_bytes"] = LPIPS.fp32_workspace_bytes(min(lp.fp32_chunk, B), H, W)
        fn = lambda: lp(x0, x1)
    elif what == "bf16":
        fn = lambda: lp(x0, x1)
    elif what == "torch":
        from oracle import lpips_oracle as L
        sd = {k: v.to(dev) for k, v in lp.state_dict().items()}
        no_grad = torch.no_grad()
        no_grad.__enter__()
        fn = lambda: L.lpips(sd, x0, x1)
    else:
        raise SystemExit(f"unknown --what {what}")
    t = _windows(fn, sync, iters, rounds, warmup)
    med, best = statistics.median(t), min(t)
    res.update(ms_per_call_median=med * 1e3, ms_per_call_min=best * 1e3, windows_ms=[round(v * 1e3, 3) for v in t],
               pairs_per_s_median=B / med, tflops_median=B * res["gflop_per_pair"] / med / 1e3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=["fp32", "layers", "layers1", "bf16", "torch"], default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=150, help="seconds each child may take")
    a = ap.parse_args()
    if a.what is not None:
        run(a.what, a.batch, a.size, a.size, a.iters, a.rounds, a.warmup)
        return 0
    for what in ("fp32", "layers", "layers1", "bf16", "torch"):
        cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--batch", str(a.batch), "--size", str(a.size), "--iters",
               str(a.iters), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"lpips_fp32_bench: {what} did not finish in {a.limit} s", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"lpips_fp32_bench: {what} ended with status {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
