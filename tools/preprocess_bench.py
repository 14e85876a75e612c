#!/usr/bin/env python3
"""The first stage of the eval tools -- B = 32 decoded images through Resize + CenterCrop (probe_eval(256, 224)), Resize((256, 256))
bilinear (zero_shot(256)) and center_crop_arr (center_crop(256)) -- two ways:

  fused   vtp_amd.Preprocess (csrc/preprocess.hip: one launch per pass over the ragged batch, no host synchronisation): the host
          part (plan, tables, checks, copying the bytes into one pinned buffer), the device part from the pinned upload to the
          finished fp32 batch, and the kernels alone
  PIL     what the tools run today on the host (Image.resize / crop, then ToTensor + Normalize in numpy), in at most 16 worker
          processes that hold their sources already (no image crosses a pipe on the way in; the uint8 crops come back)

    python tools/preprocess_bench.py [--sources 500x375 2000x1500] [--steps 10] [--rounds 5] [--workers 16] [--out profiles/preprocess.log]

GPU timings are device events over windows of `steps` batches, median / min / max of `rounds` windows, after a warm-up of every
shape; the host part is wall clock.  The PIL pool is started (spawn) and measured before the GPU is touched.  Where PIL is there,
the fused bytes are compared with PIL's: the count of differing bytes is printed, and anything but 0 ends the run with an error."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PIPELINES = ("probe_eval", "zero_shot", "center_crop")


def sources(B, W, H):
    """smooth colourful images plus noise, as bytes, from a seed (the workers make the same ones)"""
    rng = np.random.default_rng([7, W, H])
    low = rng.normal(size=(B, H // 16 + 1, W // 16 + 1, 3))
    up = np.kron(low, np.ones((1, 16, 16, 1)))[:, :H, :W]
    return np.clip(128 + 60 * up + 12 * rng.normal(size=(B, H, W, 3)), 0, 255).astype(np.uint8)


# ---- PIL on the host (worker processes: numpy and PIL only) ---------------------------------------------------------------------
_SRC = {}


def pil_init(B, sizes):
    for W, H in sizes:
        _SRC[(W, H)] = sources(B, W, H)


def pil_one(job):
    from PIL import Image
    kind, W, H, b = job
    im = Image.fromarray(_SRC[(W, H)][b])
    if kind == "probe_eval":
        if W <= H:
            w, h = 256, int(256 * H / W)
        else:
            h, w = 256, int(256 * W / H)
        im = im.resize((w, h), Image.BICUBIC)
        top, left = int(round((h - 224) / 2.0)), int(round((w - 224) / 2.0))
        im = im.crop((left, top, left + 224, top + 224))
    elif kind == "zero_shot":
        im = im.resize((256, 256), Image.BILINEAR)
    else:
        while min(*im.size) >= 512:
            im = im.resize(tuple(x // 2 for x in im.size), resample=Image.BOX)
        s = 256 / min(*im.size)
        im = im.resize(tuple(round(x * s) for x in im.size), resample=Image.BICUBIC)
        arr = np.array(im)
        cy, cx = (arr.shape[0] - 256) // 2, (arr.shape[1] - 256) // 2
        im = Image.fromarray(arr[cy:cy + 256, cx:cx + 256])
    u8 = np.asarray(im)
    x = ((u8.astype(np.float32) / 255.0 - np.float32(MEAN)) / np.float32(STD)).transpose(2, 0, 1)  # ToTensor + Normalize: part of the work
    return u8, float(x[0, 0, 0])


def make(kind):
    from vtp_amd.preprocess import Preprocess
    return {"probe_eval": lambda: Preprocess.probe_eval(256, 224), "zero_shot": lambda: Preprocess.zero_shot(256),
            "center_crop": lambda: Preprocess.center_crop(256)}[kind]()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sources", nargs="+", default=["500x375", "2000x1500"], help="W x H")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--pil-batches", type=int, default=3)
    ap.add_argument("--no-pil", action="store_true")
    ap.add_argument("--no-gpu", action="store_true", help="the host parts alone (a rehearsal: no GPU timing is made up)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.batch
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sources]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say(f"# preprocessing of one batch: B={B} decoded images per source size, pipelines {', '.join(PIPELINES)}")
    pil = {}
    have_pil = False
    if not a.no_pil:
        try:
            import PIL
            have_pil = True
        except ImportError:
            say("PIL: not installed on this machine, not measured")
    if have_pil:  # before the GPU is initialised: the workers never see it
        import multiprocessing as mp
        workers = max(1, min(a.workers, 16, os.cpu_count() or 1))
        with mp.get_context("spawn").Pool(workers, initializer=pil_init, initargs=(B, sizes)) as pool:
            for W, H in sizes:
                for kind in PIPELINES:
                    jobs = [(kind, W, H, b) for b in range(B)]
                    res = pool.map(pil_one, jobs, chunksize=1)  # warm-up: imports and sources in the workers
                    ts = []
                    for _ in range(a.pil_batches):
                        t0 = time.perf_counter()
                        res = pool.map(pil_one, jobs, chunksize=1)
                        ts.append((time.perf_counter() - t0) * 1e3)
                    pil[(W, H, kind)] = (np.stack([r[0] for r in res]), statistics.median(ts))
                    say(f"source {W}x{H} {kind:11s}: PIL {PIL.__version__}, {workers} worker processes: median {statistics.median(ts):8.1f} ms per batch"
                        f"  min {min(ts):8.1f}  max {max(ts):8.1f}")

    data = {s: sources(B, *s) for s in sizes}
    for W, H in sizes:  # the host part of the fused path needs no GPU
        for kind in PIPELINES:
            pp = make(kind)
            images = list(data[(W, H)])
            pp.pack(images, pp.plan([(H, W)] * B))  # warm-up: the coefficient tables are cached
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                pk = pp.pack(images, pp.plan([(H, W)] * B))
                ts.append((time.perf_counter() - t0) * 1e3)
            say(f"source {W}x{H} {kind:11s}: host part (plan, checks, job rows, {pk.src.numel() / 1e6:.1f} MB into one buffer): median "
                f"{statistics.median(ts):8.2f} ms per batch  min {min(ts):8.2f}  max {max(ts):8.2f};  {len(pk.launches)} launches, "
                f"{len(pk.jobs)} job rows, {pk.tab.nbytes / 1e3:.1f} kB of tables, {pk.scratch_len / 1e6:.1f} MB of scratch")
    if a.no_gpu:
        say("GPU paths: not measured (--no-gpu)")
        return finish()

    import torch
    if not torch.cuda.is_available():
        sys.exit("preprocess_bench: the fused path needs the GPU (no CPU timing)")
    from vtp_amd import ops
    dev = "cuda"
    say(f"# device={torch.cuda.get_device_name(0)}")

    def events(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3

    def stats(ts):
        return f"median {statistics.median(ts):10.1f} us  min {min(ts):10.1f}  max {max(ts):10.1f}"

    wrong = 0
    for W, H in sizes:
        for kind in PIPELINES:
            pp = make(kind)
            images = list(data[(W, H)])
            plans = pp.plan([(H, W)] * B)
            pk = pp.pack(images, plans, pin=True)
            jobs_h = torch.from_numpy(pk.jobs.reshape(-1)).pin_memory()
            tab_h = torch.from_numpy(pk.tab).pin_memory()
            out = torch.empty(B, 3, pk.out_h, pk.out_w, device=dev)
            u8 = torch.empty(B, pk.out_h, pk.out_w, 3, dtype=torch.uint8, device=dev)
            scratch = torch.empty(max(pk.scratch_len, 1), dtype=torch.uint8, device=dev)
            src_d, jobs_d, tab_d = pk.src.to(dev), jobs_h.to(dev), tab_h.to(dev)
            kernels = lambda: ops.preprocess(src_d, scratch, jobs_d, tab_d, pk.launches, out, u8, MEAN, STD)

            def device_part():  # from the pinned upload to the finished output
                ops.preprocess(pk.src.to(dev, non_blocking=True), scratch, jobs_h.to(dev, non_blocking=True),
                               tab_h.to(dev, non_blocking=True), pk.launches, out, u8, MEAN, STD)

            whole = lambda: pp.apply(images, plans)
            for fn in (kernels, device_part, whole):  # warm-up: code objects, the pinned and device allocations
                fn()
                fn()
            torch.cuda.synchronize()
            if (W, H, kind) in pil:
                diff = int((u8.cpu().numpy() != pil[(W, H, kind)][0]).sum())
                wrong += diff
                say(f"source {W}x{H} {kind:11s}: fused bytes against PIL's: {diff} of {u8.numel()} differ")
            res = {"kernels alone": [], "pinned upload + kernels": [], "Preprocess.apply (host part included)": []}
            for _ in range(a.rounds):
                res["kernels alone"].append(events(kernels, a.steps))
                res["pinned upload + kernels"].append(events(device_part, a.steps))
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    whole()
                torch.cuda.synchronize()
                res["Preprocess.apply (host part included)"].append((time.perf_counter() - t0) / a.steps * 1e6)
            for k, ts in res.items():
                say(f"source {W}x{H} {kind:11s}: {k:38s} {stats(ts)}  per batch")
            mk, mu = statistics.median(res["kernels alone"]), statistics.median(res["pinned upload + kernels"])
            tail = f";  PIL / (upload + kernels) = {pil[(W, H, kind)][1] * 1e3 / mu:.1f}" if (W, H, kind) in pil else ""
            say(f"source {W}x{H} {kind:11s}: {len(pk.launches)} launches, kernels alone = {pk.src.numel() / mk / 1e3:.1f} GB/s of source bytes; "
                f"the upload of {pk.src.numel() / 1e6:.1f} MB takes {(mu - mk) / mu * 100:.0f} % of upload + kernels{tail}")
    finish()
    if wrong:
        sys.exit(f"preprocess_bench: {wrong} bytes differ from PIL")


if __name__ == "__main__":
    main()
