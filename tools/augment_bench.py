#!/usr/bin/env python3
"""The SSL crops of one training batch -- B = 32 images, DINO defaults (2 x 256 + 8 x 96 crops per image) -- three ways:

  fused   vtp_amd.MultiCrop.apply (csrc/augment.hip: two launches per output size, no host synchronisation), from byte images on
          the device, from byte images on the host (pinned upload), and the kernels alone
  torch   the same chain written with torch ops on the same GPU, crop by crop (F.interpolate(bicubic, antialias) of the box,
          the colour operations of torchvision's float-tensor path, conv2d blur), driven by the same tables
  PIL     the pipeline users run today on the host (crop + resize BICUBIC, ImageEnhance jitter, HSV hue, GaussianBlur, solarize,
          ToTensor + Normalize), in at most 16 worker processes

    python tools/augment_bench.py [--sizes 256 512] [--steps 10] [--rounds 5] [--workers 16] [--out profiles/augment.log]

GPU timings are device events over windows of `steps` batches, fused and torch alternating, median / min / max of `rounds`
windows.  The PIL pool is started (spawn) and measured before the GPU is touched: wall clock over whole batches.  Host
synchronisations are counted with torch's sync debug mode.  The draw of the tables (host, numpy) is timed separately."""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def sizes_of(tables):
    return [256, 96][:len(tables)]


# ---- PIL on the host (worker processes: numpy and PIL only) ---------------------------------------------------------------------
def pil_crop(img, r, S):
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps
    y0, x0, h, w = (int(v) for v in r[0:4])
    flags = int(r[4])
    im = img.crop((x0, y0, x0 + w, y0 + h)).resize((S, S), Image.BICUBIC)
    if flags & 1:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if flags & 2:
        for op in (int(o) for o in r[5:9]):
            if op == 0:
                im = ImageEnhance.Brightness(im).enhance(float(r[9]))
            elif op == 1:
                im = ImageEnhance.Contrast(im).enhance(float(r[10]))
            elif op == 2:
                im = ImageEnhance.Color(im).enhance(float(r[11]))
            elif op == 3:
                hh, ss, vv = im.convert("HSV").split()
                a = np.array(hh, dtype=np.uint8)
                with np.errstate(over="ignore"):
                    a += np.uint8(int(float(r[12]) * 255) % 256)
                im = Image.merge("HSV", (Image.fromarray(a, "L"), ss, vv)).convert("RGB")
    if flags & 4:
        im = im.convert("L").convert("RGB")
    if float(r[13]) > 0:
        im = im.filter(ImageFilter.GaussianBlur(radius=float(r[13])))
    if flags & 8:
        im = ImageOps.solarize(im, 128)
    x = np.asarray(im, dtype=np.float32) / 255.0
    return ((x - np.float32(MEAN)) / np.float32(STD)).transpose(2, 0, 1)


def pil_image(job):
    """all crops of one image: (u8 [Hs, Ws, 3], [(row, S), ...]) -> list of f32 [3, S, S]"""
    from PIL import Image
    u8, rows = job
    img = Image.fromarray(u8)
    return [pil_crop(img, r, S) for r, S in rows]


def pil_batch(pool, u8, tables, sizes):
    B = u8.shape[0]
    jobs = [(u8[b], [(t[v * B + b], S) for t, S in zip(tables, sizes) for v in range(len(t) // B)]) for b in range(B)]
    crops = pool.map(pil_image, jobs, chunksize=1)
    out, k = [], 0
    for t in tables:  # view-major, as the fused path lays them out
        V = len(t) // B
        out.append(np.stack([crops[b][k + v] for v in range(V) for b in range(B)]))
        k += V
    return out


# ---- the chain in torch ops on the GPU ----------------------------------------------------------------------------------------------
def torch_crop(x, r, S, mean, std):
    """x f32 [3, Hs, Ws] in [0, 1] on the device, r one table row (numpy) -> f32 [3, S, S]"""
    import torch
    import torch.nn.functional as F
    gray = lambda t: (0.2989 * t[0] + 0.587 * t[1] + 0.114 * t[2]).unsqueeze(0)
    blend = lambda a, b, f: (f * a + (1.0 - f) * b).clamp(0, 1)
    y0, x0, h, w = (int(v) for v in r[0:4])
    flags = int(r[4])
    x = F.interpolate(x[None, :, y0:y0 + h, x0:x0 + w], (S, S), mode="bicubic", antialias=True, align_corners=False)[0].clamp(0, 1)
    if flags & 1:
        x = x.flip(-1)
    if flags & 2:
        for op in (int(o) for o in r[5:9]):
            if op == 0:
                x = blend(x, torch.zeros_like(x), float(r[9]))
            elif op == 1:
                x = blend(x, gray(x).mean(), float(r[10]))
            elif op == 2:
                x = blend(x, gray(x), float(r[11]))
            elif op == 3:
                rr, gg, bb = x.unbind(0)
                maxc, minc = x.max(0).values, x.min(0).values
                eqc = maxc == minc
                cr = maxc - minc
                ones = torch.ones_like(maxc)
                s = cr / torch.where(eqc, ones, maxc)
                dv = torch.where(eqc, ones, cr)
                rc, gc, bc = (maxc - rr) / dv, (maxc - gg) / dv, (maxc - bb) / dv
                hr = (maxc == rr) * (bc - gc)
                hg = ((maxc == gg) & (maxc != rr)) * (2.0 + rc - bc)
                hb = ((maxc != gg) & (maxc != rr)) * (4.0 + gc - rc)
                hh = (torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0) + float(r[12])) % 1.0
                i = torch.floor(hh * 6.0)
                f = hh * 6.0 - i
                i = i.to(torch.int64) % 6
                v = maxc
                p, q, t = (v * (1.0 - s)).clamp(0, 1), (v * (1.0 - f * s)).clamp(0, 1), (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
                pick = lambda *o: torch.stack(o).gather(0, i[None])[0]
                x = torch.stack((pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q)))
    if flags & 4:
        x = gray(x).expand(3, -1, -1)
    if float(r[13]) > 0:
        tt = torch.linspace(-4, 4, 9, device=x.device)
        pdf = torch.exp(-0.5 * (tt / float(r[13])).pow(2))
        k1 = pdf / pdf.sum()
        k2 = (k1[:, None] * k1[None, :]).expand(3, 1, 9, 9).contiguous()
        x = F.conv2d(F.pad(x[None], (4, 4, 4, 4), mode="reflect"), k2, groups=3)[0]
    if flags & 8:
        x = torch.where(x >= 128.0 / 255.0, 1.0 - x, x)
    return (x - mean) / std


def torch_batch(u8, tables, sizes, mean, std):
    import torch
    B = u8.shape[0]
    x = u8.permute(0, 3, 1, 2).float() / 255.0
    return [torch.stack([torch_crop(x[n % B], t[n], S, mean, std) for n in range(len(t))]) for t, S in zip(tables, sizes)]


def count_syncs(fn):
    """host synchronisations torch reports while fn runs (sync debug mode 'warn')"""
    import torch
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("called a synchronizing" in str(m.message) for m in w)  # not the mode's own "prototype feature" notice


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--pil-batches", type=int, default=3)
    ap.add_argument("--no-pil", action="store_true")
    ap.add_argument("--no-gpu", action="store_true", help="the PIL part alone (a rehearsal: no GPU timing is made up)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vtp_amd.augment import MultiCrop
    B = a.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    rng = np.random.default_rng(0)
    data = {}
    for hs in a.sizes:  # smooth colourful images plus noise, as bytes; the same tables for all three paths
        low = rng.normal(size=(B, hs // 16 + 1, hs // 16 + 1, 3))
        up = np.kron(low, np.ones((1, 16, 16, 1)))[:, :hs, :hs]
        u8 = np.clip(128 + 60 * up + 12 * rng.normal(size=(B, hs, hs, 3)), 0, 255).astype(np.uint8)
        aug = MultiCrop.dino_default(seed=0)
        t0 = time.perf_counter()
        for _ in range(5):
            tables = aug.draw(B, hs, hs)
        data[hs] = (u8, tables, (time.perf_counter() - t0) / 5 * 1e3)
    say(f"# SSL crops of one batch: B={B}, 2 x 256 + 8 x 96 crops per image ({10 * B} crops, {B * (2 * 3 * 256 * 256 + 8 * 3 * 96 * 96) * 4 / 1e6:.1f} MB of fp32)")
    for hs in a.sizes:
        say(f"source {hs}x{hs}: MultiCrop.draw (host, numpy) {data[hs][2]:.2f} ms per batch")

    if not a.no_pil:  # before the GPU is initialised: the workers never see it
        import multiprocessing as mp
        workers = max(1, min(a.workers, 16, os.cpu_count() or 1))
        with mp.get_context("spawn").Pool(workers) as pool:
            for hs in a.sizes:
                u8, tables, _ = data[hs]
                pil_batch(pool, u8, tables, sizes_of(tables))  # warm-up: imports in the workers
                ts = []
                for _ in range(a.pil_batches):
                    t0 = time.perf_counter()
                    pil_batch(pool, u8, tables, sizes_of(tables))
                    ts.append((time.perf_counter() - t0) * 1e3)
                m = statistics.median(ts)
                say(f"source {hs}x{hs}: PIL pipeline, {workers} worker processes: median {m:9.1f} ms per batch  min {min(ts):9.1f}  max {max(ts):9.1f}"
                    f"  = {10 * B / m * 1e3:8.0f} crops/s = {m * workers:9.1f} core-ms per batch  (host synchronisations: not applicable, host only)")
    if a.no_gpu:
        say("GPU paths: not measured (--no-gpu)")
        return finish()

    import torch
    if not torch.cuda.is_available():
        sys.exit("augment_bench: the fused and torch paths need the GPU (no CPU timing)")
    from vtp_amd import ops
    dev = "cuda"
    say(f"# device={torch.cuda.get_device_name(0)}")
    mean, std = torch.tensor(MEAN, device=dev).view(3, 1, 1), torch.tensor(STD, device=dev).view(3, 1, 1)

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

    for hs in a.sizes:
        u8, tables, _ = data[hs]
        sizes = sizes_of(tables)
        aug = MultiCrop.dino_default(seed=0)
        uh = torch.from_numpy(u8)
        ud = uh.to(dev)
        dtab = [torch.from_numpy(t).to(dev) for t in tables]
        outs = [torch.empty(len(t), 3, S, S, device=dev) for t, S in zip(tables, sizes)]
        scr = [torch.empty(ops.augment_scratch_size(len(t), S), device=dev) for t, S in zip(tables, sizes)]
        kernels = lambda: [ops.augment_crops(ud, dt, o, MEAN, STD, s) for dt, o, s in zip(dtab, outs, scr)]
        fused_dev = lambda: aug.apply(ud, tables)
        fused_host = lambda: aug.apply(uh, tables)
        torch_fn = lambda: torch_batch(ud, tables, sizes, mean, std)
        for fn in (kernels, fused_dev, fused_host, torch_fn):  # warm-up: code objects, workspaces, library algorithm choice
            fn()
            fn()
        torch.cuda.synchronize()
        got, want = fused_dev(), torch_fn()
        diff = max(float((g - w).abs().max()) for g, w in zip(got, want))
        say(f"source {hs}x{hs}: fused against the torch chain on the same tables: max |diff| {diff:.2e} (normalised units; pixels at the solarize threshold may flip)")
        say(f"source {hs}x{hs}: host synchronisations per batch: fused (device input) {count_syncs(fused_dev)}, fused (host input) {count_syncs(fused_host)}, "
            f"torch chain {count_syncs(torch_fn)}")
        res = {"kernels alone (4 launches)": [], "MultiCrop.apply, bytes on the device": [], "MultiCrop.apply, bytes on the host": [], "torch chain": []}
        for _ in range(a.rounds):
            res["kernels alone (4 launches)"].append(events(kernels, a.steps))
            res["MultiCrop.apply, bytes on the device"].append(events(fused_dev, a.steps))
            res["MultiCrop.apply, bytes on the host"].append(events(fused_host, a.steps))
            res["torch chain"].append(events(torch_fn, max(1, a.steps // 5)))
        for k, ts in res.items():
            say(f"source {hs}x{hs}: {k:40s} {stats(ts)}  per batch")
        mk = statistics.median(res["kernels alone (4 launches)"])
        moved = B * hs * hs * 3 + 3 * sum(o.numel() * 4 for o in outs)  # bytes read once, crops written, re-read and written
        say(f"source {hs}x{hs}: kernels alone = {moved / mk / 1e6:.3f} TB/s of at most {moved / 1e6:.1f} MB moved; "
            f"{mk / 44000 * 100:.3f} % of a 44 ms training step; torch / fused = {statistics.median(res['torch chain']) / mk:.0f}")
        for S, dt, o, s in zip(sizes, dtab, outs, scr):
            ts = [events(lambda: ops.augment_crops(ud, dt, o, MEAN, STD, s), a.steps) for _ in range(a.rounds)]
            say(f"source {hs}x{hs}:   vtp_augment_crops S={S:3d} N={len(dt):3d} (2 launches) {stats(ts)}")
    finish()


if __name__ == "__main__":
    main()
