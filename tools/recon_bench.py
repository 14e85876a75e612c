#!/usr/bin/env python3
"""Reconstruction-evaluation step at the reference tool's shape (B = 32 images of 256 x 256), images and reconstructions given:
vtp_amd.ReconEval.update_pair (two launches, no host synchronisation) against the torch formulation a user of the tool runs today
(tools/test_reconstruction_hf.py:371-402: two Normalize + clamp passes, the two LPIPS inputs, SSIM as the library forms it --
reflect pad, five-fold concatenation, grouped 11 x 11 convolution, crop -- with its .item(), one .item() per image for PSNR, and the
two permute / .cpu() / * 255 / astype(uint8) chains), plus the two kernels alone.  The LPIPS network is the same kernels on either
side and is left out of both.

    python tools/recon_bench.py [--steps 10] [--rounds 5] [--out profiles/recon_eval.log]

Both loops get their inputs ready-made and are timed in alternating windows of `steps` batches, each closed by reading the result
on the host (which is when the fused path synchronises at all); the figure of record is the median window.  Two variants: metrics
only, and with the byte images of the PNG folders brought to the host (PNG encoding itself is host work on either side)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gaussian_kernel(device):
    dist = torch.arange(-5.0, 6.0, 1.0, device=device)
    g = torch.exp(-((dist / 1.5) ** 2) / 2)
    g = (g / g.sum()).unsqueeze(0)
    return (g.T @ g).expand(3, 1, 11, 11).contiguous()


def torch_ssim(p, t, kernel):
    """StructuralSimilarityIndexMeasure(data_range=1.0) as the library forms it, fp32; the batch mean, on the device"""
    B = p.shape[0]
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    p, t = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    mu_p, mu_t, e_pp, e_tt, e_pt = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), kernel, groups=3).split(B)
    mu_pp, mu_tt, mu_pt = mu_p.pow(2), mu_t.pow(2), mu_p * mu_t
    var_p, var_t, cov = torch.clamp(e_pp - mu_pp, min=0.0), torch.clamp(e_tt - mu_tt, min=0.0), e_pt - mu_pt
    s = ((2 * mu_pt + c1) * (2 * cov + c2)) / ((mu_pp + mu_tt + c1) * (var_p + var_t + c2))
    return s[..., 5:-5, 5:-5].reshape(B, -1).mean(-1).mean()


def torch_batch(images, recon, sub, div, kernel, want_u8, calculate_psnr):
    """the tool's loop body without its model and LPIPS-network calls (:371-402); returns (psnr list, ssim float, byte images)"""
    recon_denorm = torch.clamp((recon - sub) / div, 0, 1)
    orig_denorm = torch.clamp((images - sub) / div, 0, 1)
    orig_lpips, recon_lpips = orig_denorm * 2.0 - 1.0, recon_denorm * 2.0 - 1.0  # the inputs the LPIPS call would read
    ssim = torch_ssim(orig_denorm, recon_denorm, kernel).item()
    psnr = [calculate_psnr(orig_denorm[i] * 255.0, recon_denorm[i] * 255.0) for i in range(images.size(0))]
    u8 = None
    if want_u8:
        u8 = ((orig_denorm.permute(0, 2, 3, 1).cpu().numpy() * 255.0).astype(np.uint8),
              (recon_denorm.permute(0, 2, 3, 1).cpu().numpy() * 255.0).astype(np.uint8))
    return psnr, ssim, u8, (orig_lpips, recon_lpips)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("recon_bench: needs the GPU (no CPU timing)")
    from oracle.tools_oracle import calculate_psnr  # the tool's calculate_psnr as the oracle restates it
    from vtp_amd import ops
    from vtp_amd.recon_eval import ReconEval
    dev = "cuda"
    B, H, W = a.batch, a.size, a.size
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# reconstruction-eval step: B={B} {H}x{W} device={torch.cuda.get_device_name(0)}")
    torch.manual_seed(0)
    ev = ReconEval(None)
    sub = torch.tensor(ev.sub, device=dev).view(1, 3, 1, 1)
    div = torch.tensor(ev.div, device=dev).view(1, 3, 1, 1)
    d = 0.5 + 0.255 * F.interpolate(torch.randn(B, 3, H // 8, W // 8, device=dev), size=(H, W), mode="bicubic")
    images = (d * div + sub).contiguous()  # (d - mean) / std: smooth images in [0, 1], about 5 % of the values clamped
    recon = ((d + 0.02 * torch.randn_like(d)) * div + sub).contiguous()  # about 34 dB
    kernel = gaussian_kernel(dev)

    for want_u8 in (False, True):
        tag = "metrics + byte images on the host" if want_u8 else "metrics only"

        def torch_window():
            psnr, ssim = [], []
            for _ in range(a.steps):
                p, s, _, _ = torch_batch(images, recon, sub, div, kernel, want_u8, calculate_psnr)
                psnr += p
                ssim.append(s)
            return float(np.mean(psnr)), float(np.mean(ssim))

        def ours_window():
            ev.reset()
            for _ in range(a.steps):
                out = ev.update_pair(images, recon, want_u8=want_u8)
                if want_u8:
                    out.ref_u8.cpu().numpy(), out.rec_u8.cpu().numpy()
            res = ev.results()
            return res["psnr"], res["ssim"]

        def window(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps * 1e6, res

        for fn in (ours_window, torch_window):  # warm-up: code objects, library algorithm choice
            fn()
        t_ours, t_torch = [], []
        for r in range(a.rounds):
            to, ro = window(ours_window)
            tt, rt = window(torch_window)
            t_ours.append(to)
            t_torch.append(tt)
            say(f"{tag} round {r}: fused {to:9.1f} us/batch (PSNR {ro[0]:.4f} SSIM {ro[1]:.6f})   torch {tt:9.1f} us/batch (PSNR {rt[0]:.4f} SSIM {rt[1]:.6f})")
        mo, mt = statistics.median(t_ours), statistics.median(t_torch)
        say(f"{tag}: update_pair median {mo:9.1f} us  min {min(t_ours):9.1f}  max {max(t_ours):9.1f}")
        say(f"{tag}: torch loop  median {mt:9.1f} us  min {min(t_torch):9.1f}  max {max(t_torch):9.1f}")
        say(f"{tag}: torch / fused = {mt / mo:.2f}  (medians of {a.rounds} alternating windows of {a.steps} batches, host clock)")

    # the kernels alone (device events over `reps` back-to-back launches)
    reps = 20
    scratch = torch.empty(ops.recon_scratch_size(B, H, W), device=dev, dtype=torch.float64)
    ref_u8, rec_u8 = (torch.empty(B, H, W, 3, device=dev, dtype=torch.uint8) for _ in range(2))
    ref_lp, rec_lp = (torch.empty(B, 3, H, W, device=dev) for _ in range(2))
    psnr, ssim = torch.empty(B, device=dev), torch.empty(B, device=dev)
    acc = torch.zeros(8, device=dev, dtype=torch.float64)
    rd, wr_u8, wr_lp = 2 * B * 3 * H * W * 4, 2 * B * H * W * 3, 2 * B * 3 * H * W * 4
    for name, nbytes, call in (
            ("vtp_recon_metrics (partials only)", rd, lambda: ops.recon_metrics(images, recon, ev.sub, ev.div, scratch)),
            ("vtp_recon_metrics (+ byte images)", rd + wr_u8, lambda: ops.recon_metrics(images, recon, ev.sub, ev.div, scratch, ref_u8, rec_u8)),
            ("vtp_recon_metrics (+ bytes, LPIPS inputs)", rd + wr_u8 + wr_lp,
             lambda: ops.recon_metrics(images, recon, ev.sub, ev.div, scratch, ref_u8, rec_u8, ref_lp, rec_lp)),
            ("vtp_recon_finalize", scratch.numel() * 8, lambda: ops.recon_finalize(scratch, B, H, W, psnr, ssim, acc))):
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        say(f"  {name:44s} {us:9.1f} us  {nbytes / us / 1e6:6.3f} TB/s of the {nbytes / 1e6:.1f} MB it must move")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
