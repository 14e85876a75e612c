"""Reconstruction evaluation (reference: tools/test_reconstruction_hf.py) on the project's kernels: what the tool does per batch
around its model calls (:360-409) -- transform_rev and clamp of both tensors, the LPIPS inputs, SSIM, PSNR per image, the byte
images of the two PNG folders -- is ONE launch over the two image tensors plus one small launch that turns the per-tile partials
into per-image PSNR / SSIM and adds to running sums on the device (csrc/recon_eval.hip).  No .item(), no torchmetrics, and no
host synchronisation before results() is asked for.

    ev = ReconEval(model, lpips=lp)                    # lp: a vtp_amd.LPIPS or None; model None for cached pairs (update_pair)
    for batch_idx, (images, _) in enumerate(loader):
        out = ev.update(images.cuda(), want_u8=True)   # latents -> decode -> the two launches (+ LPIPS)
        save_pngs(out, ref_dir, rec_dir, png_index(batch_idx, batch_size, world, rank, 0), total_samples)
    res = ev.results()                                 # {'psnr', 'ssim', 'lpips', 'num_samples', ...} as the tool prints them

PSNR is averaged over images, SSIM and LPIPS over the batches' means, as the tool does (:386, :392, :395-397, :428-430): a short
last batch weighs like a full one there.  The per-image means are returned as well.  SSIM is the definition of torchmetrics'
StructuralSimilarityIndexMeasure(data_range=1.0) (csrc/recon_eval.hip).  rFID: with fid=vtp_amd.FID(...) every
update also hands the byte images of the two PNG folders to the FID object and results() gains 'fid' (vtp_amd/fid.py); without
one nothing about it is computed.  There is no CPU path: tensors on the CPU raise."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import torch

from . import ops
from .banks import Group, eval_device
from .tokenizer import NORMALIZE_IMAGENET

ACC_SLOTS = 8  # the accumulator block of vtp_recon_finalize (include/vtp_hip.h)


class ReconBatch(NamedTuple):
    psnr: torch.Tensor               # f32 [B], dB; +inf for an identical pair
    ssim: torch.Tensor               # f32 [B]
    sse: torch.Tensor                # f64 [B]: sum over 3 H W of (o * 255 - r * 255) ** 2
    lpips: Optional[torch.Tensor]    # f32 [B], or None without an LPIPS
    ref_u8: Optional[torch.Tensor]   # uint8 [B, H, W, 3], or None without want_u8
    rec_u8: Optional[torch.Tensor]


def png_index(batch_idx: int, batch_size: int, world: int, rank: int, i: int) -> int:
    """global_idx of image i of a rank's batch (:405)"""
    return batch_idx * batch_size * world + rank * batch_size + i


def save_pngs(out: ReconBatch, ref_dir: str, rec_dir: str, first_index: int, limit: Optional[int] = None) -> int:
    """writes ref_%06d.png / rec_%06d.png of a batch (:404-409), numbered from first_index = png_index(.., i = 0); images whose
    index reaches `limit` (the tool's total_samples) are not written.  One copy of each byte tensor to the host.  Returns the
    number of pairs written."""
    if out.ref_u8 is None or out.rec_u8 is None:
        raise ValueError("save_pngs needs the byte images: update(..., want_u8=True)")
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("save_pngs needs PIL (Pillow) to write PNG files; the byte images are out.ref_u8 / out.rec_u8") from e
    ref, rec = out.ref_u8.cpu().numpy(), out.rec_u8.cpu().numpy()
    n = 0
    for i in range(ref.shape[0]):
        idx = first_index + i
        if limit is not None and idx >= limit:
            break
        Image.fromarray(ref[i]).save(os.path.join(ref_dir, f"ref_{idx:06d}.png"))
        Image.fromarray(rec[i]).save(os.path.join(rec_dir, f"rec_{idx:06d}.png"))
        n += 1
    return n


def aggregate(acc, with_lpips: bool) -> dict:
    """the tool's result from the accumulator block (a sequence of ACC_SLOTS numbers): PSNR over images, SSIM and LPIPS over
    batch means (:428-430); an identical pair makes the PSNR mean inf, as np.mean of the tool's list does"""
    a = [float(v) for v in acc]
    n, batches = a[1], a[5]
    if n <= 0 or batches <= 0:
        raise RuntimeError("results(): nothing evaluated yet")
    return {"psnr": a[0] / n, "ssim": a[4] / batches, "lpips": a[6] / batches if with_lpips else None, "num_samples": int(n),
            "ssim_per_image": a[3] / n, "lpips_per_image": a[7] / n if with_lpips else None, "identical_images": int(a[2])}


class ReconEval:
    """model: a vtp_amd.VTPModel (None when reconstructions are given: update_pair).  lpips: a vtp_amd.LPIPS or None.  group: a
    process group whose ranks each evaluate their own batches; results() sums the accumulator block over it (the tool's mean of
    per-rank means when every rank saw as many images and batches, which its DistributedSampler arranges).  fid: a vtp_amd.FID or
    None; with one, every update feeds it the byte images and results() has 'fid'."""

    def __init__(self, model, lpips=None, group=None, device=None, fid=None):
        self.device = eval_device("ReconEval", model, device)
        self.model, self.lpips, self.group, self.fid = model, lpips, group, fid
        self._group = Group(group)
        mean, std = NORMALIZE_IMAGENET["mean"], NORMALIZE_IMAGENET["std"]
        self.sub = [-m / s for m, s in zip(mean, std)]  # transform_rev (:265-268)
        self.div = [1 / s for s in std]
        self._acc = torch.zeros(ACC_SLOTS, device=self.device, dtype=torch.float64)
        self._ws = {}

    def _workspace(self, B: int, H: int, W: int) -> dict:
        ws = self._ws.get((B, H, W))
        if ws is None:
            if W % 4 or H < 11 or W < 11:
                raise ValueError(f"images must be at least 11 x 11 (one SSIM window) with W a multiple of 4, got {H} x {W}")
            ws = {"scratch": torch.empty(ops.recon_scratch_size(B, H, W), device=self.device, dtype=torch.float64)}
            if self.lpips is not None:
                ws["ref_lp"] = torch.empty(B, 3, H, W, device=self.device, dtype=torch.float32)
                ws["rec_lp"] = torch.empty_like(ws["ref_lp"])
            self._ws[(B, H, W)] = ws
        return ws

    def update(self, images: torch.Tensor, want_u8: bool = False) -> ReconBatch:
        """the loop body of the tool (:362-409) for one batch of normalised images f32 [B, 3, H, W] on the device"""
        if self.model is None:
            raise RuntimeError("ReconEval was built without a model: use update_pair")
        if not images.is_cuda:
            raise ValueError("images must live on the MI355X (got a CPU tensor): there is no CPU path")
        with torch.no_grad():
            images = images.to(torch.float32)
            recon = self.model.get_latents_decoded_images(self.model.get_reconstruction_latents(images))
        return self.update_pair(images, recon, want_u8=want_u8)

    def update_pair(self, images: torch.Tensor, recon: torch.Tensor, want_u8: bool = False) -> ReconBatch:
        """adds one batch of (images, reconstruction), both normalised f32 [B, 3, H, W], to the evaluation: device only"""
        if not images.is_cuda or not recon.is_cuda:
            raise ValueError("images and recon must live on the MI355X (got a CPU tensor): there is no CPU path")
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1 or recon.shape != images.shape:
            raise ValueError(f"images and recon must both be [B, 3, H, W], got {tuple(images.shape)} / {tuple(recon.shape)}")
        B, _, H, W = images.shape
        ws = self._workspace(B, H, W)
        x = images.detach().to(torch.float32).contiguous()
        r = recon.detach().to(torch.float32).contiguous()
        dev = self.device
        psnr = torch.empty(B, device=dev, dtype=torch.float32)
        ssim = torch.empty(B, device=dev, dtype=torch.float32)
        sse = torch.empty(B, device=dev, dtype=torch.float64)
        need_u8 = want_u8 or self.fid is not None
        ref_u8 = torch.empty(B, H, W, 3, device=dev, dtype=torch.uint8) if need_u8 else None
        rec_u8 = torch.empty(B, H, W, 3, device=dev, dtype=torch.uint8) if need_u8 else None
        ops.recon_metrics(x, r, self.sub, self.div, ws["scratch"], ref_u8, rec_u8, ws.get("ref_lp"), ws.get("rec_lp"))
        lp = None
        if self.lpips is not None:
            lp = self.lpips(ws["ref_lp"], ws["rec_lp"]).reshape(B).to(torch.float32).contiguous()  # lpips_metric(orig, recon) (:383)
        ops.recon_finalize(ws["scratch"], B, H, W, psnr, ssim, self._acc, sse, lp)
        if self.fid is not None:
            self.fid.update(ref_u8, rec_u8)
        return ReconBatch(psnr, ssim, sse, lp, ref_u8 if want_u8 else None, rec_u8 if want_u8 else None)

    def accumulators(self) -> torch.Tensor:
        """the accumulator block, summed over the process group with one all-reduce; one copy to the host (CPU f64 [8])"""
        return self._group.summed(self._acc).cpu()

    def results(self) -> dict:
        res = aggregate(self.accumulators().tolist(), self.lpips is not None)
        if self.fid is not None:
            res["fid"] = self.fid.result()
        return res

    def reset(self) -> None:
        self._acc.zero_()
        if self.fid is not None:
            self.fid.reset()
