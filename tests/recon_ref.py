"""Helper of the reconstruction-evaluation tests (not a test): a plain torch restatement of what tools/test_reconstruction_hf.py
does per batch around its model calls (:360-409) -- transform_rev and clamp, the LPIPS inputs, the byte images, PSNR per image
(oracle.tools_oracle.calculate_psnr / denormalize, pinned to the real tool) and SSIM written THE LIBRARY'S WAY
(StructuralSimilarityIndexMeasure(data_range=1.0): reflect pad, grouped 2-D convolution over the five-fold concatenation, crop) --
in fp32 or fp64, and the tool's aggregation (:428-430).  tests/test_recon_eval_host.py checks it against the valid-convolution
form and closed forms; tests/test_recon_eval_gpu.py checks the kernels against it."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import tools_oracle as T

F32, F64 = torch.float32, torch.float64
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # IMAGENET_DEFAULT_MEAN / STD
C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2              # k1 = 0.01, k2 = 0.03, data_range = 1.0


def gaussian_kernel(dtype=F64, size=11, sigma=1.5):
    """[3, 1, 11, 11]: the outer product of the normalised 1-D Gaussian, one copy per channel"""
    dist = torch.arange((1 - size) / 2, (1 + size) / 2, 1, dtype=dtype)
    g = torch.exp(-((dist / sigma) ** 2) / 2)
    g = (g / g.sum()).unsqueeze(0)
    return (g.T @ g).expand(3, 1, size, size).contiguous()


def _ssim_map(maps, B):
    mu_p, mu_t, e_pp, e_tt, e_pt = maps.split(B)
    mu_pp, mu_tt, mu_pt = mu_p.pow(2), mu_t.pow(2), mu_p * mu_t
    var_p = torch.clamp(e_pp - mu_pp, min=0.0)
    var_t = torch.clamp(e_tt - mu_tt, min=0.0)
    cov = e_pt - mu_pt
    return ((2 * mu_pt + C1) * (2 * cov + C2)) / ((mu_pp + mu_tt + C1) * (var_p + var_t + C2))


def ssim_library(p, t):
    """per-image SSIM of p, t [B, 3, H, W] in [0, 1], in their dtype: reflect pad by 5, grouped convolution, crop 5"""
    B = p.shape[0]
    k = gaussian_kernel(p.dtype)
    pp, tp = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    maps = F.conv2d(torch.cat((pp, tp, pp * pp, tp * tp, pp * tp)), k, groups=3)
    return _ssim_map(maps, B)[..., 5:-5, 5:-5].reshape(B, -1).mean(-1)


def ssim_valid(p, t):
    """the same as the valid convolution of the unpadded images: (H - 10) x (W - 10) window positions"""
    B = p.shape[0]
    maps = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), gaussian_kernel(p.dtype), groups=3)
    return _ssim_map(maps, B).reshape(B, -1).mean(-1)


def denorm(x, dtype=F32):
    """transform_rev then torch.clamp(.., 0, 1) (:371-376), in dtype (the constants are the tool's fp32 ones)"""
    return torch.clamp(T.denormalize(x.detach().cpu().to(dtype)), 0, 1)


def batch(images, recon, dtype=F64):
    """the tool's per-batch numbers: 'psnr' [B] (f64 tensor, inf for an identical pair), 'ssim' [B], 'sse' [B]"""
    o, r = denorm(images, dtype), denorm(recon, dtype)
    psnr = torch.tensor([T.calculate_psnr(o[i] * 255.0, r[i] * 255.0) for i in range(o.shape[0])], dtype=F64)
    sse = ((o * 255.0 - r * 255.0) ** 2).flatten(1).sum(1).to(F64)
    return {"psnr": psnr, "ssim": ssim_library(o, r).to(F64), "sse": sse}


def bytes_and_lpips_inputs(x):
    """(uint8 [B, H, W, 3], f32 [B, 3, H, W]) of one tensor, the tool's fp32 expressions on the CPU (:381-382, :401-402)"""
    d = denorm(x, F32)
    u8 = torch.from_numpy((d.permute(0, 2, 3, 1).cpu().numpy() * 255.0).astype(np.uint8))
    return u8, d * 2.0 - 1.0


def aggregate_tool(batches, lpips_batches=None):
    """the tool's result (:386, :392, :395-397, :428-430) from a list of batch() dicts: PSNR averaged over images, SSIM (and LPIPS,
    a list of [B] tensors) over the batches' means; plus the per-image means"""
    psnr = torch.cat([b["psnr"] for b in batches])
    ssim = torch.cat([b["ssim"] for b in batches])
    out = {"psnr": float(np.mean(psnr.numpy())), "ssim": float(np.mean([float(b["ssim"].mean()) for b in batches])),
           "num_samples": int(psnr.numel()), "ssim_per_image": float(ssim.mean()), "lpips": None, "lpips_per_image": None}
    if lpips_batches is not None:
        out["lpips"] = float(np.mean([float(v.double().mean()) for v in lpips_batches]))
        out["lpips_per_image"] = float(torch.cat([v.double().flatten() for v in lpips_batches]).mean())
    return out


def normalise(d):
    """images in [0, 1] (any values) -> the ImageNet-normalised fp32 tensor the tool's loader produces"""
    m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    return ((d.float() - m) / s).contiguous()


def smooth_pair(B, H, W, seed, psnr_db=None):
    """(images, recon), normalised f32 [B, 3, H, W]: smooth random images 0.5 + 0.255 z (z about unit normal: about 5 % of the
    de-normalised values fall outside [0, 1] and are clamped) and the image plus white noise whose amplitude gives about
    psnr_db[b] dB (default: spread evenly from 12 to 54 dB over the batch)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, 3, max(H // 8, 2), max(W // 8, 2), generator=g)
    z = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    z = z / z.std()
    d = 0.5 + 0.255 * z
    if psnr_db is None:
        psnr_db = [12.0 + (54.0 - 12.0) * (i + 0.5) / B for i in range(B)]
    amp = torch.tensor([10.0 ** (-p / 20.0) for p in psnr_db]).view(B, 1, 1, 1)
    return normalise(d), normalise(d + amp * torch.randn(B, 3, H, W, generator=g))
