"""rFID on the gfx950 kernels (reference: _calculate_fid_manual, tools/test_reconstruction_hf.py:121-176): Inception-v3 pool
features in exact fp32, their mean and covariance accumulated in fp64 on the device, the Frechet distance on the host.

    inc = InceptionFeatures("torchvision")              # state_dict keys of torchvision.models.inception_v3
    inc.load_state_dict(torch.load("inception_v3.pth")) # the caller brings the weights (AuxLogits.*, fc.* are ignored)
    fid = FID(inc.cuda())
    ev = ReconEval(model, lpips=lp, fid=fid)            # every update feeds the byte images of the two PNG folders to `fid`
    ...
    ev.results()["fid"]

variant "torchvision" is the tool's fallback: inception_v3(transform_input=False) with fc = Identity on Resize((299, 299)) +
ToTensor of the PNGs.  variant "pytorch_fid" is that package's FIDInceptionA/C/E_1/E_2 network (average pools that leave the
padding out of the divisor, a max pool in Mixed_7c) on a bilinear resize to 299 and 2 x - 1; it is written from the published
description of those classes and is not pinned against the package.

Compute (csrc/fid.hip): activations are NHWC f32; each of the 94 convolutions is one vtp_conv2d_f32 launch with BatchNorm folded
into its weight and bias (fp64 on the host, once per weight version) and writes straight into its channel slice of the block's
concatenated output.  Every output element is one fmaf chain, so features do not depend on the batch an image came in.  There is
no CPU path and no host synchronisation in forward().  forward_taps() is the same pass plus the spatial features of sFID (one more
launch); vtp_amd/gen_eval.py builds the generation metrics on it."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import ops

F32, F64 = torch.float32, torch.float64
BN_EPS = 1e-3
FEATURE_DIM = 2048


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _inception_convs() -> List[Tuple[str, int, int, Tuple[int, int], int, Tuple[int, int]]]:
    """(name, Cin, Cout, (kh, kw), stride, (ph, pw)) of the 94 BasicConv2d of torchvision's Inception3 without AuxLogits"""
    t = []

    def add(name, cin, cout, k=1, s=1, p=0):
        t.append((name, cin, cout, _pair(k), s, _pair(p)))

    add("Conv2d_1a_3x3", 3, 32, 3, 2)
    add("Conv2d_2a_3x3", 32, 32, 3)
    add("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    add("Conv2d_3b_1x1", 64, 80)
    add("Conv2d_4a_3x3", 80, 192, 3)
    for name, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        add(f"{name}.branch1x1", cin, 64)
        add(f"{name}.branch5x5_1", cin, 48)
        add(f"{name}.branch5x5_2", 48, 64, 5, 1, 2)
        add(f"{name}.branch3x3dbl_1", cin, 64)
        add(f"{name}.branch3x3dbl_2", 64, 96, 3, 1, 1)
        add(f"{name}.branch3x3dbl_3", 96, 96, 3, 1, 1)
        add(f"{name}.branch_pool", cin, pf)
    add("Mixed_6a.branch3x3", 288, 384, 3, 2)
    add("Mixed_6a.branch3x3dbl_1", 288, 64)
    add("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    add("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(f"{name}.branch1x1", 768, 192)
        add(f"{name}.branch7x7_1", 768, c7)
        add(f"{name}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        add(f"{name}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        add(f"{name}.branch7x7dbl_1", 768, c7)
        add(f"{name}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        add(f"{name}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        add(f"{name}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        add(f"{name}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        add(f"{name}.branch_pool", 768, 192)
    add("Mixed_7a.branch3x3_1", 768, 192)
    add("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    add("Mixed_7a.branch7x7x3_1", 768, 192)
    add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    add("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for name, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(f"{name}.branch1x1", cin, 320)
        add(f"{name}.branch3x3_1", cin, 384)
        add(f"{name}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{name}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{name}.branch3x3dbl_1", cin, 448)
        add(f"{name}.branch3x3dbl_2", 448, 384, 3, 1, 1)
        add(f"{name}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{name}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{name}.branch_pool", cin, 192)
    return t


INCEPTION_CONVS = _inception_convs()
MIN_SIDE = 75  # the smallest input that leaves one pixel in front of the global pool
TAP_CONV, TAP_CHANNELS = "Mixed_6d.branch1x1", 7  # forward_taps: the spatial features of sFID


def fold_conv_bn(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """conv (no bias) + eval-mode BatchNorm as one conv with a bias, in fp64: w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(..)"""
    s = gamma.to(F64) / torch.sqrt(var.to(F64) + eps)
    return w.to(F64) * s.view(-1, 1, 1, 1), beta.to(F64) - mean.to(F64) * s


def forward_gflop(H: int = 299, W: int = 299) -> float:
    """algorithmic FLOPs of one image, 2 * MACs of the 94 convolutions: 5.7 GMAC = 11.4 GFLOP at 299 x 299"""
    pool = lambda v: (v - 3) // 2 + 1
    h, w, total, prev = H, W, 0.0, None
    for name, cin, cout, k, s, p in INCEPTION_CONVS:
        top = name.split(".")[0]
        if top != prev and prev in ("Conv2d_2b_3x3", "Conv2d_4a_3x3", "Mixed_6a", "Mixed_7a"):  # a stride-2 pool / block went before
            h, w = pool(h), pool(w)
        prev = top
        if "." not in name:
            h, w = ops.conv_out_size(h, w, k[0], k[1], s, p[0], p[1])
            ho, wo = h, w
        else:  # inside a Mixed block every stride-1 conv keeps the size, a stride-2 conv ends at the block's output size
            ho, wo = (h, w) if s == 1 else (pool(h), pool(w))
        total += 2.0 * ho * wo * k[0] * k[1] * cin * cout
    return total / 1e9


class _Holder(nn.Module):
    pass


class InceptionFeatures(nn.Module):
    def __init__(self, variant: str = "torchvision"):
        super().__init__()
        if variant not in ("torchvision", "pytorch_fid"):
            raise ValueError(f"variant must be 'torchvision' or 'pytorch_fid', got {variant!r}")
        self.variant = variant
        self._spec = {}
        for name, cin, cout, k, s, p in INCEPTION_CONVS:
            parent = self
            parts = name.split(".")
            for part in parts[:-1]:
                if not hasattr(parent, part):
                    parent.add_module(part, _Holder())
                parent = getattr(parent, part)
            blk, conv, bn = _Holder(), _Holder(), _Holder()
            conv.register_buffer("weight", torch.zeros(cout, cin, k[0], k[1]))
            bn.register_buffer("weight", torch.ones(cout))
            bn.register_buffer("bias", torch.zeros(cout))
            bn.register_buffer("running_mean", torch.zeros(cout))
            bn.register_buffer("running_var", torch.ones(cout))
            blk.conv, blk.bn = conv, bn
            parent.add_module(parts[-1], blk)
            self._spec[name] = (cin, cout, k, s, p)
        self._prepped = None
        self._w: Dict[str, torch.Tensor] = {}
        self._b: Dict[str, torch.Tensor] = {}
        self._tap_w: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------------------------------------ weights
    def _block(self, name: str) -> nn.Module:
        m = self
        for part in name.split("."):
            m = getattr(m, part)
        return m

    @torch.no_grad()
    def reset_parameters(self, seed: int = 0):
        """Seeded stand-in weights (benchmarks / tests; trained weights come through load_state_dict): Kaiming-normal convolutions,
        BatchNorm weight and running_var in U(0.5, 1.5), bias and running_mean in N(0, 0.1^2)."""
        g = torch.Generator().manual_seed(seed)
        for name, cin, cout, k, _, _ in INCEPTION_CONVS:
            blk = self._block(name)
            blk.conv.weight.copy_(torch.randn(cout, cin, k[0], k[1], generator=g) * (2.0 / (cin * k[0] * k[1])) ** 0.5)
            blk.bn.weight.copy_(0.5 + torch.rand(cout, generator=g))
            blk.bn.running_var.copy_(0.5 + torch.rand(cout, generator=g))
            blk.bn.bias.copy_(0.1 * torch.randn(cout, generator=g))
            blk.bn.running_mean.copy_(0.1 * torch.randn(cout, generator=g))
        self._prepped = None
        return self

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """torchvision's inception_v3 state dict: AuxLogits.*, fc.* and num_batches_tracked are dropped, every conv / bn key is needed"""
        sd = {k: v for k, v in state_dict.items()
              if not (k.startswith(("AuxLogits.", "fc.")) or k.endswith("num_batches_tracked"))}
        self._prepped = None
        return super().load_state_dict(sd, strict=strict, **kw)

    def _apply(self, fn, *args, **kw):
        # .to() / .cuda() / .cpu() replace the buffers by fresh tensors whose version counters start again at 0: the counters alone
        # would take a module that was moved, reloaded and moved back for the one whose weights are already folded
        self._prepped = None
        return super()._apply(fn, *args, **kw)

    def _version(self) -> int:
        return sum(int(b._version) for b in self.buffers())

    def _prep(self):
        """fold BatchNorm in fp64 on the host and upload [Cout, kh, kw, Cin] f32 weights and f32 biases, once per weight version"""
        dev = self.Conv2d_1a_3x3.conv.weight.device
        ver = (self._version(), str(dev))
        if self._prepped == ver:
            return
        if dev.type != "cuda":
            raise RuntimeError("vtp_amd.InceptionFeatures runs on the MI355X kernels only: move the module to a cuda device (no CPU path)")
        for name, *_ in INCEPTION_CONVS:
            blk = self._block(name)
            w, b = fold_conv_bn(blk.conv.weight.detach().cpu(), blk.bn.weight.detach().cpu(), blk.bn.bias.detach().cpu(),
                                blk.bn.running_mean.detach().cpu(), blk.bn.running_var.detach().cpu())
            self._w[name] = w.permute(0, 2, 3, 1).contiguous().to(F32).to(dev)
            self._b[name] = b.to(F32).to(dev)
        # the sFID tap (forward_taps): the first TAP_CHANNELS filters of Mixed_6d.branch1x1 as they are, no BatchNorm folded in
        w = self._block(TAP_CONV).conv.weight.detach()[:TAP_CHANNELS]
        self._tap_w = w.cpu().permute(0, 2, 3, 1).contiguous().to(F32).to(dev)
        self._prepped = ver

    # ------------------------------------------------------------------------------------------------ compute
    def _conv(self, name: str, x: torch.Tensor, out: Optional[torch.Tensor] = None, c0: int = 0) -> torch.Tensor:
        _, cout, k, s, p = self._spec[name]
        if out is None:
            ho, wo = ops.conv_out_size(x.shape[1], x.shape[2], k[0], k[1], s, p[0], p[1])
            out = torch.empty(x.shape[0], ho, wo, cout, device=x.device, dtype=F32)
        ops.conv2d_f32(x, self._w[name], self._b[name], out, stride=s, pad=p, relu=True, c0=c0)
        return out

    @staticmethod
    def _pool(x: torch.Tensor, stride: int, mode: int, out: Optional[torch.Tensor] = None, c0: int = 0) -> torch.Tensor:
        if out is None:
            B, H, W, C = x.shape
            ho, wo = (H, W) if stride == 1 else ((H - 3) // 2 + 1, (W - 3) // 2 + 1)
            out = torch.empty(B, ho, wo, C, device=x.device, dtype=F32)
        ops.pool3x3_f32(x, out, stride, mode, c0)
        return out

    def _new(self, x: torch.Tensor, C: int, stride: int = 1) -> torch.Tensor:
        B, H, W, _ = x.shape
        if stride == 2:
            H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        return torch.empty(B, H, W, C, device=x.device, dtype=F32)

    def _block_a(self, n: str, x, pf: int, avg: int):
        y = self._new(x, 224 + pf)
        self._conv(f"{n}.branch1x1", x, y, 0)
        self._conv(f"{n}.branch5x5_2", self._conv(f"{n}.branch5x5_1", x), y, 64)
        t = self._conv(f"{n}.branch3x3dbl_2", self._conv(f"{n}.branch3x3dbl_1", x))
        self._conv(f"{n}.branch3x3dbl_3", t, y, 128)
        self._conv(f"{n}.branch_pool", self._pool(x, 1, avg), y, 224)
        return y

    def _block_b(self, n: str, x):
        y = self._new(x, 768, 2)
        self._conv(f"{n}.branch3x3", x, y, 0)
        t = self._conv(f"{n}.branch3x3dbl_2", self._conv(f"{n}.branch3x3dbl_1", x))
        self._conv(f"{n}.branch3x3dbl_3", t, y, 384)
        self._pool(x, 2, ops.POOL_MAX, y, 480)
        return y

    def _block_c(self, n: str, x, avg: int):
        y = self._new(x, 768)
        self._conv(f"{n}.branch1x1", x, y, 0)
        t = self._conv(f"{n}.branch7x7_2", self._conv(f"{n}.branch7x7_1", x))
        self._conv(f"{n}.branch7x7_3", t, y, 192)
        t = self._conv(f"{n}.branch7x7dbl_1", x)
        for i in (2, 3, 4):
            t = self._conv(f"{n}.branch7x7dbl_{i}", t)
        self._conv(f"{n}.branch7x7dbl_5", t, y, 384)
        self._conv(f"{n}.branch_pool", self._pool(x, 1, avg), y, 576)
        return y

    def _block_d(self, n: str, x):
        y = self._new(x, 1280, 2)
        self._conv(f"{n}.branch3x3_2", self._conv(f"{n}.branch3x3_1", x), y, 0)
        t = self._conv(f"{n}.branch7x7x3_1", x)
        for i in (2, 3):
            t = self._conv(f"{n}.branch7x7x3_{i}", t)
        self._conv(f"{n}.branch7x7x3_4", t, y, 320)
        self._pool(x, 2, ops.POOL_MAX, y, 512)
        return y

    def _block_e(self, n: str, x, pool_mode: int):
        y = self._new(x, 2048)
        self._conv(f"{n}.branch1x1", x, y, 0)
        t = self._conv(f"{n}.branch3x3_1", x)
        self._conv(f"{n}.branch3x3_2a", t, y, 320)
        self._conv(f"{n}.branch3x3_2b", t, y, 704)
        t = self._conv(f"{n}.branch3x3dbl_2", self._conv(f"{n}.branch3x3dbl_1", x))
        self._conv(f"{n}.branch3x3dbl_3a", t, y, 1088)
        self._conv(f"{n}.branch3x3dbl_3b", t, y, 1472)
        self._conv(f"{n}.branch_pool", self._pool(x, 1, pool_mode), y, 1856)
        return y

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x f32 [B, 3, H, W] in [0, 1] on the device -> the 2048 pool features f32 [B, 2048]"""
        return self._run(x, False)[0]

    @torch.no_grad()
    def forward_taps(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """the pass of forward() with the sFID tap: (pool f32 [B, 2048], the bits forward() returns; spatial f32 [B, h, w, 7]).
        spatial is what the ADM evaluation suite names mixed_6/conv:0[..., :7]: the raw output (no BatchNorm, no ReLU) of the first 7
        filters of Mixed_6d.branch1x1 on the input of Mixed_6d, NHWC -- 17 x 17 x 7 = 2023 values per image at 299 x 299, flattened
        in that order.  One more vtp_conv2d_f32 launch; the layout follows the published graph names and is not pinned against
        that program."""
        return self._run(x, True)

    def _run(self, x: torch.Tensor, taps: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        if not x.is_cuda:
            raise ValueError("x must live on the MI355X (got a CPU tensor): there is no CPU path")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1:
            raise ValueError(f"x must be [B, 3, H, W], got {tuple(x.shape)}")
        self._prep()
        x = x.detach().to(F32).contiguous()
        B, _, H, W = x.shape
        fidv = self.variant == "pytorch_fid"
        if fidv:
            a = torch.empty(B, 299, 299, 3, device=x.device, dtype=F32)
            ops.resize_bilinear_nhwc(x, a, 2.0, -1.0)
        else:
            if H < MIN_SIDE or W < MIN_SIDE:
                raise ValueError(f"the input must be at least {MIN_SIDE} x {MIN_SIDE}, got {H} x {W}")
            a = torch.empty(B, H, W, 3, device=x.device, dtype=F32)
            ops.resize_bilinear_nhwc(x, a, 1.0, 0.0)
        avg = ops.POOL_AVG_INSIDE if fidv else ops.POOL_AVG
        a = self._conv("Conv2d_1a_3x3", a)
        a = self._conv("Conv2d_2a_3x3", a)
        a = self._conv("Conv2d_2b_3x3", a)
        a = self._pool(a, 2, ops.POOL_MAX)
        a = self._conv("Conv2d_3b_1x1", a)
        a = self._conv("Conv2d_4a_3x3", a)
        a = self._pool(a, 2, ops.POOL_MAX)
        a = self._block_a("Mixed_5b", a, 32, avg)
        a = self._block_a("Mixed_5c", a, 64, avg)
        a = self._block_a("Mixed_5d", a, 64, avg)
        a = self._block_b("Mixed_6a", a)
        spatial = None
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            if taps and n == TAP_CONV.split(".")[0]:
                spatial = torch.empty(B, a.shape[1], a.shape[2], TAP_CHANNELS, device=x.device, dtype=F32)
                ops.conv2d_f32(a, self._tap_w, None, spatial, relu=False)
            a = self._block_c(n, a, avg)
        a = self._block_d("Mixed_7a", a)
        a = self._block_e("Mixed_7b", a, avg)
        a = self._block_e("Mixed_7c", a, ops.POOL_MAX if fidv else ops.POOL_AVG)
        out = torch.empty(B, FEATURE_DIM, device=x.device, dtype=F32)
        ops.global_avgpool_f32(a, out)
        return out, spatial


# ---------------------------------------------------------------------------------------------------------------------- statistics
class FrechetStats:
    """running n, sum x and sum x x^T of feature rows, fp64 on the device (vtp_fid_accum: one launch per update, rows added in
    order by the one thread that owns an element -- any split of the rows over updates gives the same bits)"""

    def __init__(self, D: int = FEATURE_DIM, device=None, group=None):
        if not torch.cuda.is_available():
            raise RuntimeError("vtp_amd.FrechetStats runs on the MI355X kernels only (no CPU path)")
        self.D, self.group = int(D), group
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("vtp_amd.FrechetStats runs on the MI355X kernels only: the device must be cuda (no CPU path)")
        self._buf = torch.zeros(1 + self.D + self.D * self.D, device=self.device, dtype=F64)  # [n | sum | outer]
        self.n = 0

    @property
    def sum(self) -> torch.Tensor:
        return self._buf[1:1 + self.D]

    @property
    def outer(self) -> torch.Tensor:
        return self._buf[1 + self.D:].view(self.D, self.D)

    def update(self, feats: torch.Tensor) -> None:
        if not feats.is_cuda:
            raise ValueError("feats must live on the MI355X (got a CPU tensor): there is no CPU path")
        if feats.dim() != 2 or feats.shape[1] != self.D or feats.shape[0] < 1:
            raise ValueError(f"feats must be [n >= 1, {self.D}], got {tuple(feats.shape)}")
        f = feats.detach().to(F32)
        if f.stride(1) != 1:
            f = f.contiguous()
        ops.fid_accum(f, self.sum, self.outer)
        self.n += int(f.shape[0])

    def _gathered(self) -> torch.Tensor:
        """[n | sum | outer] summed over the group (one all-reduce), on the host (one copy)"""
        t = self._buf
        if self.group is not None:
            import torch.distributed as dist
            t = t.clone()
            t[0] = self.n
            if dist.get_world_size(self.group) > 1:
                dist.all_reduce(t, group=self.group)
            return t.cpu()
        t = t.cpu()
        t[0] = self.n
        return t

    def mean_cov(self) -> Tuple[np.ndarray, np.ndarray]:
        """(act.mean(0), np.cov(act, rowvar=False)) of every row seen, as fp64 numpy arrays"""
        t = self._gathered().numpy()
        n, D = int(round(float(t[0]))), self.D
        if n < 2:
            raise RuntimeError(f"mean_cov(): a covariance needs at least two rows, got {n}")
        mu = t[1:1 + D] / n
        sigma = (t[1 + D:].reshape(D, D) - n * np.outer(mu, mu)) / (n - 1)
        return mu, sigma

    def reset(self) -> None:
        self._buf.zero_()
        self.n = 0

    def state_dict(self) -> dict:
        return {"n": self.n, "sum": self.sum.clone(), "outer": self.outer.clone()}

    def load_state_dict(self, sd: dict) -> None:
        self.n = int(sd["n"])
        self.sum.copy_(sd["sum"])
        self.outer.copy_(sd["outer"])


def _have_scipy() -> bool:
    try:
        import scipy.linalg  # noqa: F401
        return True
    except ImportError:
        return False


def frechet_distance(mu1, sigma1, mu2, sigma2, method: str = "auto") -> float:
    """|mu1 - mu2|^2 + tr(S1 + S2 - 2 sqrtm(S1 S2)) in fp64 on the host (the tool's :172-176).  method "scipy": the real part of
    scipy.linalg.sqrtm, as the tool; "eig": tr sqrtm(S1 S2) = sum_i Re sqrt(lambda_i(S1 S2)) from torch.linalg.eigvals (the
    eigenvalues of a product of two PSD matrices are real and >= 0 up to rounding); "auto": scipy where it imports."""
    if method not in ("auto", "scipy", "eig"):
        raise ValueError(f"method must be 'auto', 'scipy' or 'eig', got {method!r}")
    mu1, mu2 = np.asarray(mu1, dtype=np.float64), np.asarray(mu2, dtype=np.float64)
    s1, s2 = np.asarray(sigma1, dtype=np.float64), np.asarray(sigma2, dtype=np.float64)
    if mu1.shape != mu2.shape or s1.shape != s2.shape or s1.shape != (mu1.size, mu1.size):
        raise ValueError("frechet_distance: mu [D] and sigma [D, D] of both sides must agree")
    if method == "auto":
        method = "scipy" if _have_scipy() else "eig"
    gap = mu1 - mu2
    if method == "scipy":
        from scipy.linalg import sqrtm
        tr_root = float(np.trace(np.real(sqrtm(s1 @ s2))))  # rounding can leave a small imaginary part: the tool keeps the real part
    else:
        lam = torch.linalg.eigvals(torch.from_numpy(s1 @ s2))
        tr_root = float(torch.sqrt(lam).real.sum())
    return float(gap @ gap) + float(np.trace(s1)) + float(np.trace(s2)) - 2.0 * tr_root


class FID:
    """rFID between the reference and the reconstructed byte images: Inception features of both, two FrechetStats, the distance"""

    def __init__(self, inception: InceptionFeatures, group=None):
        self.inception, self.group = inception, group
        dev = inception.Conv2d_1a_3x3.conv.weight.device
        if dev.type != "cuda":
            raise RuntimeError("vtp_amd.FID runs on the MI355X kernels only: move the InceptionFeatures to a cuda device (no CPU path)")
        self.device = dev
        self.ref = FrechetStats(FEATURE_DIM, dev, group)
        self.rec = FrechetStats(FEATURE_DIM, dev, group)
        self._pre = None

    def _images(self, u8: torch.Tensor) -> torch.Tensor:
        if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
            raise ValueError(f"the byte images must be uint8 [B, H, W, 3], got {u8.dtype} {tuple(u8.shape)}")
        if self.inception.variant == "pytorch_fid":
            if not u8.is_cuda:
                raise ValueError("the byte images must live on the MI355X: there is no CPU path")
            B, H, W, _ = u8.shape
            img = torch.empty(B, 3, H, W, device=u8.device, dtype=F32)
            ops.u8_to_images(u8.contiguous(), img, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))  # ToTensor: u8 / 255
            return img
        if self._pre is None:  # transforms.Resize((299, 299)) + ToTensor of the tool's ImageFolder: PIL's bilinear, bit for bit
            from .preprocess import Preprocess
            self._pre = Preprocess.resize((299, 299), "bilinear", mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), device=self.device)
        host = u8.cpu().numpy()  # Preprocess takes decoded images on the host: one copy per batch
        return self._pre([host[i] for i in range(host.shape[0])])

    def features(self, u8: torch.Tensor) -> torch.Tensor:
        return self.inception(self._images(u8))

    def update(self, ref_u8: torch.Tensor, rec_u8: torch.Tensor) -> None:
        """ref_u8, rec_u8: uint8 [B, H, W, 3], the bytes of the tool's two PNG folders"""
        self.update_features(self.features(ref_u8), self.features(rec_u8))

    def update_features(self, f_ref: torch.Tensor, f_rec: torch.Tensor) -> None:
        self.ref.update(f_ref)
        self.rec.update(f_rec)

    def result(self, method: str = "auto") -> float:
        mu1, s1 = self.ref.mean_cov()
        mu2, s2 = self.rec.mean_cov()
        return frechet_distance(mu1, s1, mu2, s2, method)

    def reset(self) -> None:
        self.ref.reset()
        self.rec.reset()
