"""Torch restatement of what the reconstruction tool computes for rFID when pytorch_fid is missing (_calculate_fid_manual,
tools/test_reconstruction_hf.py:121-176): torchvision's inception_v3(transform_input=False) with fc = Identity in eval mode,
np.cov statistics and the sqrtm distance -- and of the pytorch_fid package's variant of the same network.  torchvision is not
needed: the network is written out below, unfolded (F.conv2d -> F.batch_norm(eps=1e-3) -> relu), on a plain state dict with
torchvision's keys, and runs in whatever dtype the input and the state dict have (fp32 or fp64, CPU or GPU).

It shares no code with vtp_amd/fid.py: the layer list below is written block by block the way torchvision's classes read."""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3


def gamma(n):
    """a-priori relative bound of n roundings in a chain: n u / (1 - n u), u = 2^-24 (fp32)"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def gamma64(n):
    u = 2.0 ** -53
    return n * u / (1.0 - n * u)


# name -> (Cin, Cout, kernel, stride, padding) of every BasicConv2d, in definition order
def conv_table():
    t = {}

    def c(name, cin, cout, k=1, s=1, p=0):
        t[name] = (cin, cout, k, s, p)

    c("Conv2d_1a_3x3", 3, 32, 3, 2)
    c("Conv2d_2a_3x3", 32, 32, 3)
    c("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    c("Conv2d_3b_1x1", 64, 80, 1)
    c("Conv2d_4a_3x3", 80, 192, 3)
    for blk, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):  # InceptionA
        c(blk + ".branch1x1", cin, 64)
        c(blk + ".branch5x5_1", cin, 48)
        c(blk + ".branch5x5_2", 48, 64, 5, 1, 2)
        c(blk + ".branch3x3dbl_1", cin, 64)
        c(blk + ".branch3x3dbl_2", 64, 96, 3, 1, 1)
        c(blk + ".branch3x3dbl_3", 96, 96, 3, 1, 1)
        c(blk + ".branch_pool", cin, pf)
    c("Mixed_6a.branch3x3", 288, 384, 3, 2)  # InceptionB
    c("Mixed_6a.branch3x3dbl_1", 288, 64)
    c("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    c("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):  # InceptionC
        c(blk + ".branch1x1", 768, 192)
        c(blk + ".branch7x7_1", 768, c7)
        c(blk + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        c(blk + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        c(blk + ".branch7x7dbl_1", 768, c7)
        c(blk + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        c(blk + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        c(blk + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        c(blk + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        c(blk + ".branch_pool", 768, 192)
    c("Mixed_7a.branch3x3_1", 768, 192)  # InceptionD
    c("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    c("Mixed_7a.branch7x7x3_1", 768, 192)
    c("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    c("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    c("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for blk, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):  # InceptionE
        c(blk + ".branch1x1", cin, 320)
        c(blk + ".branch3x3_1", cin, 384)
        c(blk + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        c(blk + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        c(blk + ".branch3x3dbl_1", cin, 448)
        c(blk + ".branch3x3dbl_2", 448, 384, 3, 1, 1)
        c(blk + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        c(blk + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        c(blk + ".branch_pool", cin, 192)
    return t


CONVS = conv_table()


def state_dict_keys():
    keys = []
    for name in CONVS:
        keys.append(name + ".conv.weight")
        keys += [name + ".bn." + s for s in ("weight", "bias", "running_mean", "running_var")]
    return keys


def seeded_state_dict(seed=0, dtype=torch.float32):
    """the recipe of InceptionFeatures.reset_parameters, restated: Kaiming-normal convolutions, BatchNorm weight and running_var
    in U(0.5, 1.5), bias and running_mean in N(0, 0.1^2); drawn in fp32 in definition order from one generator"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (cin, cout, k, _, _) in CONVS.items():
        kh, kw = (k, k) if isinstance(k, int) else k
        sd[name + ".conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        sd[name + ".bn.weight"] = 0.5 + torch.rand(cout, generator=g)
        sd[name + ".bn.running_var"] = 0.5 + torch.rand(cout, generator=g)
        sd[name + ".bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
    return {k: v.to(dtype) for k, v in sd.items()}


class Net:
    """the network over a state dict; `trace` collects (name, tensor) after every conv block / pool / Mixed block when given"""

    def __init__(self, sd, variant="torchvision", trace=None):
        assert variant in ("torchvision", "pytorch_fid")
        self.sd, self.fid, self.trace = sd, variant == "pytorch_fid", trace

    def note(self, name, x):
        if self.trace is not None:
            self.trace.append((name, x))
        return x

    def conv(self, name, x):
        _, _, _, s, p = CONVS[name]
        sd = self.sd
        x = F.conv2d(x, sd[name + ".conv.weight"], None, stride=s, padding=p)
        x = F.batch_norm(x, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"],
                         training=False, eps=BN_EPS)
        return self.note(name, F.relu(x))

    def avg(self, x):
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=not self.fid)

    def block_a(self, n, x):
        b1 = self.conv(n + ".branch1x1", x)
        b5 = self.conv(n + ".branch5x5_2", self.conv(n + ".branch5x5_1", x))
        b3 = self.conv(n + ".branch3x3dbl_3", self.conv(n + ".branch3x3dbl_2", self.conv(n + ".branch3x3dbl_1", x)))
        bp = self.conv(n + ".branch_pool", self.avg(x))
        return torch.cat([b1, b5, b3, bp], 1)

    def block_b(self, n, x):
        b3 = self.conv(n + ".branch3x3", x)
        bd = self.conv(n + ".branch3x3dbl_3", self.conv(n + ".branch3x3dbl_2", self.conv(n + ".branch3x3dbl_1", x)))
        return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)

    def block_c(self, n, x):
        b1 = self.conv(n + ".branch1x1", x)
        b7 = self.conv(n + ".branch7x7_3", self.conv(n + ".branch7x7_2", self.conv(n + ".branch7x7_1", x)))
        bd = x
        for i in range(1, 6):
            bd = self.conv(n + ".branch7x7dbl_%d" % i, bd)
        bp = self.conv(n + ".branch_pool", self.avg(x))
        return torch.cat([b1, b7, bd, bp], 1)

    def block_d(self, n, x):
        b3 = self.conv(n + ".branch3x3_2", self.conv(n + ".branch3x3_1", x))
        b7 = x
        for i in range(1, 5):
            b7 = self.conv(n + ".branch7x7x3_%d" % i, b7)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)

    def block_e(self, n, x, pool):
        b1 = self.conv(n + ".branch1x1", x)
        t = self.conv(n + ".branch3x3_1", x)
        b3 = torch.cat([self.conv(n + ".branch3x3_2a", t), self.conv(n + ".branch3x3_2b", t)], 1)
        t = self.conv(n + ".branch3x3dbl_2", self.conv(n + ".branch3x3dbl_1", x))
        bd = torch.cat([self.conv(n + ".branch3x3dbl_3a", t), self.conv(n + ".branch3x3dbl_3b", t)], 1)
        bp = self.conv(n + ".branch_pool", pool(x))
        return torch.cat([b1, b3, bd, bp], 1)

    def __call__(self, x):
        if self.fid:
            x = 2 * F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) - 1
        x = self.conv("Conv2d_1a_3x3", x)
        x = self.conv("Conv2d_2a_3x3", x)
        x = self.conv("Conv2d_2b_3x3", x)
        x = self.note("maxpool1", F.max_pool2d(x, 3, 2))
        x = self.conv("Conv2d_3b_1x1", x)
        x = self.conv("Conv2d_4a_3x3", x)
        x = self.note("maxpool2", F.max_pool2d(x, 3, 2))
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = self.note(n, self.block_a(n, x))
        x = self.note("Mixed_6a", self.block_b("Mixed_6a", x))
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self.note(n, self.block_c(n, x))
        x = self.note("Mixed_7a", self.block_d("Mixed_7a", x))
        x = self.note("Mixed_7b", self.block_e("Mixed_7b", x, self.avg))
        last_pool = (lambda v: F.max_pool2d(v, 3, 1, 1)) if self.fid else self.avg
        x = self.note("Mixed_7c", self.block_e("Mixed_7c", x, last_pool))
        return torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)


@torch.no_grad()
def features(sd, x, variant="torchvision", trace=None):
    return Net(sd, variant, trace)(x)


def statistics(act):
    """the tool's :169: mean and np.cov of the activations [n, D], fp64"""
    act = np.asarray(act, dtype=np.float64)
    return act.mean(axis=0), np.cov(act, rowvar=False)


def frechet(mu1, sigma1, mu2, sigma2):
    """the tool's :172-176: squared distance of the means plus tr(S1 + S2 - 2 (S1 S2)^(1/2)), the matrix root by scipy, its real part"""
    from scipy.linalg import sqrtm
    root = np.real(sqrtm(np.matmul(sigma1, sigma2)))
    delta = np.asarray(mu1) - np.asarray(mu2)
    return float(np.dot(delta, delta) + np.trace(sigma1) + np.trace(sigma2) - 2.0 * np.trace(root))
