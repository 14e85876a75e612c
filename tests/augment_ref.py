"""Helper of the SSL-crop tests (not a test): a plain torch restatement, on the CPU, of the chain vtp_amd.MultiCrop runs per
crop (csrc/augment.hip, INTEGRATION.md "SSL crops") for ONE table row in a given dtype --

    x = u8 / 255 -> resized crop (crop the box, then antialiased bicubic to S x S, clamp to [0, 1]) -> flip -> colour jitter in
    the row's order -> grayscale -> 9 x 9 Gaussian blur (reflect padding by 4) -> solarize -> (x - mean) / std

written the way torchvision's float-tensor path writes it: the resize as the two weight matrices of
F.interpolate(mode="bicubic", antialias=True, align_corners=False) (rows first; tests/test_augment_host.py holds them to that
call), _blend / rgb_to_grayscale / _rgb2hsv / _hsv2rgb for the jitter, the blur as one conv2d with the outer product of the 1-D
kernel.  `crop` returns the normalised crop and the image just before solarize.  The mean / std are the fp32 constants in
either dtype; everything else is evaluated in the dtype asked for.

What this formulation does in fp32 against itself in fp64 (normalised units: one fp32 ulp of the largest output, 2.64, is 2.4e-7):
    144 crops at S = 16 and 32 from a 40 x 56 source (smooth, noise and near-gray images, all 24 orders, sigma 0.1 / 0.7 / 2.0)
                                                       3.9e-6 on the worst crop
    the cases below                                    1.2e-6 .. 1.7e-5; the largest are boxes up-sampled to 48 and 96, where the
                                                       fp32 rounding of a tap's position (4e-6 at 56) meets a noise image
    full-image box at S = Hs = Ws                      bit-equal to (u8 / 255 - mean) / std: the weights are exactly 0 and 1
    pixels within 1e-4 of the solarize threshold       0.017 % of the solarized crops' pixels (they may fall on either side: the
                                                       GPU test leaves them out)
    a constant image through the full chain            constant to 1.6e-6 (the renormalised taps sum to 1 within a few ulp)
tests/test_augment_host.py re-derives these; tests/test_augment_gpu.py uses the fp32-against-fp64 deviation of each case as the
`dev` of its bar."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # IMAGENET_DEFAULT_MEAN / STD
THRESHOLD = 128.0 / 255.0
FLIP, JITTER, GRAY, SOLARIZE = 1, 2, 4, 8


def row(box, flip=False, order=None, factors=(1.0, 1.0, 1.0, 0.0), gray=False, sigma=0.0, solarize=False):
    """one table row, float32 [16], written out by hand (vtp_amd.augment.encode_row is tested against this layout):
    0..3 box, 4 flags, 5..8 order (-1: none), 9..12 factors, 13 sigma"""
    r = np.zeros(16, dtype=np.float32)
    r[0:4] = box
    r[4] = FLIP * bool(flip) + JITTER * (order is not None) + GRAY * bool(gray) + SOLARIZE * bool(solarize)
    r[5:9] = -1
    if order is not None:
        r[5:5 + len(order)] = order
    r[9:13] = factors
    r[13] = sigma
    return r


def _cubic(x, a=-0.5):
    x = x.abs()
    near = ((a + 2) * x - (a + 3)) * x * x + 1
    far = ((a * x - 5 * a) * x + 8 * a) * x - 4 * a
    return torch.where(x < 1, near, torch.where(x < 2, far, torch.zeros_like(x)))


def resize_matrix(box, S, dtype):
    """[S, box]: row i holds the weights of output i over the crop's pixels -- scale = box / S, support 2 max(scale, 1), the taps
    int(center - support + 0.5) .. int(center + support + 0.5) cut to the crop and renormalised"""
    scale = torch.tensor(float(box), dtype=dtype) / S
    up = bool(scale >= 1)
    support = 2 * scale if up else torch.tensor(2.0, dtype=dtype)
    inv = 1 / scale if up else torch.tensor(1.0, dtype=dtype)
    center = scale * (torch.arange(S, dtype=dtype) + 0.5)
    lo = (center - support + 0.5).to(torch.int64).clamp_min(0)
    hi = (center + support + 0.5).to(torch.int64).clamp_max(box)
    k = torch.arange(box)
    w = _cubic((k.to(dtype)[None, :] - center[:, None] + 0.5) * inv)
    w = torch.where((k[None, :] >= lo[:, None]) & (k[None, :] < hi[:, None]), w, torch.zeros_like(w))
    return w / w.sum(1, keepdim=True)


def resized_crop(x, box, S):
    """x [3, Hs, Ws] in [0, 1] -> [3, S, S]: the crop, resized along x, then along y, clamped"""
    y0, x0, h, w = box
    c = x[:, y0:y0 + h, x0:x0 + w]
    t = c @ resize_matrix(w, S, x.dtype).T
    return (resize_matrix(h, S, x.dtype) @ t).clamp(0, 1)


def gray(x):
    r, g, b = x.unbind(0)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(0)


def blend(a, b, f):
    return (f * a + (1.0 - f) * b).clamp(0, 1)


def rgb2hsv(x):
    r, g, b = x.unbind(0)
    maxc, minc = x.max(0).values, x.min(0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return torch.stack((h, s, maxc))


def hsv2rgb(x):
    h, s, v = x.unbind(0)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - f * s)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    pick = lambda *o: torch.stack(o).gather(0, i[None])[0]
    return torch.stack((pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q)))


def hue(x, f):
    hsv = rgb2hsv(x)
    return hsv2rgb(torch.stack(((hsv[0] + f) % 1.0, hsv[1], hsv[2])))


def blur(x, sigma):
    t = torch.linspace(-4, 4, 9, dtype=x.dtype)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    k1 = pdf / pdf.sum()
    k2 = (k1[:, None] * k1[None, :]).expand(3, 1, 9, 9).contiguous()
    return F.conv2d(F.pad(x[None], (4, 4, 4, 4), mode="reflect"), k2, groups=3)[0]


def to_unit(u8, dtype):
    """uint8 [H, W, 3] -> [3, H, W] = u8 / 255 in dtype (ToTensor)"""
    return u8.permute(2, 0, 1).to(dtype) / 255


def normalise(x):
    m = torch.tensor(MEAN, dtype=F32).to(x.dtype).view(3, 1, 1)
    s = torch.tensor(STD, dtype=F32).to(x.dtype).view(3, 1, 1)
    return (x - m) / s


def crop(u8, r, S, dtype=F64):
    """one crop: u8 uint8 [Hs, Ws, 3], r one table row -> (normalised [3, S, S], the image just before solarize), in dtype"""
    r = np.asarray(r, dtype=np.float32)
    flags = int(r[4])
    fac = [float(v) for v in r[9:13]]  # the fp32 numbers of the table, exactly
    x = resized_crop(to_unit(u8, dtype), tuple(int(v) for v in r[0:4]), S)
    if flags & FLIP:
        x = x.flip(-1)
    if flags & JITTER:
        for op in (int(o) for o in r[5:9]):
            if op == 0:
                x = blend(x, torch.zeros_like(x), fac[0])
            elif op == 1:
                x = blend(x, gray(x).mean(), fac[1])
            elif op == 2:
                x = blend(x, gray(x), fac[2])
            elif op == 3:
                x = hue(x, fac[3])
    if flags & GRAY:
        x = gray(x).expand(3, -1, -1)
    if float(r[13]) > 0:
        x = blur(x, float(r[13]))
    pre = x
    if flags & SOLARIZE:
        x = torch.where(x >= THRESHOLD, 1.0 - x, x)
    return normalise(x), pre


def batch(u8, table, S, dtype=F64):
    """u8 [B, Hs, Ws, 3], table [N, 16] (crop n from image n % B) -> (out [N, 3, S, S], pre [N, 3, S, S]) in dtype"""
    B = u8.shape[0]
    both = [crop(u8[n % B], table[n], S, dtype) for n in range(len(table))]
    return torch.stack([o for o, _ in both]), torch.stack([p for _, p in both])


# ---- sources ----------------------------------------------------------------------------------------------------------------
def to_u8(x):
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def smooth(B, H, W, seed):
    """smooth colourful images: bicubic blow-up of an 8 x coarser noise, a few percent of the bytes at 0 or 255"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, 3, max(H // 8, 2), max(W // 8, 2), generator=g)
    z = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    return to_u8(0.5 + 0.28 * z / z.std())


def noise(B, H, W, seed):
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def near_gray(B, H, W, seed):
    """a smooth gray image with +-2 byte steps of colour: tiny chroma, many exactly gray pixels -- the hue's hard case"""
    g = torch.Generator().manual_seed(seed)
    base = smooth(B, H, W, seed)[..., :1].to(torch.int16).expand(B, H, W, 3)
    return (base + torch.randint(-2, 3, (B, H, W, 3), generator=g).to(torch.int16)).clamp(0, 255).to(torch.uint8)


def mixed(H=40, W=56, seed=11):
    """[3, H, W, 3]: one smooth, one noise, one near-gray image"""
    return torch.cat((smooth(1, H, W, seed), noise(1, H, W, seed + 1), near_gray(1, H, W, seed + 2)))


ORDERS = list(itertools.permutations(range(4)))
FACTORS = (1.3, 0.7, 1.15, -0.08)


def boxes(Hs, Ws):
    """the full image, all four corners, a 5 x 5 (upsampling), and 1 x 3 / 2 x 2 at the far corner"""
    h, w = Hs // 2, Ws // 2
    return [(0, 0, Hs, Ws), (0, 0, h, w), (0, Ws - w, h, w), (Hs - h, 0, h, w), (Hs - h, Ws - w, h, w), (7, 9, 5, 5),
            (Hs - 1, Ws - 3, 1, 3), (Hs - 2, Ws - 2, 2, 2)]


def _views(B, rows):
    """view-major table: every row repeated for the B images"""
    return np.stack([r for r in rows for _ in range(B)])


def cases():
    """name -> (u8 [B, Hs, Ws, 3], S, table): what tests/test_augment_gpu.py runs and tests/test_augment_host.py takes `dev` of"""
    src = mixed()
    B, Hs, Ws = src.shape[:3]
    big = smooth(1, 256, 256, 5)
    wide = smooth(1, 16, 128, 6)
    const = torch.tensor([90, 140, 200], dtype=torch.uint8).expand(1, Hs, Ws, 3).contiguous()
    full, part = (0, 0, Hs, Ws), (3, 5, 30, 41)
    chain = dict(order=(2, 1, 3, 0), factors=FACTORS)
    out = {}
    for S in (16, 48, 96):
        out[f"boxes_{S}"] = (src, S, _views(B, [row(b, flip=i % 2 == 1) for i, b in enumerate(boxes(Hs, Ws))]))
        out[f"chain_{S}"] = (src, S, _views(B, [row(part, True, sigma=1.1, solarize=True, **chain),
                                                row(full, False, gray=True, sigma=0.6, order=(3, 0, 1, 2), factors=FACTORS)]))
    out["each_op_16"] = (src, 16, _views(B, [row(part, order=(op,), factors=FACTORS) for op in range(4)]
                                         + [row(part, order=(3, 1), factors=FACTORS), row(full, order=(1,), factors=(1, 1.6, 1, 0))]))
    out["orders_16"] = (src, 16, _views(B, [row(part, i % 2 == 0, order=o, factors=FACTORS) for i, o in enumerate(ORDERS)]))
    out["gray_16"] = (src, 16, _views(B, [row(part, gray=True), row(full, True, gray=True, order=(0, 2), factors=FACTORS)]))
    out["blur_16"] = (src, 16, _views(B, [row(part, sigma=0.1), row(part, sigma=2.0), row(full, True, sigma=2.0)]))
    out["solarize_16"] = (src, 16, _views(B, [row(part, solarize=True), row(full, True, solarize=True, sigma=0.7)]))
    out["hue_near_gray_48"] = (near_gray(2, Hs, Ws, 21), 48, _views(2, [row(full, order=(3,), factors=(1, 1, 1, f)) for f in (-0.1, 0.5)]
                                                                   + [row(part, order=(3, 1, 2, 0), factors=FACTORS, sigma=0.9)]))
    out["constant_48"] = (const, 48, _views(1, [row(part, True, gray=False, sigma=1.3, solarize=True, **chain),
                                                row(full, order=(1, 0, 3, 2), factors=FACTORS, gray=True, sigma=2.0)]))
    out["ratio8_16"] = (wide, 16, _views(1, [row((0, 0, 16, 128)), row((0, 0, 16, 128), True, sigma=1.0, **chain)]))
    # sizes that are no multiple of 4 (no 16-byte stores), the smallest size the blur allows, ratio 8 on both axes over two tiles
    out["odd_10"] = (src, 10, _views(B, [row(part, True, sigma=1.1, solarize=True, **chain), row(full), row(full, order=(1,), factors=FACTORS)]))
    out["min_5"] = (src, 5, _views(B, [row((3, 5, 30, 40), sigma=2.0, **chain), row((7, 9, 5, 5), True, sigma=0.5)]))  # 40 / 5: ratio 8
    out["ratio8_33"] = (smooth(1, 264, 264, 7), 33, _views(1, [row((0, 0, 264, 264)), row((0, 0, 264, 264), True, sigma=1.0, **chain)]))
    out["global_256"] = (big, 256, _views(1, [row((0, 0, 256, 256)), row((20, 31, 190, 170), True, sigma=1.4, solarize=True, **chain)]))
    return out


def deviation(u8, S, table):
    """(ref64, pre64, dev): the fp64 evaluation and the largest deviation of the fp32 one from it, over pixels outside the
    solarize band of a solarized crop"""
    ref, pre = batch(u8, table, S, F64)
    r32, _ = batch(u8, table, S, F32)
    keep = keep_mask(table, pre)
    return ref, pre, float(((r32.double() - ref).abs() * keep).max())


def keep_mask(table, pre64, band=1e-4):
    """False where a solarized crop's fp64 value before solarize lies within `band` of the threshold"""
    sol = torch.tensor([(int(r[4]) & SOLARIZE) != 0 for r in table]).view(-1, 1, 1, 1)
    return ~(sol & ((pre64 - THRESHOLD).abs() <= band))
