"""A numpy restatement of PIL's 8-bit resampling (Resample.c) and of the four transform chains vtp_amd.Preprocess runs on the
device, written independently of vtp_amd/preprocess.py, plus the named cases the host and GPU tests share.

One 1-D pass takes `size_in` pixels over the box [in0, in1) to `out` pixels.  Coefficients in float64, normalised, rounded to
22-bit fixed point; per pixel and channel acc = 2^21 + sum K[j] src[xmin + j] in int32, dst = clamp(acc >> 22, 0, 255).
Image.resize runs the horizontal pass first, rounds it to uint8, then the vertical pass, and skips a pass whose size is unchanged
and whose box is the whole axis.

PIL is imported only inside the pil_* functions: the recorded outputs (tests/golden/preprocess_pil.safetensors, written by
tools/record_preprocess_golden.py) pin the restatement where PIL is not installed."""
import math

import numpy as np

BOX, BILINEAR, BICUBIC = "box", "bilinear", "bicubic"
FILTERS = (BOX, BILINEAR, BICUBIC)
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, BICUBIC: 2.0}
BITS = 22
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CLAMPED = [0, 0]  # values pass_1d has clamped at 0 and at 255 so far (the tests check that the cases reach both ends)


def _f(filt, x):
    if filt == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    x = abs(x)
    if filt == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(size_in, in0, in1, out, filt):
    """-> xmin int [out], n int [out], K int32 [out, ksize] (zero beyond n)"""
    scale = (in1 - in0) / out
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmin, n, K = np.zeros(out, np.int64), np.zeros(out, np.int64), np.zeros((out, ksize), np.int32)
    for xx in range(out):
        c = in0 + (xx + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        cnt = min(int(c + support + 0.5), size_in) - lo
        k, ww = [], 0.0
        for j in range(cnt):
            w = _f(filt, (j + lo - c + 0.5) * ss)
            k.append(w)
            ww += w
        for j in range(cnt):
            v = k[j] / ww if ww != 0.0 else k[j]
            K[xx, j] = int(v * (1 << BITS) - 0.5) if v < 0 else int(v * (1 << BITS) + 0.5)
        xmin[xx], n[xx] = lo, cnt
    return xmin, n, K


def pass_1d(src, axis, out, filt, in0=0, in1=None):
    """one pass along `axis` (0: vertical, 1: horizontal) of uint8 [H, W, 3]"""
    size_in = src.shape[axis]
    xmin, n, K = coeffs(size_in, in0, size_in if in1 is None else in1, out, filt)
    s = np.moveaxis(src, axis, 0).astype(np.int32)
    dst = np.empty((out,) + s.shape[1:], np.uint8)
    for xx in range(out):
        acc = np.full(s.shape[1:], 1 << (BITS - 1), np.int32)
        for j in range(int(n[xx])):
            acc = acc + K[xx, j] * s[xmin[xx] + j]
        CLAMPED[0] += int((acc >> BITS < 0).sum())
        CLAMPED[1] += int((acc >> BITS > 255).sum())
        dst[xx] = np.clip(acc >> BITS, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(dst, 0, axis))


def resize(src, h, w, filt):
    """Image.resize((w, h), filt) of uint8 [H, W, 3]: horizontal, then vertical, a pass of unchanged size skipped"""
    if src.shape[1] != w:
        src = pass_1d(src, 1, w, filt)
    if src.shape[0] != h:
        src = pass_1d(src, 0, h, filt)
    return src


# ---- the four chains -----------------------------------------------------------------------------------------------------------
def center_crop(src, S, flip=False):
    """center_crop_arr (ADM): halve with BOX while the short side >= 2 S, BICUBIC to the short side, centre crop"""
    while min(src.shape[:2]) >= 2 * S:
        src = resize(src, src.shape[0] // 2, src.shape[1] // 2, BOX)
    H, W = src.shape[:2]
    s = S / min(W, H)
    src = resize(src, round(H * s), round(W * s), BICUBIC)
    cy, cx = (src.shape[0] - S) // 2, (src.shape[1] - S) // 2
    out = src[cy:cy + S, cx:cx + S]
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def probe_eval(src, size, crop):
    """torchvision Resize(size, BICUBIC) on a PIL image, then CenterCrop(crop) (no padding: the crop must fit)"""
    H, W = src.shape[:2]
    if W <= H:
        w, h = size, int(size * H / W)
    else:
        h, w = size, int(size * W / H)
    src = resize(src, h, w, BICUBIC)
    top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
    return np.ascontiguousarray(src[top:top + crop, left:left + crop])


def zero_shot(src, S):
    return resize(src, S, S, BILINEAR)


def resized_crop(src, box, S, flip=False):
    """F.resized_crop on a PIL image: crop the box (y0, x0, h, w), BICUBIC to S x S, flip"""
    y0, x0, h, w = box
    out = resize(np.ascontiguousarray(src[y0:y0 + h, x0:x0 + w]), S, S, BICUBIC)
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


# ---- live PIL (imported here only) ----------------------------------------------------------------------------------------------
def _pil_filter(filt):
    from PIL import Image
    return {BOX: Image.BOX, BILINEAR: Image.BILINEAR, BICUBIC: Image.BICUBIC}[filt]


def pil_resize(src, h, w, filt):
    from PIL import Image
    return np.asarray(Image.fromarray(src).resize((w, h), _pil_filter(filt)))


def pil_center_crop(src, S, flip=False):
    from PIL import Image
    im = Image.fromarray(src)
    while min(*im.size) >= 2 * S:
        im = im.resize(tuple(x // 2 for x in im.size), resample=Image.BOX)
    s = S / min(*im.size)
    im = im.resize(tuple(round(x * s) for x in im.size), resample=Image.BICUBIC)
    arr = np.array(im)
    cy, cx = (arr.shape[0] - S) // 2, (arr.shape[1] - S) // 2
    out = arr[cy:cy + S, cx:cx + S]
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def pil_probe_eval(src, size, crop):
    from PIL import Image
    im = Image.fromarray(src)
    W, H = im.size
    if W <= H:
        w, h = size, int(size * H / W)
    else:
        h, w = size, int(size * W / H)
    if (w, h) != (W, H):
        im = im.resize((w, h), Image.BICUBIC)
    top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
    return np.asarray(im.crop((left, top, left + crop, top + crop)))


def pil_zero_shot(src, S):
    from PIL import Image
    return np.asarray(Image.fromarray(src).resize((S, S), Image.BILINEAR))


def pil_resized_crop(src, box, S, flip=False):
    from PIL import Image
    y0, x0, h, w = box
    im = Image.fromarray(src).crop((x0, y0, x0 + w, y0 + h)).resize((S, S), Image.BICUBIC)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
RESIZES = [(37, 53, 16, 16), (17, 23, 40, 31), (80, 95, 5, 7), (33, 33, 33, 20), (8, 8, 16, 16), (300, 211, 24, 17), (1, 9, 4, 4),
           (9, 1, 4, 4)]                                                   # H, W -> h, w
CC_SOURCES = [(16, 16), (45, 70), (67, 130), (129, 64), (15, 40), (33, 17), (21, 100)]   # H, W
CC_HALVINGS = [0, 1, 2, 2, 0, 0, 0]
PE_SOURCES = [(30, 47), (47, 30), (20, 20), (25, 20)]
PT_SOURCE = (40, 52)
S = 16


def image(H, W, seed, checker):
    """uniform noise, or a 0 / 255 checkerboard with noise (the bicubic overshoot then reaches both ends of the clamp)"""
    rng = np.random.default_rng([20240607, seed])
    noise = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    if not checker:
        return noise
    board = (((np.arange(H)[:, None] // 2 + np.arange(W)[None, :] // 2) % 2) * 255).astype(np.int32)[:, :, None]
    return np.clip(board + (noise.astype(np.int32) % 48) - 24, 0, 255).astype(np.uint8)


def train_boxes():
    """eight boxes (y0, x0, h, w) on the 40 x 52 source with their flips: six drawn, the full image, one pixel"""
    rng = np.random.default_rng([20240607, 99])
    H, W = PT_SOURCE
    boxes = []
    for _ in range(6):
        h, w = int(rng.integers(2, H + 1)), int(rng.integers(2, W + 1))
        boxes.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
    boxes += [(0, 0, H, W), (23, 31, 1, 1)]
    return boxes, [bool(i % 2) for i in range(len(boxes))]


_CASES = None


def cases():
    """name -> {"kind", "images": [uint8 [H, W, 3]], ...parameters}; every image of a case is one ragged batch"""
    global _CASES
    if _CASES is not None:
        return _CASES
    c, seed = {}, 0
    for (H, W, h, w) in RESIZES:
        for filt in FILTERS:
            c[f"resize_{H}x{W}_to_{h}x{w}_{filt}"] = {"kind": "resize", "images": [image(H, W, seed, seed % 2 == 1)], "size": (h, w),
                                                      "filter": filt}
            seed += 1
    cc = [image(H, W, 100 + i, i % 2 == 1) for i, (H, W) in enumerate(CC_SOURCES)]
    c["center_crop"] = {"kind": "center_crop", "images": cc, "S": S, "flip": False}
    c["center_crop_flip"] = {"kind": "center_crop", "images": cc, "S": S, "flip": True}
    c["probe_eval"] = {"kind": "probe_eval", "images": [image(H, W, 200 + i, i % 2 == 1) for i, (H, W) in enumerate(PE_SOURCES)],
                       "resize": 20, "crop": S}
    c["zero_shot"] = {"kind": "zero_shot", "images": cc, "S": S}
    boxes, flips = train_boxes()
    src = image(PT_SOURCE[0], PT_SOURCE[1], 300, True)
    c["probe_train"] = {"kind": "probe_train", "images": [src] * len(boxes), "boxes": boxes, "flips": flips, "S": S}
    _CASES = c
    return c


def _each(case, f_resize, f_cc, f_pe, f_zs, f_rc):
    k, im = case["kind"], case["images"]
    if k == "resize":
        return [f_resize(x, case["size"][0], case["size"][1], case["filter"]) for x in im]
    if k == "center_crop":
        return [f_cc(x, case["S"], case["flip"]) for x in im]
    if k == "probe_eval":
        return [f_pe(x, case["resize"], case["crop"]) for x in im]
    if k == "zero_shot":
        return [f_zs(x, case["S"]) for x in im]
    return [f_rc(x, b, case["S"], f) for x, b, f in zip(im, case["boxes"], case["flips"])]


def expected(case):
    """the restatement's uint8 [h, w, 3] outputs of a case, one per image"""
    return _each(case, resize, center_crop, probe_eval, zero_shot, resized_crop)


def pil_expected(case):
    """live PIL's outputs of a case"""
    return _each(case, pil_resize, pil_center_crop, pil_probe_eval, pil_zero_shot, pil_resized_crop)


def plans_for(pp_module, case):
    """(Preprocess object, plans) that run a case on the device"""
    P = pp_module
    k = case["kind"]
    sizes = [x.shape[:2] for x in case["images"]]
    if k == "resize":
        pp = P.Preprocess.resize(case["size"], case["filter"])
    elif k == "center_crop":
        pp = P.Preprocess.center_crop(case["S"], flip=case["flip"])
    elif k == "probe_eval":
        pp = P.Preprocess.probe_eval(case["resize"], case["crop"])
    elif k == "zero_shot":
        pp = P.Preprocess.zero_shot(case["S"])
    else:
        pp = P.Preprocess.probe_train(case["S"])
        return pp, [P.plan_resized_crop(H, W, b, case["S"], f) for (H, W), b, f in zip(sizes, case["boxes"], case["flips"])]
    return pp, pp.plan(sizes)


def to_float(u8):
    """ToTensor + Normalize in torchvision's fp32 op order, numpy: uint8 [h, w, 3] -> f32 [3, h, w]"""
    x = u8.astype(np.float32) / np.float32(255)
    return ((x - np.float32(MEAN)) / np.float32(STD)).transpose(2, 0, 1)


def run_jobs(packed):
    """the kernels of csrc/preprocess.hip in numpy, job row by job row, on what Preprocess.pack returned -> uint8 [B, h, w, 3].
    It reads only the job rows and the tables: a host check of the layout the device gets."""
    src = packed.src.numpy().astype(np.int64)
    scratch = np.full(max(packed.scratch_len, 1), 0xA5, np.int64)
    tab = packed.tab.astype(np.int64)
    out = np.zeros((packed.B, packed.out_h, packed.out_w, 3), np.uint8)
    for l, (first, count, _) in enumerate(packed.launches.tolist()):
        for row in packed.jobs[first:first + count].tolist():
            s, dst, oh, ow, sy, sx, ts, bnd, coef, ks, sub, flags = row[:12]
            base = scratch if flags & 1 else src
            oy, ox = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
            xs = ow - 1 - ox if flags & 4 else ox
            e = oy if flags & 2 else xs
            mn, n = tab[bnd + 2 * e] - sub, tab[bnd + 2 * e + 1]
            acc = np.full((oh, ow, 3), 1 << (BITS - 1), np.int64)
            for j in range(int(n.max())):
                on = j < n
                addr = np.where(on, s + oy * sy + xs * sx + (mn + j) * ts, 0)
                k = np.where(on, tab[np.where(on, coef + e * ks + j, 0)], 0)
                acc += k[:, :, None] * base[addr[:, :, None] + np.arange(3)]
            assert np.abs(acc).max() < 2 ** 31
            v = np.clip(acc >> BITS, 0, 255)
            if l == len(packed.launches) - 1:
                out[dst] = v
            else:
                scratch[dst:dst + oh * ow * 3] = v.reshape(-1)
    return out
