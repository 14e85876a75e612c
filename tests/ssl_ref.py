"""The self-supervised and contrastive loss kernels (csrc/ssl.hip, csrc/losses.hip, the loss part of csrc/clip.hip and colsum_bf16_rows
of csrc/elementwise.hip) restated in float64 on the bf16- or fp32-rounded inputs the kernels get, the case tables of
tests/test_ssl_kernels_gpu.py, and the bars.  Not a test module; tests/test_ssl_ref_host.py pins the references against independent
torch code and shows, at the GPU test's own inputs, that wrong variants miss the bars.  Everything here runs on the CPU and nothing
imports vtp_amd.  SigLIP, KoLeo and Sinkhorn-Knopp take their definitions from oracle/loss_oracle.py.

Every reference that is a sum also returns the sum of the absolute values of its terms; the bars are built from those.

Bars.  U = 2^-24 is the unit roundoff of fp32 (half an ulp).  A sum of n terms formed sequentially, or through a tree of that many
levels, is off by at most n U sum|terms| (first order; each bar counts the roundings of the kernel's own order: the longest
per-thread chain plus the levels of the wave and block trees).  `__expf(x)` is v_exp_f32 after one multiply by log2 e: its relative
error is (|x| + 2) U, the rounding of x log2 e seen through the exponential plus one ulp of the instruction.  `__logf` is v_log_f32
times ln 2: 2 U |result| and one ulp.  sqrt, rsqrt and the division count one ulp (2 U) each.  A bf16 output adds 2^-8 |ref|: half an
ulp of bf16 is 2^(e-8) for a reference in [2^e, 2^(e+1)), at most 2^-8 |ref|.  A value below 2^-126 is flushed to zero by v_exp_f32
and by the conversion, so bars of outputs that can be that small carry FLUSH = 2^-126 (a term the first derivation forgot; without
it the row with one logit 8.0 above the rest, whose other probabilities are e^-200, cannot be met by any fp32 kernel).  Atomic
accumulation into one address from n workgroups may come in any order: n U (|prefill| + sum|terms|).  None of the constants was
fitted to what the kernels give."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss_oracle as LO

BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
U = 2.0 ** -24
BF_HALF_ULP = 2.0 ** -8
FLUSH = 2.0 ** -126
SENTINEL = 7.0


def f32(x) -> float:
    """the fp32 value a C `float` argument holds"""
    return float(np.float32(x))


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def cdiv(a, b):
    return -(-a // b)


def ratio(got, ref, bar) -> float:
    """worst |got - ref| / bar over every element; a NaN or an infinity in `got` is an infinite ratio; a zero bar must be met exactly"""
    got, ref = torch.as_tensor(got).detach().to(F64).cpu(), torch.as_tensor(ref).detach().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    bar = torch.as_tensor(bar, dtype=F64).expand_as(err)
    inf = torch.full_like(err, float("inf"))
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    r = torch.where(torch.isfinite(got), r, inf)
    return float(r.max())


def unit_rows(B, D, g):
    """fp32 rows normalised in float64 before the rounding"""
    return F.normalize(torch.randn(B, D, generator=g, dtype=F64), dim=-1).to(F32)


# ------------------------------------------------------------------------------------------------------- softmax_center
SOFTMAX_K = (8, 1528, 2040, 2048, 2056, 8184, 8192, 8200, 16400, 65536, 65544)
SOFTMAX_T = (1, 3)
SOFTMAX_INV_TEMP = 1.0 / 0.07
HAND_INV_TEMP = 25.0


def softmax_case(K, T, with_center):
    g = gen(K, T, 1)
    logits = 0.8 * torch.randn(T, K, generator=g)
    logits[:, K - 3] = 4.0          # the largest logit (five sigma) sits in the last columns: a tail left out of a sum cannot hide
    center = 0.3 * torch.randn(K, generator=g) if with_center else None
    return logits.to(BF), center


def softmax_hand_case(K, with_center):
    """row 0 constant, row 1 with one logit 8.0 above the rest; z = (logit - centre) * 25 reaches +-200 in row 0 with the centre
    given and +-100 in row 1, so exp(z) overflows fp32 unless the row maximum is subtracted.  The centre is a constant that bf16
    arithmetic takes away exactly (8.5 - 0.5 = 8)."""
    c = 0.5 if with_center else 0.0
    logits = torch.full((2, K), 8.0 + c)
    logits[1] = -4.0 + c
    logits[1, K - 3] = 4.0 + c           # in the last columns, like the largest logit of softmax_case
    return logits.to(BF), (torch.full((K,), c) if with_center else None)


def scaled_logits(logits, center, inv_temp):
    z = logits.to(F64)
    if center is not None:
        z = z - center.to(F64)
    return z * f32(inv_temp)


def softmax_center_ref(logits, center, inv_temp):
    """-> (probs, se, z): probs = softmax((logits - centre) * inv_temp); se = sum exp(z - max), whose terms are all positive (it is
    its own sum of absolute values); z the scaled logits"""
    z = scaled_logits(logits, center, inv_temp)
    e = torch.exp(z - z.amax(1, keepdim=True))
    se = e.sum(1, keepdim=True)
    return e / se, se, z


def lse_steps(K, online=True):
    """roundings on the longest path of a row's sum of exponentials.  Three-pass / dino_ce form (row_lse, 256 threads): a thread walks
    8 ceil(K / 2048) elements with the running maximum (rescale multiply, exponential's own ulp, add: 4 per element), then 6 shuffle
    levels and the 4 wave partials, again 4 each.  Register form (8192 <= K <= 65536, 1024 threads): 8 ceil(K / 8192) plain adds, 6
    shuffle levels, 16 wave partials."""
    if online:
        return 4 * (8 * cdiv(K, 2048) + 6 + 4)
    return 8 * cdiv(K, 8192) + 6 + 16


def softmax_is_reg(K):
    return 8192 <= K <= 65536


def softmax_bar(ref, z, K):
    """bf16 output.  z = fl(fl(l - c) it) is off by 2 U |z| <= 2 U Z; x = z - max by 4 U Z + U X (X the row's range); so a numerator is
    off by (|x| + 2) U + 4 U Z + U X <= U (2 X + 2 + 4 Z) relatively, the denominator by the same plus its summation, and the running
    maximum's rescales telescope to one more X; 1 / se and the product add 2 U."""
    Z = z.abs().amax(1, keepdim=True)
    X = z.amax(1, keepdim=True) - z.amin(1, keepdim=True)
    rel = U * (lse_steps(K, not softmax_is_reg(K)) + X + 2 * (2 * X + 2 + 4 * Z) + 2)
    return BF_HALF_ULP * ref.abs() + rel * ref.abs() + FLUSH


# ------------------------------------------------------------------------------------------------------- dino_ce
DINO_K = (8, 1528, 2048, 4104, 65536)
DINO_INV_TEMP = 10.0
DINO_PREFILL = 3.0
#            t0  t1   w      two targets, one target, t0 = -1, w = 0 with a valid t0, and two more live rows
DINO_ROWS = ((0, 1, 0.37), (2, -1, 1.0), (-1, -1, 0.5), (1, 3, 0.0), (3, 0, 0.125), (1, -1, 2.5))


def dino_case(K):
    g = gen(K, 2)
    S = (0.8 * torch.randn(len(DINO_ROWS), K, generator=g)).to(BF)
    P = softmax_center_ref((0.8 * torch.randn(4, K, generator=g)).to(BF), None, SOFTMAX_INV_TEMP)[0].to(BF)
    t0 = torch.tensor([r[0] for r in DINO_ROWS], dtype=I32)
    t1 = torch.tensor([r[1] for r in DINO_ROWS], dtype=I32)
    w = torch.tensor([r[2] for r in DINO_ROWS], dtype=F32)
    return S, P, t0, t1, w


def dino_ce_ref(S, P, t0, t1, w, inv_temp):
    """per row r with w != 0 and t0 >= 0:  loss[r] = w sum_k -q[k] lsm[k],  dS[r] = w inv_temp (n_targets softmax(z) - q),
    z = S inv_temp, lsm = log_softmax(z), q = P[t0] + P[t1] (t1 < 0: P[t0] alone).  Other rows: loss 0, dS 0.
    -> dict(loss [T], loss_abs [T] = w sum |q lsm|, dS [T, K], and what the bars need)"""
    it = f32(inv_temp)
    z = S.to(F64) * it
    lse = torch.logsumexp(z, 1, keepdim=True)
    lsm = z - lse
    live = ((w != 0) & (t0 >= 0)).view(-1, 1).to(F64)
    Pd = P.to(F64)
    two = (t1 >= 0).view(-1, 1).to(F64)
    q = Pd[t0.clamp_min(0).long()] + two * Pd[t1.clamp_min(0).long()]
    nt = 1.0 + two
    wd = w.to(F64).view(-1, 1)
    terms = -(q * lsm) * wd * live
    dS = wd * it * (nt * torch.exp(lsm) - q) * live
    return dict(loss=terms.sum(1), loss_abs=terms.abs().sum(1), dS=dS, z=z, lse=lse, lsm=lsm, q=q * live, nt=nt, w=wd * live, it=it,
                live=live)


def _dino_dlsm(r, K):
    """|error| of lsm = fl(z - lse) per row [T, 1]: z one rounding (U Z); se relatively lse_steps U + X U (rescales) + 2 (X + 2 + 2 Z) U
    (arguments); the logarithm 2 U |log se| + 2 U; the sum mx + log se and the difference U |lse| + U |lsm| <= 2 U (|lse| + Z)"""
    z, lse = r["z"], r["lse"]
    Z = z.abs().amax(1, keepdim=True)
    X = z.amax(1, keepdim=True) - z.amin(1, keepdim=True)
    logse = (lse - z.amax(1, keepdim=True)).abs()
    return U * (Z + lse_steps(K) + X + 2 * (X + 2 + 2 * Z) + 2 * logse + 2 + 2 * (lse.abs() + Z))


def dino_loss_bar(r, K, prefill, workgroups):
    """fp32 scalar.  Per row: w [ (chain + 2) U sum |q lsm| + sum(q) dlsm ] with chain = 8 ceil(K / 2048) + 6 + 4, the product w * loss
    one more U; then one atomic add per workgroup onto the prefilled accumulator.  -> (per-row bars [T], bar of the whole launch)"""
    chain = 8 * cdiv(K, 2048) + 6 + 4
    rows = (chain + 3) * U * r["loss_abs"] + (r["w"].abs() * r["q"].sum(1, keepdim=True) * _dino_dlsm(r, K)).view(-1)
    total = rows.sum() + workgroups * U * (abs(prefill) + r["loss_abs"].sum())
    return rows + U * (abs(prefill) + r["loss_abs"]), total


def dino_ds_bar(r, K):
    """bf16 output w it (nt p - q): p = exp(lsm) is off by (|lsm| + 2) U + dlsm relatively; the difference and the two products by
    3 U (nt p + q)"""
    p = torch.exp(r["lsm"])
    fp32 = (r["w"] * r["it"]).abs() * (r["nt"] * p * ((r["lsm"].abs() + 2) * U + _dino_dlsm(r, K)) + 3 * U * (r["nt"] * p + r["q"]))
    return BF_HALF_ULP * r["dS"].abs() + fp32 + FLUSH


# ------------------------------------------------------------------------------------------------------- center_ema
EMA_K = (1, 255, 257, 65536)
EMA_COUNTS = (None, 0.0, 0.5, 5.0)     # None: the count comes from the host as inv_count = 1 / 7
EMA_HOST_INV_COUNT = 1.0 / 7.0
EMA_MOMENTUM = 0.9


def ema_case(K):
    g = gen(K, 3)
    return 0.3 * torch.randn(K, generator=g), 5.0 * torch.randn(K, generator=g)


def center_ema_ref(center, col_sum, inv_count, count, momentum, clamp=True):
    """m c + (1 - m) col_sum / max(count, 1)   (count None: times inv_count)  -> (value, sum of |terms|)"""
    m = f32(momentum)
    ic = f32(inv_count) if count is None else 1.0 / (max(f32(count), 1.0) if clamp else f32(count) or 1e-300)
    a, b = m * center.to(F64), (1.0 - m) * col_sum.to(F64) * ic
    return a + b, a.abs() + b.abs()


def ema_bar(sumabs):
    """fp32: 1 - m, its two products, the reciprocal of the count, m c and the sum: 6 roundings"""
    return 6 * U * sumabs


# ------------------------------------------------------------------------------------------------------- weight norm
WN_CASES = ((1, 8), (63, 256), (64, 256), (65, 256), (130, 200), (70, 264), (66, 512), (9, 520))
WN_PREFILL = 1.5
WN_MIN_SUMSQ = 2.0 ** -126


def wn_case(K, C):
    g = gen(K, C, 4)
    v = 0.02 * torch.randn(K, C, generator=g)
    if K > 1:
        v[1] *= 1e-15       # a prototype row of norm 1e-16: its sum of squares, about 1e-33, is still a normal fp32 number (see below)
    gain = (torch.rand(K, generator=g) + 0.5) * torch.where(torch.rand(K, generator=g) < 0.25, -1.0, 1.0)
    dW = torch.randn(K, C, generator=g)
    return v, gain, dW


def weight_norm_prep_ref(v, gain):
    """-> (weff = g v / |v|, inv = 1 / |v|, s = sum v^2, all terms positive).  Specified for rows whose sum of squares is a normal fp32
    number; below 2^-126 the kernel, like the fp32 parametrisation of torch, divides by zero (WN_MIN_SUMSQ, checked by the host test)"""
    vd = v.to(F64)
    s = (vd * vd).sum(1)
    inv = s.rsqrt()
    return gain.to(F64).view(-1, 1) * inv.view(-1, 1) * vd, inv, s


def wn_inv_bar(inv, C):
    """s: ceil(C / 64) adds per lane, 6 shuffle levels, the square: halved by the root; rsqrt one ulp"""
    return U * inv.abs() * ((cdiv(C, 64) + 6 + 1) / 2 + 2)


def wn_weff_bar(weff, C):
    """bf16 of v * (g * inv): two more roundings"""
    return BF_HALF_ULP * weff.abs() + U * weff.abs() * ((cdiv(C, 64) + 6 + 1) / 2 + 4)


def weight_norm_bwd_ref(dW, v, gain, inv, projection=True):
    """with vhat = v inv:  dg = <dW, vhat>,  dv = g inv (dW - dg vhat)   -> dict(dv, dv_abs, dg, dg_abs)"""
    dWd, vd, invd, gd = dW.to(F64), v.to(F64), inv.to(F64).view(-1, 1), gain.to(F64).view(-1, 1)
    t = dWd * vd * invd
    dot, dot_abs = t.sum(1, keepdim=True), t.abs().sum(1, keepdim=True)
    sc, vh = gd * invd, vd * invd
    dv = sc * (dWd - (dot * vh if projection else 0.0))
    return dict(dv=dv, dv_abs=sc.abs() * (dWd.abs() + (dot * vh).abs()), dg=dot.view(-1), dg_abs=dot_abs.view(-1), scvh=(sc * vh).abs())


def wn_bwd_bars(r, C, prefill):
    """dot: ceil(C / 64) lane terms of two products each, 6 levels.  dg += dot and dv += sc (dW - dot vh): 5 roundings on the terms,
    dot's error through |sc vh|, one rounding of the accumulation  -> (dv bar, dg bar)"""
    ddot = (cdiv(C, 64) + 6 + 2) * U * r["dg_abs"]
    dg = ddot + U * (abs(prefill) + r["dg_abs"])
    dv = 5 * U * r["dv_abs"] + r["scvh"] * ddot.view(-1, 1) + U * (abs(prefill) + r["dv_abs"])
    return dv, dg


# ------------------------------------------------------------------------------------------------------- l2norm
L2_D = (1, 255, 256, 257, 768)
L2_EPS = (1e-12, 1e-8)
L2_ROWS = 3   # row 1 is all zero


def l2_case(D):
    g = gen(D, 5)
    x = torch.randn(L2_ROWS, D, generator=g)
    x[1] = 0
    dy = torch.randn(L2_ROWS, D, generator=g)
    return x, dy


def l2norm_fwd_ref(x, eps):
    """-> (y = x r, r = 1 / max(|x|, eps), s = sum x^2)"""
    xd = x.to(F64)
    s = (xd * xd).sum(1)
    r = 1.0 / s.sqrt().clamp_min(f32(eps))
    return xd * r.view(-1, 1), r, s


def l2_steps(D):
    return cdiv(D, 256) + 6 + 4 + 1


def l2_inv_bar(r, D):
    """the sum of squares halved by the root, the root, the reciprocal (an ulp each), and the rounding of eps itself"""
    return U * r.abs() * (l2_steps(D) / 2 + 2 + 2 + 1)


def l2_y_bar(y, D):
    return U * y.abs() * (l2_steps(D) / 2 + 2 + 2 + 2)


def l2norm_bwd_ref(dy, y, inv):
    """dx = inv (dy - y <y, dy>)  -> dict(dx, dx_abs, s_abs, ry)"""
    dyd, yd, r = dy.to(F64), y.to(F64), inv.to(F64).view(-1, 1)
    t = dyd * yd
    s, s_abs = t.sum(1, keepdim=True), t.abs().sum(1, keepdim=True)
    return dict(dx=r * (dyd - yd * s), dx_abs=r.abs() * (dyd.abs() + (yd * s).abs()), s_abs=s_abs, ry=(r * yd).abs())


def l2_bwd_bar(r, D):
    return 3 * U * r["dx_abs"] + r["ry"] * l2_steps(D) * U * r["s_abs"]


# ------------------------------------------------------------------------------------------------------- CLIP / SigLIP
PAIR_SHAPES = ((1, 1, 0), (3, 255, 252), (4, 256, 0), (5, 257, 252), (257, 257, 0))     # (B_local, B_all, label offset)
PAIR_D = (4, 128, 772)
PAIR_SCALES = (0.0, math.log(100.0))
SIGLIP_BIASES = (-10.0, 10.0)


def pair_prefill(ls):
    """what the accumulators of the pair losses hold before the launch: of the size of the results, which grow with the scale (the
    host test shows that each exceeds every bar it meets, so that `=` written for `+=` cannot pass)"""
    return 0.75 if ls == 0.0 else 48.0



def pair_case(Bl, Bg, off, D):
    """unit fp32 rows: all texts and images, each image a little nearer to its own text (cosine about 0.1: at a scale of 100 the
    logits do not saturate, so that the loss and its gradients are not all but zero)"""
    g = gen(Bl, Bg, off, D, 6)
    txt_all = unit_rows(Bg, D, g)
    noise = torch.randn(Bg, D, generator=g, dtype=F64)
    img_all = F.normalize(noise / math.sqrt(D) + 0.1 * txt_all.to(F64), dim=-1).to(F32)
    return img_all[off:off + Bl].clone(), txt_all[off:off + Bl].clone(), img_all, txt_all


def _logits(a, b, ls):
    """-> (L = exp(ls) a b^T, its error bound): the dot is D products added in groups of four (at most D roundings on a path), the
    scale is __expf(ls), (|ls| + 2) U, and one product"""
    s = math.exp(f32(ls))
    ad, bd = a.to(F64), b.to(F64)
    return s * ad @ bd.T, U * s * (a.shape[1] + abs(f32(ls)) + 3) * (ad.abs() @ bd.abs().T), s


def _row_steps(N):
    return cdiv(N, 256) + 6 + 4


def _ce_side(a_l, b_all, ls, off, w, label_offset=True):
    """one direction of the CLIP loss: rows of a_l against all rows of b_all"""
    L, EL, s = _logits(a_l, b_all, ls)
    Bl, N = L.shape
    lab = torch.arange(Bl) + (off if label_offset else 0)
    lse = torch.logsumexp(L, 1, keepdim=True)
    arg = L - lse
    p = torch.exp(arg)
    G = w * p
    G[torch.arange(Bl), lab] -= w
    terms = w * (lse.view(-1) - L[torch.arange(Bl), lab])
    # errors: se relatively (steps + 2 X + 2) U + 2 EL (arguments and the maximum); log 2 U |log se| + 2 U; lse = mx + log se
    ELm = EL.amax(1, keepdim=True)
    X = L.amax(1, keepdim=True) - L.amin(1, keepdim=True)
    logse = (lse - L.amax(1, keepdim=True)).abs()
    dlse = 3 * ELm + U * (_row_steps(N) + 2 * X + 2 + 2 * logse + 2 + lse.abs())
    dterms = w * (dlse.view(-1) + EL[torch.arange(Bl), lab] + U * (lse.view(-1).abs() + L[torch.arange(Bl), lab].abs())) + U * terms.abs()
    darg = EL + dlse + U * arg.abs()
    dG = w * p * ((arg.abs() + 2) * U + darg) + 2 * U * (G.abs() + w * p) + FLUSH
    return dict(L=L, EL=EL, s=s, G=G, dG=dG, terms=terms, dterms=dterms, a=a_l.to(F64), b=b_all.to(F64), ls=f32(ls))


def _grad_rows(d):
    """exp(ls) G b and exp(ls) G^T a with their bars: a path of N (or B_local) products, the scale as above, the error of G"""
    G, dG, a, b, s = d["G"], d["dG"], d["a"], d["b"], d["s"]
    k = abs(d["ls"]) + 4
    rows = s * G @ b
    rows_bar = U * (G.shape[1] + k) * s * (G.abs() @ b.abs()) + s * (dG @ b.abs()) + FLUSH
    cols = s * G.T @ a
    cols_bar = U * (G.shape[0] + k) * s * (G.abs().T @ a.abs()) + s * (dG.T @ a.abs()) + FLUSH
    return rows, rows_bar, cols, cols_bar


def _dls(d):
    """d log-scale = sum G L: per row a sum of N products, the errors of G and L; then one atomic per workgroup"""
    G, L = d["G"], d["L"]
    val, sabs = (G * L).sum(), (G * L).abs().sum()
    bar = U * (_row_steps(L.shape[1]) + 1) * sabs + (d["dG"] * L.abs() + G.abs() * d["EL"]).sum()
    return val, sabs, bar


def clip_ref(img_l, txt_l, img_all, txt_all, ls, off, prefill=0.0, weight=0.5, label_offset=True):
    """OpenCLIP ClipLoss on local rows against gathered rows: loss = w sum_m [CE(L1[m], off + m) + CE(L2[m], off + m)], w = 0.5 / B_local,
    L1 = e^ls img_l txt_all^T, L2 = e^ls txt_l img_all^T; the gradients treat the four feature matrices as independent.
    -> dict name -> (value, bar); loss and d_logit_scale as increments onto `prefill`"""
    Bl = img_l.shape[0]
    w = f32(np.float32(weight) / np.float32(Bl))
    s1 = _ce_side(img_l, txt_all, ls, off, w, label_offset)
    s2 = _ce_side(txt_l, img_all, ls, off, w, label_offset)
    out = {}
    tabs = s1["terms"].abs().sum() + s2["terms"].abs().sum()
    out["loss"] = (s1["terms"].sum() + s2["terms"].sum(), s1["dterms"].sum() + s2["dterms"].sum() + 2 * Bl * U * (abs(prefill) + tabs))
    v1, a1, b1 = _dls(s1)
    v2, a2, b2 = _dls(s2)
    out["d_logit_scale"] = (v1 + v2, b1 + b2 + 2 * Bl * U * (abs(prefill) + a1 + a2))
    r, rb, c, cb = _grad_rows(s1)
    out["d_img_local"], out["d_txt_all"] = (r, rb), (c, cb)
    r, rb, c, cb = _grad_rows(s2)
    out["d_txt_local"], out["d_img_all"] = (r, rb), (c, cb)
    return out


def siglip_parts(img_l, txt_all, ls, bias, off, label_offset=True, dls_with_bias=False):
    """the SigLIP loss by the kernel's own formulas in float64, with the magnitudes the bars need (the reference VALUES come from
    oracle/loss_oracle.py through siglip_ref; the host test shows the two agree).  z = L + b, y = +1 on the label else -1, t = -y z:
    loss = w sum softplus(t), g = dloss/dz = -w y sigmoid(t), d_ls = sum g L, d_bias = sum g, w = 1 / B_local."""
    L, EL, s = _logits(img_l, txt_all, ls)
    Bl, N = L.shape
    w = f32(1.0 / Bl)
    b = f32(bias)
    y = -torch.ones_like(L)
    y[torch.arange(Bl), torch.arange(Bl) + (off if label_offset else 0)] = 1.0
    z = L + b
    t = -y * z
    sp = F.softplus(t, threshold=1e9)
    g = -w * y * torch.sigmoid(t)
    # errors: z off by EL + U |z|; softplus has slope <= 1, its exponential, log1p and sum cost U (4 + 2 sp);
    # sigmoid(t) relatively (|t| + 2) U for the exponential, 3 U for 1 +, / and the product, and dz through the slope 1 - sigmoid <= 1
    dz = EL + U * z.abs()
    dsp = dz + U * (4 + 2 * sp)
    dg = g.abs() * ((t.abs() + 2) * U + 3 * U + dz) + FLUSH
    return dict(L=L, EL=EL, s=s, G=g, dG=dg, a=img_l.to(F64), b=txt_all.to(F64), ls=f32(ls), sp=sp, dsp=dsp, w=w,
                gl=g * (z if dls_with_bias else L))


def siglip_ref(img_l, txt_all, ls, bias, off, prefill=0.0):
    """values: oracle/loss_oracle.py siglip_loss and its float64 autograd; bars: from siglip_parts.  -> dict name -> (value, bar)"""
    i64, t64 = img_l.to(F64).requires_grad_(True), txt_all.to(F64).requires_grad_(True)
    l64, b64 = torch.tensor(f32(ls), dtype=F64, requires_grad=True), torch.tensor(f32(bias), dtype=F64, requires_grad=True)
    loss = LO.siglip_loss(i64, t64, l64, b64, off)
    loss.backward()
    p = siglip_parts(img_l, txt_all, ls, bias, off)
    return siglip_bars(p, dict(loss=loss.detach(), d_img_local=i64.grad, d_txt_all=t64.grad, d_logit_scale=l64.grad, d_logit_bias=b64.grad),
                       prefill)


def siglip_values(p):
    """the five results from the parts (for the wrong variants of the host test)"""
    rows, _, cols, _ = _grad_rows(p)
    return dict(loss=p["w"] * p["sp"].sum(), d_img_local=rows, d_txt_all=cols, d_logit_scale=p["gl"].sum(), d_logit_bias=p["G"].sum())


def siglip_bars(p, values, prefill):
    Bl, N = p["L"].shape
    steps = _row_steps(N) + 1
    _, rb, _, cb = _grad_rows(p)
    w, sp, G, L = p["w"], p["sp"], p["G"], p["L"]
    atom = lambda sabs: Bl * U * (abs(prefill) + sabs)
    bars = dict(loss=w * (p["dsp"].sum() + U * steps * sp.sum()) + atom(w * sp.sum()),
                d_img_local=rb, d_txt_all=cb,
                d_logit_scale=U * steps * (G * L).abs().sum() + (p["dG"] * L.abs() + G.abs() * p["EL"]).sum() + atom((G * L).abs().sum()),
                d_logit_bias=U * steps * G.abs().sum() + p["dG"].sum() + atom(G.abs().sum()))
    # the values are the oracle's, with the exact 1 / B_local: the weight the kernel gets is its fp32 rounding, one more U
    return {k: (values[k], bars[k] + U * torch.as_tensor(values[k]).abs()) for k in bars}


# ------------------------------------------------------------------------------------------------------- KoLeo
#              B    D      identical rows (groups)       queries planted beside a group: (row, beside)
KOLEO_CASES = ((2, 4, (), ()),
               (2, 4, ((0, 1),), ()),
               (3, 256, ((0, 2),), ()),
               (256, 260, (), ()),
               (257, 64, ((0, 256),), ((5, 0),)),                 # candidates 0 and 256 sit in thread 0's own loop
               (260, 768, ((3, 131, 259),), ((7, 3),)),          # 3 and 259 in thread 3's loop; query 3 itself: 131 against 259
               (4, 16384, (), ()),
               (4, 16384, ((2, 3),), ()))
KOLEO_EPS = 1e-8
KOLEO_PREFILL = 0.25


def koleo_case(B, D, groups, beside):
    """already-normalised fp32 rows.  Rows come in planted pairs (2m, 2m + 1), x_{2m+1} = x_{2m} + noise, so that every nearest
    neighbour is decided by a wide margin; the rows of a group are then made bit-identical, a `beside` row is put next to a group,
    and the pair partner of every row moved this way is planted next to it again."""
    g = gen(B, D, len(groups), 7)
    x = F.normalize(torch.randn(B, D, generator=g, dtype=F64), dim=-1)
    noise = torch.randn(B, D, generator=g, dtype=F64) / math.sqrt(D)
    for m in range(1, B, 2):
        x[m] = x[m - 1] + 0.3 * noise[m]
    moved, bases = [], [grp[0] for grp in groups]
    for grp in groups:
        for j in grp[1:]:
            x[j] = x[grp[0]]
            moved.append(j)
    for q, near in beside:
        x[q] = x[near] + 0.1 * noise[q]
        moved.append(q)
    for j in moved:
        p = j ^ 1
        if p < B and p not in moved and p not in bases:
            x[p] = x[j] + 0.3 * noise[p]
    x = F.normalize(x, dim=-1).to(F32)
    for grp in groups:
        for j in grp[1:]:
            x[j] = x[grp[0]]
    return x


def koleo_gap(xn):
    """per row: (float64 gap between the best dot product and the best one of a row that is not bit-identical to the best row, index
    of the first best row).  Identical rows give identical fp32 dot products whatever the order of the sum, so a tie among them is
    exact on the device too and the first index has to win."""
    xd = xn.to(F64)
    dots = xd @ xd.T
    dots.fill_diagonal_(-float("inf"))
    best = dots.argmax(1)
    same = (xn[best].unsqueeze(1) == xn.unsqueeze(0)).all(-1)         # [i, j]: row j is identical to row best[i]
    rest = dots.masked_fill(same, -float("inf"))
    gap = dots.max(1).values - rest.max(1).values                    # inf when every other row is identical to the best
    first = torch.where(same & torch.isfinite(dots), torch.arange(xn.shape[0]).expand_as(dots), xn.shape[0]).min(1).values
    return gap, first


def koleo_ref(xn, weight, eps=KOLEO_EPS, prefill=0.0, nn=None, minus_g=True):
    """DINOv2 KoLeoLoss on rows that are already normalised.  nn comes from oracle/loss_oracle.py (its renormalisation in float64 scales
    row i by 1 + O(2^-24), which moves no decision that koleo_gap accepts); the loss and the gradient with respect to the rows the
    kernel gets, with the neighbour held fixed:
        df = x_i - x_nn + 1e-8,  dist = |df|,  loss = -w sum_i log(dist + eps),  g_i = -w df / (dist (dist + eps)),
        d_xn[i] += g_i,  d_xn[nn_i] -= g_i
    -> dict(nn, loss, loss_bar, d_xn, d_xn_bar)"""
    B, D = xn.shape
    xd = xn.to(F64)
    if nn is None:
        nn = LO.koleo_loss(xd, eps)[1]
    w, e, pd = f32(weight), f32(eps), f32(1e-8)
    diff = xd - xd[nn]
    df = diff + pd
    s = (df * df).sum(1, keepdim=True)
    dist = s.sqrt()
    terms = -w * torch.log(dist + e).view(-1)
    c = -w / (dist * (dist + e))
    gi = c * df
    d_xn = gi.clone()
    if minus_g:
        d_xn.index_add_(0, nn, -gi)
    # errors.  df = fl(fl(x_i - x_nn) + 1e-8): U (|x_i - x_nn| + |df|).  s: ceil(D / 256) + 6 + 4 + 1 roundings and the errors of df;
    # dist relatively rho = ds / (2 s) + 2 U.  log(dist + eps): rho + U for the argument, 2 U |log| + 2 U for __logf; the product by w.
    ddf = U * (diff.abs() + df.abs())
    ds = U * (cdiv(D, 256) + 11) * s + (2 * df.abs() * ddf).sum(1, keepdim=True)
    rho = ds / (2 * s) + 2 * U
    dterm = abs(w) * (rho.view(-1) + 3 * U + 2 * U * torch.log(dist + e).abs().view(-1)) + U * terms.abs()
    loss_bar = dterm.sum() + B * U * (abs(prefill) + terms.abs().sum())
    # g = c df, c = -w / (dist (dist + eps)): 2 rho + 6 U relatively (product, division, an ulp), and the error of df
    dgi = gi.abs() * (2 * rho + 7 * U) + c.abs() * ddf
    contrib = 1.0 + torch.bincount(nn, minlength=B).to(F64).view(-1, 1)
    gabs, gerr = gi.abs().clone(), dgi.clone()
    gabs.index_add_(0, nn, gi.abs())
    gerr.index_add_(0, nn, dgi)
    return dict(nn=nn, loss=terms.sum(), loss_bar=loss_bar, d_xn=d_xn, d_xn_bar=gerr + contrib * U * (abs(prefill) + gabs), dist=dist)


# ------------------------------------------------------------------------------------------------------- Sinkhorn-Knopp
SK_T = (1, 63, 64, 65, 130)
SK_K = (8, 2040, 2056, 4096)
SK_CASES = tuple((T, K) for T in SK_T for K in SK_K) + ((130, 65536),)
SK_PAD = 3
SK_INV_TEMP = 1.0 / 0.07
SK_LOGIT_BOUND = 1.7       # |z| <= 24.3: the kernels shift by ONE maximum over all rows, so e^(z - shift) needs a range below 87
SK_HOSTILE = 60.0


def sk_case(T, K, pad=SK_PAD):
    """bf16 logits [T + pad, K]: T valid rows bounded by SK_LOGIT_BOUND (the head's logits are scaled cosines), then `pad` rows
    SK_HOSTILE above the valid maximum, which overflow every exponential they enter"""
    g = gen(T, K, 8)
    valid = (0.8 * torch.randn(T, K, generator=g)).clamp(-SK_LOGIT_BOUND, SK_LOGIT_BOUND).to(BF)
    hostile = (valid.float().max() + SK_HOSTILE + torch.rand(pad, K, generator=g)).to(BF)
    return torch.cat([valid, hostile], 0)


def sinkhorn_ref(logits, inv_temp, n_rows, n_iter=3):
    """oracle/loss_oracle.py sinkhorn_knopp on the first n_rows rows, [n_rows, K] float64.  The result does not depend on the sample
    count: a uniform factor on u leaves after the last column normalisation."""
    return LO.sinkhorn_knopp(logits[:n_rows].to(F64) * f32(inv_temp), 1.0, n_iter)


def sinkhorn_uv_ref(logits, inv_temp, n_rows, count, n_iter=3, rows_in_sums=None):
    """the factorised form the kernels run, in float64: Q = E u v count with E = exp(z - max z),
    v[k] = 1 / (K sum_t E[t, k] u[t]),  u[t] = 1 / (count sum_k E[t, k] v[k]),  starting from u = 1.
    -> (probs [n_rows, K], u [n_rows]); u does not depend on the shift and is where `count` shows.
    rows_in_sums: rows that enter the prototype sums (default n_rows)"""
    m = n_rows if rows_in_sums is None else rows_in_sums
    z = logits[:max(m, n_rows)].to(F64) * f32(inv_temp)
    E = torch.exp(z - z[:n_rows].max())
    K = z.shape[1]
    u = torch.ones(z.shape[0], dtype=F64)
    for _ in range(n_iter):
        v = 1.0 / (K * (E[:m] * u[:m, None]).sum(0))
        u = 1.0 / (count * (E * v).sum(1))
    return (E * u[:, None] * v * count)[:n_rows], u[:n_rows]


def sinkhorn_rel(logits, inv_temp, n_rows, n_iter=3):
    """relative fp32 error of u, of v and of E u v count.  An exponential: z = fl(l it) and x = fl(z - shift) give U (Z + X), then
    (X + 2) U.  A prototype sum: up to 64 rows in sequence in a row block, one atomic per row block, one more sum between ranks.  A
    sample sum: 8 ceil(K / 2048) + 6 + 4.  Each reciprocal: a product, a division.  The errors of u and v carry through."""
    z = logits[:n_rows].to(F64) * f32(inv_temp)
    Z, X = float(z.abs().max()), float(z.max() - z.min())
    K = z.shape[1]
    e_exp = U * (Z + 2 * X + 2)
    n_col = min(n_rows, 64) + cdiv(n_rows, 64) + 1
    n_row = 8 * cdiv(K, 2048) + 10
    eu = 0.0
    for _ in range(n_iter):
        ev = eu + e_exp + U * (n_col + 1) + 3 * U
        eu = ev + e_exp + U * (n_row + 1) + 3 * U
    return eu, eu + ev + e_exp + 3 * U


def sinkhorn_probs_bar(ref, rel):
    return BF_HALF_ULP * ref.abs() + rel * ref.abs() + FLUSH


# ------------------------------------------------------------------------------------------------------- colsum_bf16_rows
COLSUM_RMAX = 300
COLSUM_ROWS = (0, 1, 255, 256, 257, 300)
COLSUM_C = (8, 72)
COLSUM_BEYOND = 1e4
COLSUM_PREFILL = -2.5


def colsum_case(n_rows, C):
    """bf16 [R_max, C + 8] (the row stride is wider than the C columns summed); every row from n_rows on holds 1e4"""
    g = gen(n_rows, C, 9)
    x = torch.randn(COLSUM_RMAX, C + 8, generator=g)
    x[n_rows:] = COLSUM_BEYOND
    return x.to(BF)


def colsum_rows_ref(x, n_rows, C):
    xd = x[:n_rows, :C].to(F64)
    return xd.sum(0), xd.abs().sum(0)


def colsum_bar(sumabs, prefill, R_max=COLSUM_RMAX):
    """a thread adds 8 rows, a column's 32 partials are added in sequence, one atomic per block of 256 rows onto the prefill"""
    return U * (8 + 32 + cdiv(R_max, 256) + 1) * (abs(prefill) + sumabs)


# ------------------------------------------------------------------------------------------------------- token rows
#               T     D     rows of the source   indices
TOKEN_CASES = ((6, 8, 9, "mixed"), (5, 8, 9, "none"), (4097, 2048, 4100, "mixed"))


def token_case(T, D, n_src, kind):
    """bf16 source [n_src, D] (NaN and -0.0 among the values: rows are moved as bits) and unique indices int32 [T], -1: no row"""
    g = gen(T, D, 10)
    src = torch.randn(n_src, D, generator=g).to(BF)
    idx = torch.randperm(n_src, generator=g)[:T].to(I32)
    src[idx[0], 0], src[idx[2], D - 1] = float("nan"), -0.0
    if kind == "none":
        idx[:] = -1
    else:
        idx[1::3] = -1
    return src, idx


def gather_token_rows_ref(src, idx):
    """dst[t] = src[idx[t]], or zeros where idx[t] < 0"""
    out = src[idx.clamp_min(0).long()].clone()
    out[idx < 0] = 0
    return out


def scatter_token_rows_ref(d_dst, idx, d_src):
    """d_src[idx[t]] = d_dst[t] where idx[t] >= 0; the other rows of d_src stay"""
    out = d_src.clone()
    out[idx[idx >= 0].long()] = d_dst[idx >= 0]
    return out


def bits(t):
    return t.contiguous().view(torch.int16)
