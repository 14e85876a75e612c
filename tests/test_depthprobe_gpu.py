"""GPU: the depth-probe kernels (csrc/depthprobe.hip: vtp_depth_pix / vtp_depth_dlogits / vtp_depth_sgd, exact fp32 with fp64
statistics) and vtp_amd.DepthProbe against fp64 (tests/depth_ref.py, itself pinned to torch's CPU ops by
tests/test_depthprobe_host.py).

Bounds.  gamma_n = n u / (1 - n u), u = 2^-24, bounds a chain of n fp32 roundings in any order.  Primed letters are what the kernel
holds, plain ones the fp64 reference; every bound is formed from the reference alone.

Logits (tests/test_segprobe_gpu.py): bz(p, c) = up(gamma_{K+1} (|X| |W|^T + |b|))(p, c) + gamma_8 up(|Z|)(p, c), sbz(p) = sum_c bz.

dhat.  max(., 0) is 1-Lipschitz, so |a'_c - a_c| <= bz before a'_c rounds, and with perturbed a the quotient moves by exactly
sum_c da_c (e_c - dhat) / S', S' >= S - sbz.  Roundings: a_c rounds once and 0.1f is within u of 0.1 (2), e_c is four roundings of
positive terms (4), the fmaf chain of T and the sum of S are C each over positive terms, the division is 1: relative gamma_{2C+9},
stated as gamma_{2C+10}:
    bd(p) = sum_c bz |e_c - dhat| / (S - sbz) + gamma_{2C+10} dhat,        bS(p) = sbz + gamma_{C+2} S.

G.  g' = fl(logf(d') - logf(gt)) with logf within one ulp (2 u relative):
    bg(p) = bd / (dhat - bd) + gamma_4 (|log dhat| + |log gt|) + gamma_2 |g|.
The fp64 sums add nothing visible: bm1 = mean bg, and with dev = g - lam m1, L'^2 - L^2 = (2/n) sum dev dg + (1/n) sum dg^2 - lam dm1^2,
|L' - L| = |L'^2 - L^2| / (L' + L):
    bL = ((2/n) sum |dev| bg + (1/n) sum bg^2 + lam bm1^2) / L.
The numerator nu = g - lam m1 is fl(g' - fl(lam m1')):  bnu = (bg + lam bm1 + u |lam m1|) (1 + u) + u |nu|.
r = 1 / (dhat S) is two roundings on d', S';  1 / (n L) is one on L'.  With
    R = (1 + bd / (dhat - bd)) (1 + bS / (S - bS)) (1 + bL / (L - bL)) (1 + gamma_5)
the factor q = nu r / (n L), two more products, obeys  bq = bnu |r| / (n L) R + |q| (R - 1).
delta = e_c - dhat is one rounding on e'_c (within gamma_4 e_c) and d':  bdelta = (gamma_4 e_c + bd) (1 + u) + u |delta|, and the
product t = q delta rounds once:
    bt(p, c) = (|q| + bq) (|delta| + bdelta) (1 + gamma_2) - |q| |delta|.
The pixel's weight is the product of two fp32 tap weights, each off the fp64 one by at most gamma_3 times the axis length (src is
two roundings of a number below it, the weight one more), the product rounds once: bw = gamma_3 (h + w) + u, and a weight the
reference has at 0 can be up to bw in the kernel for the pixels next to the cell's support.  The raster-order fmaf chain over at
most Hl Wl pixels adds gamma_{Hl Wl + 1}.  With on(p, c) = [z_p[c] > 0 or the pair is near (below)]:
    bG(cell, c) = sum_p w_p on bt + bw sum_{p next to the support} on (|t| + bt) + gamma_{Hl Wl + 1} sum_p w_p on (|t| + bt).

The ReLU.  A valid (pixel, bin) pair is NEAR when |z_p[c]| <= bz(p, c): the kernel may hold the other sign and then adds, or drops,
the pair's whole term.  slack(cell, c) = sum over near pairs of w_p |q_p (e_c - dhat_p)|, and the cell pass must satisfy
|G' - G| <= bG + slack elementwise, 1e-5 relative Frobenius over the elements whose slack is 0, with near pairs at most 0.1 % of the
valid pairs and elements with non-zero slack at most 10 % of the elements -- so the exclusion cannot hide a failure.

1e-5 (relative; Frobenius for tensors) is the project's bar for fp32 arithmetic against fp64 (tests/test_losses_gpu.py)."""
import functools
import math
import os

import pytest
import torch

import depth_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
NCASE = len(R.CASES)
LO, HI, LAM = R.MIN_DEPTH, R.MAX_DEPTH, R.LAM


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _sliced(x, pad=8, off=4):
    """x on the GPU as a column slice (offset `off`, row stride K + pad) of a wider NaN-poisoned matrix"""
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=F32)
    wide[:, off:off + x.shape[1]] = x
    return wide.to(DEV)[:, off:off + x.shape[1]]


def _relF(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _dilate(A):
    """bool [out, in]: the support of a tap matrix, one cell wider on both sides"""
    s = A > 0
    d = s.clone()
    d[:, 1:] |= s[:, :-1]
    d[:, :-1] |= s[:, 1:]
    return d.to(F64)


def _bounds(r, bz, h, w):
    """bd [B, Hl, Wl], bG and slack [B, h, w, C] of the module docstring, and the near pairs, from one head's reference"""
    B, Hl, Wl, C = r["up"].shape
    e, S, dhat, ok = r["e"], r["S"], r["dhat"], r["valid"]
    delta = e - dhat[..., None]
    sbz = bz.sum(-1)
    bd = (bz * delta.abs()).sum(-1) / (S - sbz) + R.gamma(2 * C + 10) * dhat
    out = dict(bd=bd, near=(r["up"].abs() <= bz) & ok[..., None])
    n, L, lam = r["n"], r["loss"], LAM
    if n == 0 or L == 0:
        return out
    bS = sbz + R.gamma(C + 2) * S
    gt_log = torch.where(ok, r["gt"].double(), torch.ones((), dtype=F64)).log().abs()
    bg = (bd / (dhat - bd) + R.gamma(4) * (dhat.log().abs() + gt_log) + R.gamma(2) * r["g"].abs()) * ok
    assert bool((dhat > bd).all()) and bool((S > bS).all())
    bm1 = float(bg.sum() / n)
    nu = (r["g"] - lam * r["m1"]) * ok
    bL = float((2.0 * (nu.abs() * bg).sum() + (bg * bg).sum()) / n + lam * bm1 * bm1) / L
    assert L > bL
    bnu = (bg + lam * bm1 + U * abs(lam * r["m1"])) * (1 + U) + U * nu.abs()
    rr = 1.0 / (dhat * S)
    Rf = (1 + bd / (dhat - bd)) * (1 + bS / (S - bS)) * (1 + bL / (L - bL)) * (1 + R.gamma(5))
    q = r["q"]
    bq = (bnu * rr / (n * L) * Rf + q.abs() * (Rf - 1)) * ok
    bdelta = (R.gamma(4) * e + bd[..., None]) * (1 + U) + U * delta.abs()
    t = q[..., None] * delta
    bt = (q.abs() + bq)[..., None] * (delta.abs() + bdelta) * (1 + R.gamma(2)) - t.abs()
    on = ((r["up"] > 0) | out["near"]) & ok[..., None]
    Ay, Ax = R.tap_matrix(Hl, h), R.tap_matrix(Wl, w)
    bw = R.gamma(3) * (h + w) + U
    tot = (t.abs() + bt) * on
    out["bG"] = torch.einsum("yi,xj,byxc->bijc", Ay, Ax, bt * on + R.gamma(Hl * Wl + 1) * tot) \
        + bw * torch.einsum("yi,xj,byxc->bijc", _dilate(Ay), _dilate(Ax), tot)
    out["slack"] = torch.einsum("yi,xj,byxc->bijc", Ay, Ax, t.abs() * out["near"])
    return out


@functools.lru_cache(maxsize=None)
def _reference(i, H, variant):
    """the case's operands and, per head, the fp64 results and the bounds of the module docstring; computed once and never written"""
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, gt = R.make_case(i, H, variant)
    heads = []
    for hh in range(H):
        Wh, bh = W[hh * C:(hh + 1) * C].double(), b[hh * C:(hh + 1) * C].double()
        z = (X.double() @ Wh.T + bh).view(B, h, w, C)
        r = R.loss_and_grad(z, gt)
        r["gt"] = gt
        bz_cells = R.gamma(K + 1) * (X.double().abs() @ Wh.abs().T + bh.abs()).view(B, h, w, C)
        bz = R.upsample(bz_cells, Hl, Wl) + R.gamma(8) * R.upsample(z.abs(), Hl, Wl)
        bo = _bounds(r, bz, h, w)
        keep = dict(dhat=r["dhat"], loss=r["loss"], n=r["n"], G=r["G"], valid=r["valid"], n_near=int(bo["near"].sum()), **bo)
        del keep["near"]
        heads.append(keep)
    return X, W, b, gt, heads


def _pixel_pass(i, H, variant, mode="train"):
    """low-resolution logits from vtp_probe_logits (NaN columns past H C), then vtp_depth_pix on poisoned outputs; mode "train"
    (aux, no counters), "eval" (counters, no aux) or "both"."""
    from vtp_amd import ops
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, gt, _ = _reference(i, H, variant)
    M, N = B * h * w, H * C
    z = torch.full((M, N + 3), float("nan"), device=DEV, dtype=F32)
    ops.probe_logits(_sliced(X), W.to(DEV), b.to(DEV), z, M, N, K)
    nbytes, abytes = ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, H, C), ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, H, C, aux=True)
    ws = torch.full((nbytes + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    aux = torch.full((abytes + 64,), 0xA5, device=DEV, dtype=torch.uint8) if mode != "eval" else None
    out = dict(z=z, gt=gt.to(DEV), loss=torch.full((H,), float("nan"), device=DEV), stats=torch.full((H, 4), float("nan"), device=DEV, dtype=F64),
               dhat=torch.full((H, B, Hl, Wl), float("nan"), device=DEV), aux=None if aux is None else aux[:abytes],
               counts=torch.full((H, 4), 3, device=DEV, dtype=torch.int64) if mode != "train" else None,
               sums=torch.full((H, 6), 3.0, device=DEV, dtype=F64) if mode != "train" else None)
    ops.depth_pix(z, out["gt"], (h, w), H, C, LO, HI, LAM, dhat=out["dhat"], aux=out["aux"], loss=out["loss"], stats=out["stats"],
                  workspace=ws[:nbytes], eval_counts=out["counts"], eval_sums=out["sums"])
    assert bool((ws[nbytes:] == 0xA5).all()), "wrote past the workspace"
    assert aux is None or bool((aux[abytes:] == 0xA5).all()), "wrote past the aux plane"
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. pixel pass
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("i", range(NCASE))
def test_pixel_pass_depth_loss_and_counters(i, H):
    _gpu()
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, gt, heads = _reference(i, H, None)
    o = _pixel_pass(i, H, None, "both")
    assert not bool(o["dhat"].isnan().any()), "dhat is written for every pixel"
    for hh, r in enumerate(heads):
        got = o["dhat"][hh].cpu().double()
        err = (got - r["dhat"]).abs()
        print(f"DEPTH-PIX case {i} H={H} head {hh}: dhat max err/bound {float((err / r['bd']).max()):.3f}")
        assert bool((err <= r["bd"]).all())
        assert bool((got >= LO).all()) and bool((got <= HI).all())
        rel = abs(float(o["loss"][hh]) - r["loss"]) / r["loss"]
        print(f"DEPTH-PIX case {i} H={H} head {hh}: loss rel err {rel:.2e}")
        assert rel <= 1e-5
        n, m1, m2, L = o["stats"][hh].tolist()
        assert n == r["n"] and float(torch.tensor(L, dtype=F32)) == float(o["loss"][hh])
        assert L == pytest.approx(math.sqrt(max(m2 - LAM * m1 * m1, 0.0)), rel=1e-12)
        # the counters hold what the formulas give on the kernel's own fp32 dhat: counts exactly, fp64 sums to fp64 accuracy but
        # for g, which the kernel takes from logf (one ulp of each logarithm per pixel)
        counts, sums = R.counters(got, gt)
        assert (o["counts"][hh].cpu() - 3).tolist() == counts.tolist() and int(counts[0]) == r["n"]
        gs = o["sums"][hh].cpu() - 3.0
        ok = r["valid"]
        blog = R.gamma(6) * float((got[ok].log().abs() + gt.double()[ok].log().abs()).sum())
        assert abs(float(gs[0] - sums[0])) <= blog and abs(float(gs[5] - sums[5])) <= blog
        assert abs(float(gs[1] - sums[1])) <= 2.0 * blog * float((got[ok].log() - gt.double()[ok].log()).abs().max()) + 1e-12 * float(sums[1])
        for k in (2, 3, 4):
            assert float(gs[k]) == pytest.approx(float(sums[k]), rel=1e-12, abs=1e-12), k
    # the training call (aux, no counters) and the evaluation call (counters, no aux): the same loss and dhat bits
    for mode in ("train", "eval"):
        o2 = _pixel_pass(i, H, None, mode)
        assert torch.equal(o2["loss"], o["loss"]) and torch.equal(o2["stats"], o["stats"]) and torch.equal(o2["dhat"], o["dhat"])
    assert torch.equal(o2["counts"], o["counts"]) and torch.equal(o2["sums"], o["sums"])


@pytest.mark.parametrize("variant", ["nan", "inf", "far"])
@pytest.mark.parametrize("i", [0, 2, 6])
def test_pixel_pass_skips_a_planted_label(i, variant):
    _gpu()
    H = 1
    r, plain = _reference(i, H, variant)[4][0], _reference(i, H, None)[4][0]
    o = _pixel_pass(i, H, variant, "both")
    assert r["n"] == plain["n"] - 1 and o["stats"][0, 0].item() == r["n"] and int(o["counts"][0, 0]) - 3 == r["n"]
    assert abs(float(o["loss"][0]) - r["loss"]) <= 1e-5 * r["loss"] and bool(o["sums"].isfinite().all())
    assert bool(((o["dhat"][0].cpu().double() - r["dhat"]).abs() <= r["bd"]).all())


@pytest.mark.parametrize("i", range(NCASE))
def test_pixel_pass_without_a_valid_pixel(i):
    _gpu()
    H = 3
    o = _pixel_pass(i, H, "all_invalid", "both")
    assert o["loss"].tolist() == [0.0] * H and o["stats"].tolist() == [[0.0] * 4] * H
    assert bool((o["counts"] == 3).all()) and bool((o["sums"] == 3.0).all()), "counters untouched"
    for hh, r in enumerate(_reference(i, H, "all_invalid")[4]):  # dhat is still every pixel's
        assert bool(((o["dhat"][hh].cpu().double() - r["dhat"]).abs() <= r["bd"]).all())


def test_prediction_is_the_depth_of_the_pixel_pass():
    _gpu()
    from vtp_amd import ops
    i, H = 2, 3
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    o = _pixel_pass(i, H, None, "train")
    d = torch.full((H, B, Hl, Wl), float("nan"), device=DEV)
    ops.depth_pix(o["z"], None, (h, w), H, C, LO, HI, LAM, out_hw=(Hl, Wl), dhat=d)
    assert torch.equal(d, o["dhat"])


# ---------------------------------------------------------------------------------------------------------------- 2. cell pass
def _cell_pass(i, H, variant):
    from vtp_amd import ops
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    o = _pixel_pass(i, H, variant, "train")
    G = torch.full((B * h * w, H * C + 5), float("nan"), device=DEV, dtype=F32)
    ops.depth_dlogits(o["z"], (B, Hl, Wl), (h, w), H, C, LO, HI, LAM, o["aux"], o["stats"], G)
    assert bool(G[:, H * C:].isnan().all()), "wrote past column H * C"
    return o, G[:, :H * C]


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("i", range(NCASE))
def test_cell_pass_gradient(i, H):
    """G against fp64 by the rule of the module docstring: elementwise within bG + slack, 1e-5 relative Frobenius over the elements
    without slack, exact 0 on cells no pixel touches; and the exclusion is small: near pairs at most 0.1 % of the valid pairs,
    elements with slack at most 10 %.  (The reference alone, CPU: at most 3.2e-4 of the pairs and 4.3 % of the elements, worst at
    cases 2 and 5, none at the four small cases; the smallest |z| met was 6.5e-9.)"""
    _gpu()
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, gt, heads = _reference(i, H, None)
    _, G = _cell_pass(i, H, None)
    Ay, Ax = R.tap_matrix(Hl, h), R.tap_matrix(Wl, w)
    touched = (Ay.sum(0) > 0)[:, None] & (Ax.sum(0) > 0)[None, :]
    if i == 6:
        assert int((~touched).sum()) > 0
    for hh, r in enumerate(heads):
        g = G[:, hh * C:(hh + 1) * C].cpu().view(B, h, w, C).double()
        assert bool((g[:, ~touched] == 0).all()), "a cell without support must be exactly 0"
        free = r["slack"] == 0
        n_slack, pairs = int((~free).sum()), r["n"] * C
        print(f"DEPTH-DL case {i} H={H} head {hh}: {r['n_near']} near pairs of {pairs} ({r['n_near'] / pairs:.1e}), "
              f"{n_slack} of {free.numel()} elements with slack ({n_slack / free.numel():.1%})")
        assert r["n_near"] <= 1e-3 * pairs and n_slack <= 0.10 * free.numel()
        err = (g - r["G"]).abs()
        print(f"DEPTH-DL case {i} H={H} head {hh}: max err/(bG + slack) {float((err / (r['bG'] + r['slack']).clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= r["bG"] + r["slack"]).all())
        e = float((err * free).norm() / ((r["G"] * free).norm() + 1e-300))
        print(f"DEPTH-DL case {i} H={H} head {hh}: G relF {e:.2e} over the elements without slack")
        assert e <= 1e-5


@pytest.mark.parametrize("i", [1, 3, 6])
def test_cell_pass_without_a_valid_pixel(i):
    _gpu()
    _, G = _cell_pass(i, 3, "all_invalid")
    assert bool((G == 0).all()), "no valid pixel: G is 0 everywhere, no NaN from 1 / 0 or 0 / 0"


def test_cell_pass_with_a_zero_loss():
    """one valid pixel: g = m1, L = sqrt(max((1 - lam) g^2, 0)) > 0 unless g = 0; with lam = 1 the loss is exactly 0 and so is G"""
    _gpu()
    from vtp_amd import ops
    i, H = 3, 1
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    o = _pixel_pass(i, H, None, "train")
    gt = torch.zeros(B, Hl, Wl, device=DEV)
    gt[1, 2, 1] = 3.0
    nb = ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, H, C)
    ws = torch.empty(nb, device=DEV, dtype=torch.uint8)
    ops.depth_pix(o["z"], gt, (h, w), H, C, LO, HI, 1.0, aux=o["aux"], loss=o["loss"], stats=o["stats"], workspace=ws)
    assert o["loss"].tolist() == [0.0] and o["stats"][0, 0].item() == 1.0
    G = torch.full((B * h * w, C), float("nan"), device=DEV)
    ops.depth_dlogits(o["z"], (B, Hl, Wl), (h, w), H, C, LO, HI, 1.0, o["aux"], o["stats"], G)
    assert bool((G == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 3. weight step
def _sgd_operands(M, H, C, K, seed):
    N = H * C
    g = torch.Generator().manual_seed(seed)
    Gm, X = 0.1 * torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    state = [0.05 * torch.randn(N, K, generator=g), 0.05 * torch.randn(N, generator=g),
             0.02 * torch.randn(N, K, generator=g), 0.02 * torch.randn(N, generator=g)]  # W, bias, mW, mb
    lr = torch.tensor([0.1 * (hh + 1) for hh in range(H)], dtype=F32)
    return Gm, X, state, lr


@pytest.mark.parametrize("C", [2, 21, 150])
def test_weight_step_has_the_bits_of_seg_sgd(C):
    _gpu()
    from vtp_amd import ops
    s = ops.seg_sgd_slice()
    for M, H, K in ((3, 1, 40), (s + 1, 3, 132)):
        Gm, X, state, lr = _sgd_operands(M, H, C, K, 3000 + C + M)
        Gd, Xd, lrd = Gm.to(DEV), _sliced(X), lr.to(DEV)
        seg, dep = [t.to(DEV) for t in state], [t.to(DEV) for t in state]
        assert ops.depth_sgd_workspace_bytes(M, H * C, K) == ops.seg_sgd_workspace_bytes(M, H * C, K)
        ws = torch.empty(ops.seg_sgd_workspace_bytes(M, H * C, K), device=DEV, dtype=torch.uint8)
        ops.seg_sgd(*seg, Gd, Xd, lrd, M, H, C, K, 0.9, ws)
        ops.depth_sgd(*dep, Gd, Xd, lrd, M, H, C, K, 0.9, ws)
        for name, a, b_, t0 in zip(("W", "bias", "mW", "mb"), dep, seg, state):
            assert not torch.equal(a.cpu(), t0), (name, "the step changed nothing")
            assert torch.equal(a, b_), (name, M, H, C, K)


@pytest.mark.parametrize("C", [256, 257])
def test_weight_step_within_the_sliced_chain_bound(C):
    """vtp_depth_sgd past vtp_seg_sgd's 255 outputs, by the bound of tests/test_segprobe_gpu.py: dW[n, k] is a k-ordered fmaf chain
    per slice and the S slices are added in order, |dW - dW_ref| <= gamma_{M+S+3} (|G|^T |X|) =: bd; m = fmaf(momentum, m0, dW):
    |m - m_ref| <= bd + 2 u (|m_ref| + bd) =: bm; W = fmaf(-lr, m, W0): |W - W_ref| <= lr bm + 2 u (|W_ref| + lr bm)."""
    _gpu()
    from vtp_amd import ops
    s = ops.seg_sgd_slice()
    mom = float(torch.tensor(0.9, dtype=F32))
    for M, H, K in ((s - 1, 1, 40), (s, 2, 40), (s + 1, 1, 132), (2 * s + 5, 1, 40)):
        N, S = H * C, -(-M // s)
        Gm, X, (w0, b0, m0, mb0), lr = _sgd_operands(M, H, C, K, 4000 + C + M)
        lr_row = lr.double().repeat_interleave(C)
        Gd = torch.full((M, N + 5), float("nan"), dtype=F32)
        Gd[:, :N] = Gm
        Gd = Gd.to(DEV)[:, :N]

        def guarded(t):  # two rows (entries) of NaN after the tensor proper
            full = torch.full((N + 2, *t.shape[1:]), float("nan"), dtype=F32)
            full[:N] = t
            return full.to(DEV)

        Wd, bd_, mWd, mbd = guarded(w0), guarded(b0), guarded(m0), guarded(mb0)
        nbytes = ops.depth_sgd_workspace_bytes(M, N, K)
        ws = torch.full((nbytes + 64,), 0xA5, device=DEV, dtype=torch.uint8)
        ops.depth_sgd(Wd[:N], bd_[:N], mWd[:N], mbd[:N], Gd, _sliced(X), lr.to(DEV), M, H, C, K, mom, ws[:nbytes])
        assert bool((ws[nbytes:] == 0xA5).all()), "wrote past the workspace"
        for t in (Wd, bd_, mWd, mbd):
            assert bool(t[N:].isnan().all()) and not bool(t[:N].isnan().any()), "wrote past N, or read past K"
        gam = R.gamma(M + S + 3)
        for got_m, got_p, mm0, p0, d_ref, d_abs, r in (
                (mWd[:N], Wd[:N], m0, w0, Gm.double().T @ X.double(), Gm.double().abs().T @ X.double().abs(), lr_row[:, None]),
                (mbd[:N], bd_[:N], mb0, b0, Gm.double().sum(0), Gm.double().abs().sum(0), lr_row)):
            m_ref = mom * mm0.double() + d_ref
            p_ref = p0.double() - r * m_ref
            bm = gam * d_abs + 2 * U * (m_ref.abs() + gam * d_abs)
            bp = r * bm + 2 * U * (p_ref.abs() + r * bm)
            em, ep = (got_m.cpu().double() - m_ref).abs(), (got_p.cpu().double() - p_ref).abs()
            assert bool((em <= bm).all()) and bool((ep <= bp).all()), (M, N, K, float((em / bm).max()), float((ep / bp).max()))


# ---------------------------------------------------------------------------------------------------------------- 4. repeatability
def _probe(heads, C, D, seed=0, **kw):
    from vtp_amd import DepthProbe
    torch.manual_seed(seed)
    return DepthProbe(None, heads, n_bins=C, embed_dim=D, **kw)


def _batch(B, h, w, Hl, Wl, width, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * h * w, width, generator=g)
    y = LO + (HI - LO) * torch.rand(B, Hl, Wl, generator=g)
    y[torch.rand(B, Hl, Wl, generator=g) < 0.1] = 0.0
    return x.to(DEV), (h, w), y.to(DEV)


def _state(p):
    return [t.clone() for g in p.groups for t in (g.weight, g.bias, g.m_weight, g.m_bias)]


def _spread(p, factor=30.0):
    for g in p.groups:
        g.weight.mul_(factor)  # away from the all-equal bins of the 0.01 init


def test_kernels_repeat_bit_for_bit():
    _gpu()
    (o1, g1), (o2, g2) = _cell_pass(5, 3, None), _cell_pass(5, 3, None)
    assert torch.equal(o1["dhat"], o2["dhat"]) and torch.equal(o1["loss"], o2["loss"]) and torch.equal(o1["stats"], o2["stats"])
    assert torch.equal(o1["aux"], o2["aux"]) and torch.equal(g1, g2)


def test_a_step_repeats_bit_for_bit_and_chunks_of_heads_change_nothing():
    _gpu()
    B, h, w, Hl, Wl, C, D = 3, 4, 5, 40, 52, 70, 32
    heads = [("a", 1, 0.5), ("b", 1, 0.25), ("c", 1, 0.125)]
    runs = []
    for chunk in (None, None, 1, 2):
        p = _probe(heads, C, D, max_iter=10)
        _spread(p)
        p.head_chunk = chunk
        losses = [p.step_features(*_batch(B, h, w, Hl, Wl, D, 40 + s)) for s in range(2)]
        runs.append(losses + _state(p))
    assert not torch.equal(runs[0][0], runs[0][1])
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


def test_evaluation_does_not_depend_on_the_batch_split():
    _gpu()
    B, h, w, Hl, Wl, C, D = 3, 4, 5, 40, 52, 70, 32
    heads = [("a", 1, 0.5), ("b", 2, 0.25)]
    x, hw, y = _batch(B, h, w, Hl, Wl, 2 * D, 7)
    M1 = h * w
    splits = {"all": [slice(0, 3)], "1+rest": [slice(0, 1), slice(1, 3)], "one by one": [slice(0, 1), slice(1, 2), slice(2, 3)]}
    got = {}
    for name, parts in splits.items():
        p = _probe(heads, C, D)
        _spread(p)
        for s in parts:
            p.evaluate_features(x[s.start * M1:s.stop * M1], hw, y[s])
        got[name] = (p._counts.clone(), p._sums.clone(), p.metrics(), p.best())
    c0, s0, m0, b0 = got["all"]
    assert c0[:, 0].tolist() == [int((y > 0).sum())] * 2 and bool((s0[:, 1] > 0).all())
    for name in ("1+rest", "one by one"):
        c, s, m, b = got[name]
        assert torch.equal(c, c0) and torch.equal(s.view(torch.int64), s0.view(torch.int64)), name
        assert m == m0 and b == b0
    assert set(m0) == {"a", "b"} and b0[0] == min(m0, key=lambda k: m0[k]["rmse"])
    # the metrics are the formulas on the predicted depth
    d = p.predict_features(x, hw, (Hl, Wl))
    for j, k in enumerate(p.keys):
        want = R.metrics(*R.counters(d[j].cpu(), y.cpu()))
        for name, v in want.items():
            assert m0[k][name] == pytest.approx(v, rel=1e-5), (k, name)
    p.reset_eval()
    assert int(p._counts.sum()) == 0 and float(p._sums.abs().sum()) == 0.0
    with pytest.raises(RuntimeError, match="nothing evaluated"):
        p.metrics()


def test_predict_features_is_the_depth_of_the_pixel_pass():
    _gpu()
    from vtp_amd import ops
    B, h, w, Hl, Wl, C, D = 2, 3, 4, 24, 32, 70, 32
    p = _probe([("a", 1, 0.5), ("b", 2, 0.25), ("c", 1, 0.1)], C, D)
    _spread(p)
    x, hw, y = _batch(B, h, w, Hl, Wl, 2 * D, 11)
    d = p.predict_features(x, hw, (Hl, Wl))
    assert tuple(d.shape) == (3, B, Hl, Wl) and bool((d >= LO).all()) and bool((d <= HI).all())
    for g in p.groups:
        z = torch.empty(B * h * w, g.H * C, device=DEV)
        ops.probe_logits(x[:, g.col0:g.col0 + g.K], g.weight, g.bias, z, B * h * w, g.H * C, g.K)
        want = torch.empty(g.H, B, Hl, Wl, device=DEV)
        ws = torch.empty(ops.depth_pix_workspace_bytes(B, h, w, Hl, Wl, g.H, C), device=DEV, dtype=torch.uint8)
        ops.depth_pix(z, y, hw, g.H, C, LO, HI, LAM, dhat=want, loss=torch.empty(g.H, device=DEV),
                      stats=torch.empty(g.H, 4, device=DEV, dtype=F64), workspace=ws)
        assert torch.equal(d[g.off:g.off + g.H], want)
    assert not torch.equal(d[0], d[1])
    assert tuple(p.predict_features(x, hw, (5, 3)).shape) == (3, B, 5, 3)


def test_equal_heads_stay_bit_identical():
    _gpu()
    B, h, w, Hl, Wl, C, D = 2, 3, 4, 24, 32, 70, 32
    p = _probe([("a", 1, 0.3), ("b", 1, 0.3), ("c", 1, 0.1)], C, D)
    _spread(p)
    p.groups[0].weight[1].copy_(p.groups[0].weight[0])
    for s in range(3):
        losses = p.step_features(*_batch(B, h, w, Hl, Wl, D, 60 + s))
        assert float(losses[0]) == float(losses[1])
    g = p.groups[0]
    for t in (g.weight, g.bias, g.m_weight, g.m_bias):
        assert torch.equal(t[0], t[1]) and not torch.equal(t[0], t[2])


def test_the_constructor_and_the_inputs_refuse_what_the_kernels_would():
    _gpu()
    from vtp_amd import DepthProbe
    for kw, msg in ((dict(n_bins=1), "n_bins"), (dict(n_bins=1025), "n_bins"), (dict(min_depth=0.0), "min_depth"),
                    (dict(min_depth=2.0, max_depth=1.0), "min_depth"), (dict(max_iter=0), "max_iter"), (dict(embed_dim=6), "multiple of 4")):
        with pytest.raises(ValueError, match=msg):
            DepthProbe(None, [("a", 1, 0.1)], **{"embed_dim": 4, **kw})
    p = _probe([("a", 1, 0.1)], 16, 4)
    with pytest.raises(ValueError, match="floating-point depth"):
        p.step_features(torch.zeros(4, 4, device=DEV), (2, 2), torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="features must be"):
        p.evaluate_features(torch.zeros(4, 8, device=DEV), (2, 2), torch.ones(1, 8, 8, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- 5. memory
def test_a_step_allocates_a_fraction_of_the_upsampled_logits():
    """B = 2, 8 x 8 cells, 128 x 128 labels, 256 bins, H = 1: the [H, B, C, Hl, Wl] fp32 tensor torch would hold is 33.6 MB; one step
    may raise the peak by less than a sixteenth of it (its own arrays -- three aux planes of 131 KB, Z, G, the workspaces, among them
    the weight-gradient slice of 66 KB -- total well under 1 MB)"""
    _gpu()
    B, h, w, Hl, Wl, C, D = 2, 8, 8, 128, 128, 256, 64
    p = _probe([("a", 1, 0.1)], C, D)
    x, hw, y = _batch(B, h, w, Hl, Wl, D, 3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    p.step_features(x, hw, y)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"DEPTH-MEM: peak rise {rise / 1e6:.2f} MB of {B * C * Hl * Wl * 4 / 1e6:.1f} MB")
    assert rise < B * C * Hl * Wl * 4 / 16


# ---------------------------------------------------------------------------------------------------------------- 6. class level
TRAJ = dict(B=2, h=3, w=3, Hl=24, Wl=24, C=16, D=32, seed=90)  # a seed without a near pair (see the test)


def _near_pairs(r, x, W, b, K, h, w):
    """near pairs (module docstring) of one head's reference dict at weights W [C, K], b [C] and features x [M, K]"""
    B, Hl, Wl, C = r["up"].shape
    cells = R.gamma(K + 1) * (x.abs() @ W.abs().T + b.abs()).view(B, h, w, C)
    z = (x @ W.T + b).view(B, h, w, C)
    bz = R.upsample(cells, Hl, Wl) + R.gamma(8) * R.upsample(z.abs(), Hl, Wl)
    return int(((r["up"].abs() <= bz) & r["valid"][..., None]).sum())


def test_three_steps_follow_the_fp64_trajectory():
    """three steps of three heads in two groups against RefDepth, SegProbe's tolerances (1e-5 on every loss, 1e-5 relative Frobenius
    on the final weights).  A condition, checked on the reference at every step: no (pixel, bin) pair is near, so no ReLU can fall
    on the other side in fp32 and the fp64 trajectory is the one to follow."""
    _gpu()
    B, h, w, Hl, Wl, C, D = (TRAJ[k] for k in ("B", "h", "w", "Hl", "Wl", "C", "D"))
    heads = [("one_a", 1, 0.5), ("two", 2, 0.25), ("one_b", 1, 0.1)]
    p = _probe(heads, C, D, max_iter=10)
    _spread(p)
    assert p.keys == ["one_a", "one_b", "two"] and [g.K for g in p.groups] == [D, 2 * D]
    ref = R.RefDepth(heads, {k: (g.weight[j].cpu(), g.bias[j].cpu()) for g in p.groups for j, k in enumerate(g.keys)}, D, 0.9, 10)
    for s in range(3):
        x, hw, y = _batch(B, h, w, Hl, Wl, 2 * D, TRAJ["seed"] + s)
        if s == 1:
            y[0, 0, :4] = torch.tensor([float("nan"), float("inf"), -1.0, 10.5], device=DEV)  # none of them a measurement
        fwd = ref.forward(x.cpu(), hw, y)
        near = sum(_near_pairs(fwd[k], x.cpu().double()[:, (2 - n) * D:], ref.W[k], ref.b[k], n * D, h, w) for k, n, _ in heads)
        assert near == 0, f"step {s}: {near} near pairs in the reference: choose another seed"
        got = p.step_features(x, hw, y)
        want = ref.step(x.cpu(), hw, y)
        assert p.learning_rates(s)["two"] == pytest.approx(R.cosine_lr(0.25, s, 10), rel=1e-15)
        for j, k in enumerate(p.keys):
            assert float(got[j]) == pytest.approx(want[k]["loss"], rel=1e-5), (s, k)
    for g in p.groups:
        for j, k in enumerate(g.keys):
            eW, eb = _relF(g.weight[j], ref.W[k]), _relF(g.bias[j], ref.b[k])
            print(f"DEPTH-TRAJ {k}: weight relF {eW:.2e} bias relF {eb:.2e}")
            assert eW <= 1e-5 and eb <= 1e-5


def test_planted_problem_is_learned_and_checkpoints_continue_bit_for_bit():
    """labels produced by a hidden head of the same form: RefDepth's loss falls, and the GPU follows it (1e-3 on the loss after 20
    steps: ReLUs near 0 may fall on either side on the way, which the kernel tests bound and the trajectory test excludes)"""
    _gpu()
    B, h, w, Hl, Wl, C, D = 2, 4, 4, 32, 32, 16, 32
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * h * w, D, generator=g)
    hidden = (x.double() @ torch.randn(D, C, generator=g).double()).view(B, h, w, C)
    y = R.loss_and_grad(hidden, torch.ones(B, Hl, Wl))["dhat"].to(F32)  # the depth a linear head on these features can reach
    x, y = x.to(DEV), y.to(DEV)
    p = _probe([("a", 1, 0.5)], C, D)
    _spread(p)
    ref = R.RefDepth([("a", 1, 0.5)], {"a": (p.groups[0].weight[0].cpu(), p.groups[0].bias[0].cpu())}, D)
    p.evaluate_features(x, (h, w), y)
    rmse0 = p.metrics()["a"]["rmse"]
    p.reset_eval()
    losses, want = [], []
    for _ in range(20):
        losses.append(float(p.step_features(x, (h, w), y)[0]))
        want.append(ref.step(x.cpu(), (h, w), y)["a"]["loss"])
    p.evaluate_features(x, (h, w), y)
    m = p.metrics()["a"]
    print(f"DEPTH-PLANTED: loss {losses[0]:.4f} -> {losses[-1]:.4f} (fp64 {want[0]:.4f} -> {want[-1]:.4f}), rmse {rmse0:.3f} -> {m['rmse']:.3f}, "
          f"d1 {m['d1']:.3f}")
    assert want[-1] < 0.5 * want[0] and losses[-1] < 0.5 * losses[0]
    assert losses[0] == pytest.approx(want[0], rel=1e-5) and losses[-1] == pytest.approx(want[-1], rel=1e-3)
    assert m["valid"] == B * Hl * Wl and p.best() == ("a", m["rmse"])
    q = _probe([("a", 1, 0.5)], C, D, seed=9)
    q.load_state_dict({k: v.cpu() for k, v in p.state_dict().items()})
    assert q.steps == p.steps == 20
    for _ in range(2):
        assert torch.equal(p.step_features(x, (h, w), y), q.step_features(x, (h, w), y))
    assert all(torch.equal(a, b) for a, b in zip(_state(p), _state(q)))


def test_through_the_tiny_model(golden, golden_sd):
    _gpu()
    from oracle.ref_stubs import TINY
    from vtp_amd import DepthProbe, VTPConfig, VTPModel
    model = VTPModel(VTPConfig(**TINY))
    model.load_state_dict(golden_sd, strict=True)
    model = model.to(DEV).eval()
    D, C = TINY["vision_embed_dim"], 8
    images = golden["in.image"].to(DEV)
    B, _, Hi, Wi = images.shape
    h, w = Hi // 16, Wi // 16
    depth = (0.5 + 9.0 * torch.rand(B, Hi, Wi, generator=torch.Generator().manual_seed(0))).to(DEV)
    outs = model.get_intermediate_layers_feature(images, n=2, norm=True, return_class_token=True)
    for cls_concat in (False, True):
        p = DepthProbe(model, [("one", 1, 0.1), ("two", 2, 0.1)], n_bins=C, cls_concat=cls_concat)
        feats = p.features(images)
        if cls_concat:  # per block: the patch tokens, then the block's class token repeated for every one of them
            want = torch.cat([t for patch, cls_t in outs for t in (patch.reshape(-1, D), cls_t.repeat_interleave(h * w, dim=0))], dim=1)
        else:
            want = torch.cat([patch.reshape(-1, D) for patch, _ in outs], dim=1)
        assert tuple(feats.shape) == (B * h * w, 2 * p.Dc) and p.Dc == (2 * D if cls_concat else D)
        assert [g.K for g in p.groups] == [p.Dc, 2 * p.Dc] and [g.col0 for g in p.groups] == [p.Dc, 0]
        assert torch.equal(feats, want)
        loss = p.step(images, depth)
        ev = p.evaluate(images, depth[:, ::2, ::2].contiguous())  # evaluation at the labels' own size
        pred = p.predict(images, (Hi, Wi))
        assert loss.shape == ev.shape == (2,) and bool(loss.isfinite().all()) and bool(ev.isfinite().all())
        assert tuple(pred.shape) == (2, B, Hi, Wi) and bool((pred >= p.min_depth).all()) and bool((pred <= p.max_depth).all())
        m = p.metrics()
        assert m["one"]["valid"] == B * (Hi // 2) * (Wi // 2) and 0.0 <= m["one"]["d1"] <= m["one"]["d3"] <= 1.0
