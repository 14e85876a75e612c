"""tests/ssl_ref.py without a GPU: its references against independent torch code (F.softmax, F.cross_entropy, F.normalize, the weight_norm
parametrisation, float64 autograd for every gradient, oracle/loss_oracle.py), the proof that the bars of tests/test_ssl_kernels_gpu.py
discriminate -- deliberately wrong variants miss the GPU test's bar at the GPU test's own inputs -- and the conditions on the cases
that keep the GPU test from passing or failing by luck."""
import math

import pytest
import torch
import torch.nn.functional as F

import ssl_ref as R
from oracle import loss_oracle as LO

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def close(a, b, tol=1e-11):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


def misses(bad, ref, bar):
    return R.ratio(bad, ref, bar) > 1.0


# ------------------------------------------------------------------------------------------------------------ the yardstick itself
def test_ratio_looks_at_every_element():
    ref = torch.linspace(-1, 1, 4096, dtype=F64).view(64, 64)
    bar = 1e-6 * ref.abs() + 1e-9
    assert R.ratio(ref.clone(), ref, bar) == 0.0
    for i, j in ((0, 0), (63, 63), (17, 40)):
        bad = ref.clone()
        bad[i, j] += 2 * float(bar[i, j])
        assert 1.9 < R.ratio(bad, ref, bar) < 2.1
        bad[i, j] = float("nan")
        assert R.ratio(bad, ref, bar) == float("inf")
    assert R.ratio(torch.tensor([1.0]), torch.tensor([0.0]), torch.tensor([0.0])) == float("inf")    # a zero bar is met exactly


# ------------------------------------------------------------------------------------------------------------ softmax_center
def _softmax_variant(logits, center, inv_temp, kind):
    it = R.f32(inv_temp)
    l = logits.to(F64)
    c = torch.zeros((), dtype=F64) if center is None else center.to(F64)
    z = {"plus": (l + c) * it, "temp_first": l * it - c, "no_temp": l - c}.get(kind, (l - c) * it)
    e = torch.exp(z - z.amax(1, keepdim=True))
    K = l.shape[1]
    se = e[:, :K - K % 2048].sum(1, keepdim=True) if kind == "tail" else e.sum(1, keepdim=True)
    return e / se


def _softmax_mutants(K, with_center, hand):
    """the variants that change the operation at a case: none of the centre ones without a centre or with the constant centre of the
    hand-built rows (a softmax does not see a constant), the tail one only where K % 2048 columns exist"""
    return ["no_temp"] + (["plus", "temp_first"] if with_center and not hand else []) + (["tail"] if K % 2048 else [])


@pytest.mark.parametrize("K", R.SOFTMAX_K)
def test_softmax_ref_and_mutants(K):
    cases = [(R.softmax_case(K, T, wc), R.SOFTMAX_INV_TEMP, wc, False) for T in R.SOFTMAX_T for wc in (True, False)]
    cases += [(R.softmax_hand_case(K, wc), R.HAND_INV_TEMP, wc, True) for wc in (True, False)]
    for (logits, center), it, wc, hand in cases:
        ref, se, z = R.softmax_center_ref(logits, center, it)
        zz = (logits.double() - (center.double() if wc else 0.0)) * R.f32(it)
        assert close(ref, F.softmax(zz, dim=-1)) and bool((se >= 1.0).all())
        bar = R.softmax_bar(ref, z, K)
        assert misses(ref.to(BF).float() * (1 + 2.0 ** -6), ref, bar)          # two bf16 ulps off
        assert not misses(ref.to(BF), ref, bar)                              # the correctly rounded answer passes
        for kind in _softmax_mutants(K, wc, hand):
            assert misses(_softmax_variant(logits, center, it, kind), ref, bar), (K, wc, hand, kind)
        if hand:
            assert bool((ref[0] == ref[0, 0]).all()) and float(z.abs().max()) >= 100.0
            assert float(z.max()) > 88 and not bool(torch.isfinite(torch.exp(z.to(F32).max())))          # e^z overflows fp32: the maximum has to be subtracted
            assert float(z[1].max() - z[1].min()) == 8.0 * R.HAND_INV_TEMP


def test_softmax_cases_cover_the_dispatch():
    reg = [K for K in R.SOFTMAX_K if R.softmax_is_reg(K)]
    assert min(reg) == 8192 and max(reg) == 65536 and 8184 in R.SOFTMAX_K and 65544 in R.SOFTMAX_K
    assert any(K < 2048 - 512 for K in R.SOFTMAX_K)            # whole waves of row_lse without an element
    assert any(K % 8192 for K in reg) and any(K % 2048 for K in R.SOFTMAX_K if not R.softmax_is_reg(K))


# ------------------------------------------------------------------------------------------------------------ dino_ce
def _dino_variant(S, P, t0, t1, w, inv_temp, nt_one=False, drop_second=False, no_w_grad=False):
    """loss per row by F.cross_entropy with probability targets, dS by autograd; the wrong variants by the formulas"""
    it = R.f32(inv_temp)
    T, K = S.shape
    Sd = S.to(F64).requires_grad_(True)
    z = Sd * it
    loss = torch.zeros(T, dtype=F64)
    for r in range(T):
        if float(w[r]) == 0 or int(t0[r]) < 0:
            continue
        for t in ([int(t0[r])] if drop_second or int(t1[r]) < 0 else [int(t0[r]), int(t1[r])]):
            loss[r] = loss[r] + float(w[r]) * F.cross_entropy(z[r:r + 1], P[t:t + 1].to(F64), reduction="sum")
    (dS,) = torch.autograd.grad(loss.sum(), Sd)
    if nt_one or no_w_grad or drop_second:
        ref = R.dino_ce_ref(S, P, t0, t1, w, inv_temp)
        q = P.to(F64)[t0.clamp_min(0).long()] * ref["live"] if drop_second else ref["q"]
        nt = torch.ones_like(ref["nt"]) if nt_one else ref["nt"]
        wg = ref["live"] if no_w_grad else ref["w"]
        dS = wg * it * (nt * torch.exp(ref["lsm"]) - q)
    return loss.detach(), dS


@pytest.mark.parametrize("K", R.DINO_K)
def test_dino_ref_and_mutants(K):
    case = R.dino_case(K)
    # n_targets in the gradient stands for the sum of the targets: with target rows that sum to one exactly, the reference is autograd
    S, P, t0, t1, w = case
    P1 = P.double() / P.double().sum(1, keepdim=True)
    exact = R.dino_ce_ref(S, P1, t0, t1, w, R.DINO_INV_TEMP)
    loss, dS = _dino_variant(S, P1, t0, t1, w, R.DINO_INV_TEMP)
    assert close(exact["loss"], loss) and close(exact["dS"], dS, 1e-9)
    assert float((P.double().sum(1) - 1).abs().max()) < 2.0 ** -8          # the bf16 targets of the case: as far from one as rounding puts them
    ref = R.dino_ce_ref(*case, R.DINO_INV_TEMP)
    assert close(ref["loss"], _dino_variant(*case, R.DINO_INV_TEMP)[0])
    assert bool((ref["loss_abs"] >= ref["loss"].abs() - 1e-12).all())
    live = ref["live"].view(-1) > 0
    assert live.tolist() == [True, True, False, False, True, True]          # two targets, one, t0 = -1, w = 0, two, one
    assert not bool(ref["dS"][~live].any()) and not bool(ref["loss"][~live].any())
    row_bar, total_bar = R.dino_loss_bar(ref, K, R.DINO_PREFILL, len(live))
    ds_bar = R.dino_ds_bar(ref, K)
    for kw in (dict(nt_one=True), dict(drop_second=True), dict(no_w_grad=True)):
        bad_loss, bad_dS = _dino_variant(*case, R.DINO_INV_TEMP, **kw)
        assert misses(bad_dS, ref["dS"], ds_bar), kw
        if "drop_second" in kw:
            assert misses(bad_loss[live], ref["loss"][live], row_bar[live])
            assert misses(bad_loss.sum().view(1), ref["loss"].sum().view(1), total_bar.view(1))
    # `=` for `+=` on the accumulator
    assert misses(ref["loss"].sum().view(1), (R.DINO_PREFILL + ref["loss"].sum()).view(1), total_bar.view(1))


# ------------------------------------------------------------------------------------------------------------ center_ema
@pytest.mark.parametrize("K", R.EMA_K)
def test_center_ema_ref_and_mutant(K):
    center, colsum = R.ema_case(K)
    missed = 0
    for count in R.EMA_COUNTS:
        ref, sumabs = R.center_ema_ref(center, colsum, R.EMA_HOST_INV_COUNT, count, R.EMA_MOMENTUM)
        m = R.f32(R.EMA_MOMENTUM)
        ic = R.f32(R.EMA_HOST_INV_COUNT) if count is None else 1.0 / max(count, 1.0)
        assert close(ref, torch.lerp(colsum.double() * ic, center.double(), m))
        if count is not None:
            bad, _ = R.center_ema_ref(center, colsum, None, count, R.EMA_MOMENTUM, clamp=False)
            assert misses(bad, ref, R.ema_bar(sumabs)) == (count < 1.0)
            missed += count < 1.0
    assert missed == 2


# ------------------------------------------------------------------------------------------------------------ weight norm
@pytest.mark.parametrize("K,C", R.WN_CASES)
def test_weight_norm_refs_and_mutants(K, C):
    v, g, dW = R.wn_case(K, C)
    weff, inv, s = R.weight_norm_prep_ref(v, g)
    assert float(s.min()) >= 2.0 ** 10 * R.WN_MIN_SUMSQ and (K == 1 or float(s.min()) < 1e-30)     # a tiny row, squares still normal
    assert bool(torch.isfinite(weff.to(F32)).all())
    lin = torch.nn.utils.parametrizations.weight_norm(torch.nn.Linear(C, K, bias=False).double(), dim=0)
    with torch.no_grad():
        lin.parametrizations.weight.original0.copy_(g.double().view(K, 1))
        lin.parametrizations.weight.original1.copy_(v.double())
    assert close(weff, lin.weight.detach()) and close(inv, 1.0 / v.double().norm(dim=1))
    (lin.weight * dW.double()).sum().backward()
    ref = R.weight_norm_bwd_ref(dW, v, g, inv)
    assert close(ref["dv"], lin.parametrizations.weight.original1.grad, 1e-9)
    assert close(ref["dg"], lin.parametrizations.weight.original0.grad.view(-1), 1e-9)
    # at the GPU test's inputs: the fp32-rounded norms
    ref = R.weight_norm_bwd_ref(dW, v, g, inv.to(F32))
    dv_bar, dg_bar = R.wn_bwd_bars(ref, C, R.WN_PREFILL)
    bad = R.weight_norm_bwd_ref(dW, v, g, inv.to(F32), projection=False)
    assert misses(R.WN_PREFILL + bad["dv"], R.WN_PREFILL + ref["dv"], dv_bar)
    assert misses(ref["dv"], R.WN_PREFILL + ref["dv"], dv_bar) and misses(ref["dg"], R.WN_PREFILL + ref["dg"], dg_bar)   # `=` for `+=`
    assert misses(v.double() * inv.view(-1, 1), weff, R.wn_weff_bar(weff, C))          # the gain left out
    assert misses(1.0 / s, inv, R.wn_inv_bar(inv, C))                                  # the root left out


def test_weight_norm_cases_cover_the_paths():
    assert any(C <= 256 for _, C in R.WN_CASES) and any(C > 256 for _, C in R.WN_CASES)       # tiled and plain with weffT
    assert {K % 64 for K, C in R.WN_CASES if C <= 256} >= {0, 1, 63} and any(K > 64 for K, _ in R.WN_CASES)
    assert any(C % 64 for _, C in R.WN_CASES) and any(C > 64 for _, C in R.WN_CASES)         # more than one trip of the lane loop


# ------------------------------------------------------------------------------------------------------------ l2norm
@pytest.mark.parametrize("eps", R.L2_EPS)
@pytest.mark.parametrize("D", R.L2_D)
def test_l2norm_refs_and_mutants(D, eps):
    x, dy = R.l2_case(D)
    y, inv, s = R.l2norm_fwd_ref(x, eps)
    xr = x.double().requires_grad_(True)
    yt = F.normalize(xr, dim=-1, eps=R.f32(eps))
    assert close(y, yt.detach())
    assert not bool(y[1].any()) and float(inv[1]) == 1.0 / R.f32(eps)
    yt.backward(dy.double())
    ref = R.l2norm_bwd_ref(dy, y, inv)
    keep = [0, 2]
    assert close(ref["dx"][keep], xr.grad[keep], 1e-9)
    assert close(ref["dx"][1], dy[1].double() / R.f32(eps)) and bool(torch.isfinite(ref["dx"].to(F32)).all())
    # at the GPU test's inputs
    ref = R.l2norm_bwd_ref(dy, y.to(F32), inv.to(F32))
    if D > 1:
        assert misses(inv.view(-1, 1) * dy.double(), ref["dx"], R.l2_bwd_bar(ref, D))      # the projection left out
    else:
        assert misses(2 * ref["dx"] + inv.view(-1, 1) * dy.double(), ref["dx"], R.l2_bwd_bar(ref, D))
    assert misses(1.0 / s.clamp_min(R.f32(eps)), inv, R.l2_inv_bar(inv, D))                # the root left out
    assert misses(x.double() / (s.sqrt() + 1.0).view(-1, 1), y, R.l2_y_bar(y, D))


# ------------------------------------------------------------------------------------------------------------ CLIP
def _clip_autograd(img_l, txt_l, img_all, txt_all, ls, off, weight=0.5, label_offset=True):
    il, tl, ia, ta = (t.double().requires_grad_(True) for t in (img_l, txt_l, img_all, txt_all))
    l64 = torch.tensor(R.f32(ls), dtype=F64, requires_grad=True)
    Bl = il.shape[0]
    lab = torch.arange(Bl) + (off if label_offset else 0)
    w = R.f32(weight / Bl) if weight != 0.5 else R.f32(0.5 / Bl)
    loss = w * (F.cross_entropy(l64.exp() * il @ ta.T, lab, reduction="sum") + F.cross_entropy(l64.exp() * tl @ ia.T, lab, reduction="sum"))
    loss.backward()
    return dict(loss=loss.detach(), d_logit_scale=l64.grad, d_img_local=il.grad, d_txt_local=tl.grad, d_img_all=ia.grad, d_txt_all=ta.grad)


@pytest.mark.parametrize("D", R.PAIR_D)
@pytest.mark.parametrize("Bl,Bg,off", R.PAIR_SHAPES)
def test_clip_ref_and_mutants(Bl, Bg, off, D):
    case = R.pair_case(Bl, Bg, off, D)
    for t in case:
        assert close(t.double().norm(dim=-1), torch.ones(t.shape[0]), 1e-6)
    for ls in R.PAIR_SCALES:
        ref = R.clip_ref(*case, ls, off, R.pair_prefill(ls))
        want = _clip_autograd(*case, ls, off)
        for k, (val, bar) in ref.items():
            assert close(val, want[k].reshape(val.shape), 1e-9), k
            assert bool((torch.as_tensor(bar) > 0).all()), k
        mutants = [dict(weight=1.0)] + ([dict(label_offset=False)] if off else [])
        for kw in mutants:
            bad = _clip_autograd(*case, ls, off, **kw)
            if Bg > 1:
                assert all(misses(bad[k], ref[k][0], ref[k][1]) for k in ("loss", "d_img_local", "d_txt_all")), (kw, ls)
            else:   # one pair: the loss is log 1 and every gradient zero whatever the weight; only the accumulators can tell
                assert close(bad["loss"], 0.0 * bad["loss"]) and float(ref["loss"][0]) == 0.0
        for k in ("loss", "d_logit_scale"):                                   # `=` for `+=`
            assert misses(ref[k][0].reshape(1), (R.pair_prefill(ls) + ref[k][0]).reshape(1), ref[k][1].reshape(1))


# ------------------------------------------------------------------------------------------------------------ SigLIP
@pytest.mark.parametrize("D", R.PAIR_D)
@pytest.mark.parametrize("Bl,Bg,off", R.PAIR_SHAPES)
def test_siglip_ref_and_mutants(Bl, Bg, off, D):
    img_l, _, _, txt_all = R.pair_case(Bl, Bg, off, D)
    dls_hits = []
    for ls in R.PAIR_SCALES:
        for bias in R.SIGLIP_BIASES:
            ref = R.siglip_ref(img_l, txt_all, ls, bias, off, R.pair_prefill(ls))       # the oracle and its autograd
            own = R.siglip_values(R.siglip_parts(img_l, txt_all, ls, bias, off))     # the kernel's formulas
            for k, (val, bar) in ref.items():
                assert close(own[k], val.reshape(own[k].shape), 2.0 ** -23), k          # fp32(1 / B_local) against 1 / B_local
            bad = R.siglip_values(R.siglip_parts(img_l, txt_all, ls, bias, off, dls_with_bias=True))
            hit = misses(bad["d_logit_scale"].view(1), ref["d_logit_scale"][0].view(1), ref["d_logit_scale"][1].view(1))
            dls_hits.append(hit)
            assert hit or Bg == 1, (ls, bias)     # one pair: where its sigmoid has vanished, so has the bias gradient b times which is the difference
            if off:
                bad = R.siglip_values(R.siglip_parts(img_l, txt_all, ls, bias, off, label_offset=False))
                miss = {k: misses(bad[k].reshape(-1), ref[k][0].reshape(-1), ref[k][1].reshape(-1)) for k in ref}
                assert miss["loss"] and miss["d_img_local"] and miss["d_txt_all"], (ls, bias, miss)
            for k in ("loss", "d_logit_scale", "d_logit_bias"):                      # `=` for `+=`
                assert misses(ref[k][0].reshape(1), (R.pair_prefill(ls) + ref[k][0]).reshape(1), ref[k][1].reshape(1)), k
    assert any(dls_hits)


def test_pair_cases_cross_the_row_loops():
    assert any(Bg > 256 for _, Bg, _ in R.PAIR_SHAPES) and any(Bl > 256 for Bl, _, _ in R.PAIR_SHAPES)     # the 256-thread stride
    assert any(off and off + Bl == Bg for Bl, Bg, off in R.PAIR_SHAPES) and any(D > 256 and D % 256 for D in R.PAIR_D)
    assert all(D % 4 == 0 for D in R.PAIR_D)


# ------------------------------------------------------------------------------------------------------------ KoLeo
@pytest.mark.parametrize("B,D,groups,beside", R.KOLEO_CASES)
def test_koleo_ref_conditions_and_mutants(B, D, groups, beside):
    xn = R.koleo_case(B, D, groups, beside)
    assert xn.dtype == F32 and close(xn.double().norm(dim=-1), torch.ones(B), 1e-6)
    gap, first = R.koleo_gap(xn)
    # the condition: an fp32 dot product of unit rows errs by at most D 2^-24, so a gap of four times that decides the neighbour
    assert float(gap.min()) >= 4 * D * 2.0 ** -24, float(gap.min())
    tied = torch.zeros(B, dtype=torch.bool)
    for grp in groups:
        for j in grp:
            assert torch.equal(xn[j], xn[grp[0]])
        others = [i for i in range(B) if first[i] == grp[0] and i not in grp]     # the rows that face the tie from outside
        assert all(q in others for q, near in beside if near in grp)
        tied[list(grp)] = True
        tied[others] = True
        assert all(int(first[i]) == (grp[0] if i != grp[0] else grp[1]) for i in list(grp) + others)
    loss_lo, nn_lo = LO.koleo_loss(xn.double(), R.KOLEO_EPS)
    assert torch.equal(nn_lo[~tied], first[~tied])             # the oracle's neighbours wherever no tie is planted
    ref = R.koleo_ref(xn, 1.0 / B, R.KOLEO_EPS, R.KOLEO_PREFILL, nn=first)
    if not groups:
        assert torch.equal(R.koleo_ref(xn, 1.0 / B)["nn"], first)
    # the oracle renormalises its rows in float64 (a relative 2^-24 on each): its loss agrees as far as that allows
    assert abs(float(loss_lo) - float(ref["loss"])) <= 1e-6 * max(1.0, float((2.0 ** -24 / ref["dist"]).max()) * 1e6)
    # gradient: autograd of the same loss with the neighbours held fixed
    xr = xn.double().requires_grad_(True)
    dist = ((xr - xr[first] + R.f32(1e-8)) ** 2).sum(1).sqrt()
    (-R.f32(1.0 / B) * torch.log(dist + R.f32(R.KOLEO_EPS)).sum()).backward()
    assert close(ref["d_xn"], xr.grad, 1e-9)
    if groups:      # identical rows: the distance is 1e-8 sqrt(D), finite
        i = groups[0][0]
        assert close(ref["dist"][i], R.f32(1e-8) * math.sqrt(D), 1e-12) and bool(torch.isfinite(ref["d_xn"].to(F32)).all())
    # wrong variants.  nn is compared exactly, so any other index is a miss
    if any(len(grp) > 2 or any(first[i] == grp[0] for i in range(B) if i not in grp) for grp in groups):
        xd = xn.double()
        dots = xd @ xd.T
        dots.fill_diagonal_(-float("inf"))
        last = torch.where(dots >= dots.max(1, keepdim=True).values - 1e-13, torch.arange(B).expand(B, B), -1).max(1).values
        assert not torch.equal(last, first)                    # the tie resolved to the larger index
    assert not torch.equal(torch.arange(B), first)             # self allowed as neighbour
    bad = R.koleo_ref(xn, 1.0 / B, R.KOLEO_EPS, R.KOLEO_PREFILL, nn=first, minus_g=False)
    assert misses(bad["d_xn"], ref["d_xn"], ref["d_xn_bar"])
    if B > 2 or not groups:     # two identical rows alone: gradients of 1e7, whose rounding is larger than any sensible prefill
        assert misses(ref["d_xn"], R.KOLEO_PREFILL + ref["d_xn"], ref["d_xn_bar"])        # `=` for `+=`
    assert misses(ref["loss"].view(1), (R.KOLEO_PREFILL + ref["loss"]).view(1), ref["loss_bar"].view(1))


def test_koleo_cases_cross_the_row_loops():
    shapes = {(B, D) for B, D, _, _ in R.KOLEO_CASES}
    assert shapes == {(2, 4), (3, 256), (256, 260), (257, 64), (260, 768), (4, 16384)}
    same_thread = [(g, q) for B, D, gs, q in R.KOLEO_CASES for g in gs if any(abs(a - b) % 256 == 0 for a in g for b in g if a != b)]
    assert len(same_thread) == 2                              # two candidates of one thread's own j loop, twice


# ------------------------------------------------------------------------------------------------------------ Sinkhorn-Knopp
@pytest.mark.parametrize("T,K", R.SK_CASES)
def test_sinkhorn_ref_and_mutants(T, K):
    logits = R.sk_case(T, K)
    assert logits.shape == (T + R.SK_PAD, K)
    z = logits[:T].double() * R.f32(R.SK_INV_TEMP)
    assert float(z.max() - z.min()) < 80.0                     # e^(z - shift) stays a normal fp32 number
    assert float(logits[T:].float().min()) >= float(logits[:T].float().max()) + R.SK_HOSTILE - 0.5
    ref = R.sinkhorn_ref(logits, R.SK_INV_TEMP, T)
    probs, u = R.sinkhorn_uv_ref(logits, R.SK_INV_TEMP, T, float(T))
    assert close(probs, ref, 1e-10) and close(ref.sum(1), torch.ones(T), 1e-10)
    assert close(R.sinkhorn_uv_ref(logits, R.SK_INV_TEMP, T, 3.0 * T)[0], ref, 1e-10)        # the count leaves the targets alone
    rel_u, rel_p = R.sinkhorn_rel(logits, R.SK_INV_TEMP, T)
    bar = R.sinkhorn_probs_bar(ref, rel_p)
    assert rel_p < 2.0 ** -10                                  # the fp32 part stays below the bf16 rounding
    bad, _ = R.sinkhorn_uv_ref(logits, R.SK_INV_TEMP, T, float(T), rows_in_sums=T + R.SK_PAD)
    assert misses(bad, ref, bar)                               # padded rows counted in the prototype sums
    _, bad_u = R.sinkhorn_uv_ref(logits, R.SK_INV_TEMP, T, float(T + R.SK_PAD))
    assert misses(bad_u, u, rel_u * u)                         # the count taken from the buffer height
    two, _ = R.sinkhorn_uv_ref(logits, R.SK_INV_TEMP, T, float(T), n_iter=2)
    assert misses(two, ref, bar) == (T > 1)                    # two iterations (one sample: the first is already the fixed point)


def test_sinkhorn_cases_cross_the_row_blocks():
    assert {T for T, _ in R.SK_CASES} == {1, 63, 64, 65, 130} and (130, 65536) in R.SK_CASES
    assert all(K % 8 == 0 for _, K in R.SK_CASES) and any(K % 2048 for _, K in R.SK_CASES) and any(K < 2048 for _, K in R.SK_CASES)


# ------------------------------------------------------------------------------------------------------------ colsum_bf16_rows
@pytest.mark.parametrize("C", R.COLSUM_C)
def test_colsum_ref_and_mutant(C):
    for n in R.COLSUM_ROWS:
        x = R.colsum_case(n, C)
        assert x.shape == (R.COLSUM_RMAX, C + 8) and bool((x[n:] == R.COLSUM_BEYOND).all())
        ref, sumabs = R.colsum_rows_ref(x, n, C)
        assert close(ref, x.double()[:n, :C].sum(0)) if n else not bool(ref.any())
        bar = R.colsum_bar(sumabs, R.COLSUM_PREFILL)
        if n < R.COLSUM_RMAX:
            bad, _ = R.colsum_rows_ref(x, n + 1, C)
            assert misses(R.COLSUM_PREFILL + bad, R.COLSUM_PREFILL + ref, bar)       # one row beyond the count
        if n:
            assert misses(ref, R.COLSUM_PREFILL + ref, bar)                          # `=` for `+=`


# ------------------------------------------------------------------------------------------------------------ token rows
@pytest.mark.parametrize("T,D,n_src,kind", R.TOKEN_CASES)
def test_token_row_refs(T, D, n_src, kind):
    src, idx = R.token_case(T, D, n_src, kind)
    live = idx >= 0
    assert len(set(idx[live].tolist())) == int(live.sum()) and (kind == "none") == (not bool(live.any()))
    got = R.gather_token_rows_ref(src, idx)
    want = torch.zeros(T, D, dtype=BF)
    want[live] = torch.index_select(src, 0, idx[live].long())
    assert torch.equal(R.bits(got), R.bits(want))
    if bool(live.any()):
        assert not torch.equal(R.bits(src[idx.clamp_min(0).long()]), R.bits(got))     # -1 read as row 0
    base = torch.full((n_src, D), R.SENTINEL, dtype=BF)
    back = R.scatter_token_rows_ref(got, idx, base)
    want = base.clone().index_copy_(0, idx[live].long(), got[live])
    assert torch.equal(R.bits(back), R.bits(want))
    assert int((back == R.SENTINEL).all(1).sum()) >= n_src - int(live.sum())


def test_token_cases_reach_the_grid_stride_loop():
    assert any(T * D // 8 > 4096 * 256 for T, D, _, _ in R.TOKEN_CASES) and any(D == 8 for _, D, _, _ in R.TOKEN_CASES)
