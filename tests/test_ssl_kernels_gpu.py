"""The self-supervised and contrastive loss kernels one by one against tests/ssl_ref.py (float64 on the CPU): softmax_center (both entry
points), dino_ce, center_ema, weight_norm_prep / _bwd, gather / scatter_token_rows (csrc/ssl.hip), siglip_loss, koleo, sinkhorn_knopp in
its whole, phased and two-rank forms (csrc/losses.hip), l2norm_fwd / _bwd and clip_loss (csrc/clip.hip) and colsum_bf16_rows
(csrc/elementwise.hip).  The cases and the derived bars live in tests/ssl_ref.py; tests/test_ssl_ref_host.py shows without a GPU that
each bar rejects wrong variants at these inputs.

Buffers a kernel must fully write are prefilled with NaN, rows it must not touch with 7.0, accumulators with a non-zero value.

Every test prints `ssl_kernels: <kernel> <case>: worst error / bar` (profiles/ssl_kernels.log)."""
import pytest
import torch

import ssl_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
NAN = float("nan")


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def full(shape, value, dtype=F32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def report(kernel, case, r, note=""):
    print(f"ssl_kernels: {kernel} {case}: worst error / bar = {r:.3f}{note}")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(R.bits(a.cpu()), R.bits(b.cpu()))


def untouched(t):
    return bool((t == R.SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ softmax_center
def run_softmax(logits, center, inv_temp, T, K):
    """T rows of a (T + 1)-row buffer: the last row keeps the sentinel"""
    from vtp_amd import ops
    probs = full((T + 1, K), NAN, BF)
    probs[T] = R.SENTINEL
    ops.softmax_center(logits, center, inv_temp, probs, T, K)
    assert untouched(probs[T])
    return probs[:T]


def check_softmax(logits_c, center_c, inv_temp, K):
    T = logits_c.shape[0]
    logits, center = dev(logits_c), dev(center_c)
    got = run_softmax(logits, center, inv_temp, T, K)
    got_dev = run_softmax(logits, center, torch.tensor([inv_temp], dtype=F32, device=DEV), T, K)
    assert same_bits(got, got_dev)                            # the device-temperature entry: the same bits
    ref, _, z = R.softmax_center_ref(logits_c, center_c, inv_temp)
    bar = R.softmax_bar(ref, z, K)
    r = R.ratio(got, ref, bar)                                # a NaN anywhere is an infinite ratio
    rs = R.ratio(got.double().sum(1).cpu(), torch.ones(T, dtype=F64), bar.sum(1))
    return got.cpu(), ref, max(r, rs)


@pytest.mark.parametrize("K", R.SOFTMAX_K)
def test_softmax_center(K):
    for T in R.SOFTMAX_T:
        for with_center in (True, False):
            logits, center = R.softmax_case(K, T, with_center)
            _, _, r = check_softmax(logits, center, R.SOFTMAX_INV_TEMP, K)
            report("softmax_center", (K, T, "centre" if with_center else "no centre"), r)
            assert r <= 1.0, (K, T, with_center, r)


@pytest.mark.parametrize("K", R.SOFTMAX_K)
def test_softmax_center_hand_rows(K):
    for with_center in (True, False):
        logits, center = R.softmax_hand_case(K, with_center)
        got, ref, r = check_softmax(logits, center, R.HAND_INV_TEMP, K)
        report("softmax_center", (K, "hand rows", "centre" if with_center else "no centre"), r)
        assert r <= 1.0, (K, with_center, r)
        assert bool((R.bits(got[0]) == R.bits(got[0])[0]).all())          # the constant row: exactly uniform


# ------------------------------------------------------------------------------------------------------------ dino_ce
@pytest.mark.parametrize("K", R.DINO_K)
def test_dino_ce(K):
    from vtp_amd import ops
    S_c, P_c, t0_c, t1_c, w_c = R.dino_case(K)
    T = S_c.shape[0]
    ref = R.dino_ce_ref(S_c, P_c, t0_c, t1_c, w_c, R.DINO_INV_TEMP)
    row_bar, total_bar = R.dino_loss_bar(ref, K, R.DINO_PREFILL, T)
    S, P, t0, t1, w = (dev(t) for t in (S_c, P_c, t0_c, t1_c, w_c))
    loss = full((1,), R.DINO_PREFILL)
    dS = full((T + 1, K), NAN, BF)
    dS[T] = R.SENTINEL
    ops.dino_ce(S, P, t0, t1, w, R.DINO_INV_TEMP, loss, dS, T, K)
    assert untouched(dS[T])
    r_ds = R.ratio(dS[:T], ref["dS"], R.dino_ds_bar(ref, K))
    r_sum = R.ratio(loss, (R.DINO_PREFILL + ref["loss"].sum()).view(1), total_bar.view(1))
    r_row = 0.0
    for i in range(T):                                        # the loss of each row: single-row views of the same buffers
        li = full((1,), R.DINO_PREFILL)
        di = full((1, K), NAN, BF)
        ops.dino_ce(S[i:i + 1], P, t0[i:i + 1], t1[i:i + 1], w[i:i + 1], R.DINO_INV_TEMP, li, di, 1, K)
        assert same_bits(di, dS[i:i + 1])
        if float(ref["live"][i]) == 0:                        # a padding row: zero bits, and nothing added
            assert not bool(R.bits(dS[i].cpu()).any()) and float(li) == R.DINO_PREFILL
        else:
            r_row = max(r_row, R.ratio(li, (R.DINO_PREFILL + ref["loss"][i]).view(1), row_bar[i].view(1)))
    r = max(r_ds, r_sum, r_row)
    report("dino_ce", (K,), r, f" (dS {r_ds:.3f}, loss per row {r_row:.3f}, launch {r_sum:.3f})")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------ Sinkhorn-Knopp
class _SK:
    """the buffers of one process: logits [rows, K] of which n_valid count; n_valid None: no device row count"""

    def __init__(self, logits_c, K, n_valid, count, device_counts=True):
        self.T, self.K = logits_c.shape[0], K
        self.lg = dev(logits_c)
        self.probs = full((self.T, K), NAN, BF)
        self.u, self.v = full((self.T,), NAN), full((K,), NAN)
        self.scr = full((8 + K + self.T,), NAN)
        self.count = 0.0 if device_counts else float(count)
        self.cnt = torch.tensor([float(count)], device=DEV) if device_counts else None
        self.rows = torch.tensor([n_valid], dtype=I32, device=DEV) if device_counts else None

    def run(self, it, phase):
        from vtp_amd import ops
        ops.sinkhorn_knopp(self.lg, R.SK_INV_TEMP, self.probs, self.u, self.v, self.scr, self.T, self.K, self.count, it, phase, self.cnt,
                           self.rows)


def run_phased(procs, K, n_iter=3):
    """phases 0, (1, 2) x n_iter, 3 over one or more emulated ranks: the maximum and the prototype sums are combined on the host where
    the trainer all-reduces them"""
    for p in procs:
        p.run(0, 0)
    if len(procs) > 1:
        m = torch.stack([p.scr[0] for p in procs]).max()
        for p in procs:
            p.scr[0] = m
    for i in range(n_iter):
        for p in procs:
            p.run(i, 1)
        if len(procs) > 1:
            s = torch.stack([p.scr[8:8 + K] for p in procs]).sum(0)
            for p in procs:
                p.scr[8:8 + K] = s
        for p in procs:
            p.run(i, 2)
    for p in procs:
        p.run(n_iter, 3)


@pytest.mark.parametrize("T,K", R.SK_CASES)
def test_sinkhorn_knopp(T, K):
    logits = R.sk_case(T, K)
    ref = R.sinkhorn_ref(logits, R.SK_INV_TEMP, T)
    _, u_ref = R.sinkhorn_uv_ref(logits, R.SK_INV_TEMP, T, float(T))
    rel_u, rel_p = R.sinkhorn_rel(logits, R.SK_INV_TEMP, T)
    bar = R.sinkhorn_probs_bar(ref, rel_p)

    def worst(probs, u=None):
        r = max(R.ratio(probs, ref, bar), R.ratio(probs.double().sum(1).cpu(), torch.ones(T, dtype=F64), bar.sum(1)))
        return r if u is None else max(r, R.ratio(u, u_ref, rel_u * u_ref))

    padded = _SK(logits, K, T, T)                             # hostile rows behind the device row count
    padded.run(3, -1)
    r_pad = worst(padded.probs[:T], padded.u[:T])
    plain = _SK(logits[:T], K, T, T, device_counts=False)     # the same rows alone, counts from the host
    plain.run(3, -1)
    r_plain = worst(plain.probs, plain.u)
    phased = _SK(logits, K, T, T)
    run_phased([phased], K)
    r_ph = worst(phased.probs[:T], phased.u[:T])
    if T <= 64:                                               # one row block per column: a fixed order of every sum
        assert same_bits(padded.probs[:T], plain.probs) and same_bits(padded.u[:T], plain.u)
        assert same_bits(phased.probs[:T], padded.probs[:T]) and same_bits(phased.u[:T], padded.u[:T])
    # two emulated ranks: rows [0, h) and [h, T), each with its own hostile rows behind; the count is the global one
    h = T // 2
    pad = logits[T:]
    ranks = [_SK(torch.cat([logits[:h], pad]), K, h, T), _SK(torch.cat([logits[h:T], pad]), K, T - h, T)]
    run_phased(ranks, K)
    both = torch.cat([ranks[0].probs[:h], ranks[1].probs[:T - h]])
    r_ranks = worst(both, torch.cat([ranks[0].u[:h], ranks[1].u[:T - h]]))
    r = max(r_pad, r_plain, r_ph, r_ranks)
    report("sinkhorn_knopp", (T, K), r, f" (padded {r_pad:.3f}, alone {r_plain:.3f}, phased {r_ph:.3f}, two ranks {r_ranks:.3f})")
    assert r <= 1.0


@pytest.mark.parametrize("K", (8, 2056))
def test_sinkhorn_knopp_without_rows(K):
    """n_rows = 0, a step without masked patches: the call returns; what it leaves in probs is unspecified and nothing reads it: the
    cross entropy over the all-padding rows adds nothing and writes zero rows"""
    from vtp_amd import ops
    T = 3
    sk = _SK(R.sk_case(1, K, pad=T)[1:], K, 0, 0)
    sk.run(3, -1)
    torch.cuda.synchronize()
    run_phased([sk], K)
    torch.cuda.synchronize()
    S = dev(R.dino_case(K)[0][:T])
    idx = full((T,), -1, I32)
    loss, dS = full((1,), R.DINO_PREFILL), full((T, K), NAN, BF)
    ops.dino_ce(S, sk.probs, idx, idx, full((T,), 1.0), R.DINO_INV_TEMP, loss, dS, T, K)
    assert float(loss) == R.DINO_PREFILL and not bool(R.bits(dS.cpu()).any())
    report("sinkhorn_knopp", (0, K), 0.0, " (no rows: returns; dino_ce over padding rows adds nothing)")


# ------------------------------------------------------------------------------------------------------------ KoLeo
@pytest.mark.parametrize("B,D,groups,beside", R.KOLEO_CASES)
def test_koleo(B, D, groups, beside):
    from vtp_amd import ops
    xn_c = R.koleo_case(B, D, groups, beside)
    _, first = R.koleo_gap(xn_c)
    ref = R.koleo_ref(xn_c, 1.0 / B, R.KOLEO_EPS, R.KOLEO_PREFILL, nn=first)
    xn = dev(xn_c)
    nn = full((B,), -7, I32)
    d_xn, loss = full((B, D), R.KOLEO_PREFILL), full((1,), R.KOLEO_PREFILL)
    ops.koleo(xn, nn, d_xn, loss, B, D, 1.0 / B, R.KOLEO_EPS)
    assert torch.equal(nn.cpu().long(), ref["nn"])            # exact, ties to the smaller index
    r_loss = R.ratio(loss, (R.KOLEO_PREFILL + ref["loss"]).view(1), ref["loss_bar"].view(1))
    r_g = R.ratio(d_xn, R.KOLEO_PREFILL + ref["d_xn"], ref["d_xn_bar"])
    r = max(r_loss, r_g)
    report("koleo", (B, D, "ties" if groups else "no tie"), r, f" (loss {r_loss:.3f}, d_xn {r_g:.3f})")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------ SigLIP and CLIP
def _worst(got, ref, prefill, prefilled=()):
    """got: name -> tensor; ref: name -> (value, bar); names in `prefilled` were accumulated onto `prefill`"""
    out = {}
    for k, (val, bar) in ref.items():
        val = torch.as_tensor(val, dtype=F64).reshape(got[k].shape)
        bar = torch.as_tensor(bar, dtype=F64).reshape(got[k].shape)
        out[k] = R.ratio(got[k], val + (prefill if k in prefilled else 0.0), bar)
    return out


@pytest.mark.parametrize("D", R.PAIR_D)
@pytest.mark.parametrize("Bl,Bg,off", R.PAIR_SHAPES)
def test_siglip_loss(Bl, Bg, off, D):
    from vtp_amd import ops
    img_l_c, _, _, txt_all_c = R.pair_case(Bl, Bg, off, D)
    img_l, txt_all = dev(img_l_c), dev(txt_all_c)
    acc = ("loss", "d_logit_scale", "d_logit_bias")
    for ls in R.PAIR_SCALES:
        for bias in R.SIGLIP_BIASES:
            ref = R.siglip_ref(img_l_c, txt_all_c, ls, bias, off, R.pair_prefill(ls))
            got = dict(loss=full((1,), R.pair_prefill(ls)), d_logit_scale=full((1,), R.pair_prefill(ls)), d_logit_bias=full((1,), R.pair_prefill(ls)),
                       d_img_local=full((Bl, D), NAN), d_txt_all=full((Bg, D), NAN))
            ops.siglip_loss(img_l, txt_all, full((1,), ls), full((1,), bias), Bl, Bg, D, off, got["loss"], got["d_img_local"],
                            got["d_txt_all"], got["d_logit_scale"], got["d_logit_bias"], full((Bl * Bg,), NAN))
            rs = _worst(got, ref, R.pair_prefill(ls), acc)
            r = max(rs.values())
            report("siglip_loss", (Bl, Bg, off, D, round(ls, 3), bias), r, " (" + ", ".join(f"{k} {v:.3f}" for k, v in rs.items()) + ")")
            assert r <= 1.0, rs


@pytest.mark.parametrize("D", R.PAIR_D)
@pytest.mark.parametrize("Bl,Bg,off", R.PAIR_SHAPES)
def test_clip_loss(Bl, Bg, off, D):
    from vtp_amd import ops
    case_c = R.pair_case(Bl, Bg, off, D)
    img_l, txt_l, img_all, txt_all = (dev(t) for t in case_c)
    for ls in R.PAIR_SCALES:
        ref = R.clip_ref(*case_c, ls, off, R.pair_prefill(ls))
        got = dict(loss=full((1,), R.pair_prefill(ls)), d_logit_scale=full((1,), R.pair_prefill(ls)), d_img_local=full((Bl, D), NAN),
                   d_txt_local=full((Bl, D), NAN), d_img_all=full((Bg, D), NAN), d_txt_all=full((Bg, D), NAN))
        ops.clip_loss(img_l, txt_l, img_all, txt_all, full((1,), ls), Bl, Bg, D, off, got["loss"], got["d_img_local"], got["d_txt_local"],
                      got["d_img_all"], got["d_txt_all"], got["d_logit_scale"], full((2 * Bl * Bg,), NAN))
        rs = _worst(got, ref, R.pair_prefill(ls), ("loss", "d_logit_scale"))
        r = max(rs.values())
        report("clip_loss", (Bl, Bg, off, D, round(ls, 3)), r, " (" + ", ".join(f"{k} {v:.3f}" for k, v in rs.items()) + ")")
        assert r <= 1.0, rs


def test_pair_losses_reject_bad_shapes():
    from vtp_amd import ops
    z = lambda *s: torch.zeros(*s, device=DEV)
    one = z(1)
    for Bl, Bg, off, D in ((2, 4, 0, 6), (3, 4, 2, 8)):       # D % 4 != 0; off + Bl > Bg
        with pytest.raises(RuntimeError):
            ops.siglip_loss(z(Bl, D), z(Bg, D), one, one, Bl, Bg, D, off, z(1), z(Bl, D), z(Bg, D), z(1), z(1), z(Bl * Bg))
        with pytest.raises(RuntimeError):
            ops.clip_loss(z(Bl, D), z(Bl, D), z(Bg, D), z(Bg, D), one, Bl, Bg, D, off, z(1), z(Bl, D), z(Bl, D), z(Bg, D), z(Bg, D), z(1),
                          z(2 * Bl * Bg))
    torch.cuda.synchronize()
    report("siglip_loss / clip_loss", "bad shapes", 0.0, " (D % 4 != 0 and off + Bl > Bg raise RuntimeError)")


# ------------------------------------------------------------------------------------------------------------ weight norm
@pytest.mark.parametrize("K,C", R.WN_CASES)
def test_weight_norm_prep_and_bwd(K, C):
    from vtp_amd import ops
    v_c, g_c, dW_c = R.wn_case(K, C)
    v, g, dW = dev(v_c), dev(g_c), dev(dW_c)
    weff_ref, inv_ref, _ = R.weight_norm_prep_ref(v_c, g_c)
    r_prep = 0.0
    for transposed in (True, False):                          # with weffT and C <= 256: the tiled kernel; else the plain one
        weff, inv = full((K + 1, C), NAN, BF), full((K + 1,), NAN)
        weff[K], inv[K] = R.SENTINEL, R.SENTINEL
        weffT = full((C, K), NAN, BF) if transposed else None
        ops.weight_norm_prep(v, g, weff, weffT, inv, K, C)
        assert untouched(weff[K]) and untouched(inv[K:])
        if transposed:
            assert same_bits(weffT, weff[:K].T.contiguous())
        r_prep = max(r_prep, R.ratio(weff[:K], weff_ref, R.wn_weff_bar(weff_ref, C)), R.ratio(inv[:K], inv_ref, R.wn_inv_bar(inv_ref, C)))
    inv_c = inv_ref.to(F32)                                   # the backward on the rounded float64 norms, whatever prep gave
    ref = R.weight_norm_bwd_ref(dW_c, v_c, g_c, inv_c)
    dv_bar, dg_bar = R.wn_bwd_bars(ref, C, R.WN_PREFILL)
    dv, dg = full((K + 1, C), R.WN_PREFILL), full((K + 1,), R.WN_PREFILL)
    dv[K], dg[K] = R.SENTINEL, R.SENTINEL
    ops.weight_norm_bwd(dW, v, g, dev(inv_c), dv, dg, K, C)
    assert untouched(dv[K]) and untouched(dg[K:])
    r_dv = R.ratio(dv[:K], R.WN_PREFILL + ref["dv"], dv_bar)
    r_dg = R.ratio(dg[:K], R.WN_PREFILL + ref["dg"], dg_bar)
    r = max(r_prep, r_dv, r_dg)
    report("weight_norm_prep/_bwd", (K, C), r, f" (prep {r_prep:.3f}, dv {r_dv:.3f}, dg {r_dg:.3f})")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------ l2norm
@pytest.mark.parametrize("eps", R.L2_EPS)
@pytest.mark.parametrize("D", R.L2_D)
def test_l2norm_fwd_and_bwd(D, eps):
    from vtp_amd import ops
    x_c, dy_c = R.l2_case(D)
    B = x_c.shape[0]
    y_ref, inv_ref, _ = R.l2norm_fwd_ref(x_c, eps)
    y, inv = full((B + 1, D), NAN), full((B + 1,), NAN)
    y[B], inv[B] = R.SENTINEL, R.SENTINEL
    ops.l2norm_fwd(dev(x_c), y, inv, B, D, eps)
    assert untouched(y[B]) and untouched(inv[B:])
    r_fwd = max(R.ratio(y[:B], y_ref, R.l2_y_bar(y_ref, D)), R.ratio(inv[:B], inv_ref, R.l2_inv_bar(inv_ref, D)))
    assert not bool(y[1].any())                               # the zero row: y = 0 (inv = 1 / eps and a finite dx are in the ratios)
    y_c, inv_c = y_ref.to(F32), inv_ref.to(F32)
    ref = R.l2norm_bwd_ref(dy_c, y_c, inv_c)
    dx = full((B + 1, D), NAN)
    dx[B] = R.SENTINEL
    ops.l2norm_bwd(dev(dy_c), dev(y_c), dev(inv_c), dx, B, D)
    assert untouched(dx[B])
    r_bwd = R.ratio(dx[:B], ref["dx"], R.l2_bwd_bar(ref, D))
    r = max(r_fwd, r_bwd)
    report("l2norm_fwd/_bwd", (D, eps), r, f" (fwd {r_fwd:.3f}, bwd {r_bwd:.3f})")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------ center_ema
@pytest.mark.parametrize("K", R.EMA_K)
def test_center_ema(K):
    from vtp_amd import ops
    center_c, colsum_c = R.ema_case(K)
    worst = 0.0
    for count in R.EMA_COUNTS:
        buf = full((K + 1,), R.SENTINEL)
        buf[:K] = dev(center_c)
        cnt = None if count is None else torch.tensor([count], dtype=F32, device=DEV)
        ops.center_ema(buf, dev(colsum_c), R.EMA_HOST_INV_COUNT if count is None else 0.0, R.EMA_MOMENTUM, K, cnt)
        assert untouched(buf[K:])
        ref, sumabs = R.center_ema_ref(center_c, colsum_c, R.EMA_HOST_INV_COUNT, count, R.EMA_MOMENTUM)
        r = R.ratio(buf[:K], ref, R.ema_bar(sumabs))
        report("center_ema", (K, "host count" if count is None else f"device count {count}"), r)
        worst = max(worst, r)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ colsum_bf16_rows
@pytest.mark.parametrize("C", R.COLSUM_C)
def test_colsum_bf16_rows(C):
    from vtp_amd import ops
    worst = 0.0
    for n in R.COLSUM_ROWS:
        x_c = R.colsum_case(n, C)
        out = full((C + 8,), R.COLSUM_PREFILL)
        out[C:] = R.SENTINEL
        ops.colsum_bf16_rows(dev(x_c), C + 8, out, torch.tensor([n], dtype=I32, device=DEV), R.COLSUM_RMAX, C)
        assert untouched(out[C:])
        ref, sumabs = R.colsum_rows_ref(x_c, n, C)
        r = R.ratio(out[:C], R.COLSUM_PREFILL + ref, R.colsum_bar(sumabs, R.COLSUM_PREFILL))
        report("colsum_bf16_rows", (n, C), r)
        worst = max(worst, r)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ token rows
@pytest.mark.parametrize("T,D,n_src,kind", R.TOKEN_CASES)
def test_gather_and_scatter_token_rows(T, D, n_src, kind):
    from vtp_amd import ops
    src_c, idx_c = R.token_case(T, D, n_src, kind)
    src, idx = dev(src_c), dev(idx_c)
    dst = full((T + 1, D), NAN, BF)
    dst[T] = R.SENTINEL
    ops.gather_token_rows(src, idx, dst, T, D)
    assert untouched(dst[T]) and same_bits(dst[:T], R.gather_token_rows_ref(src_c, idx_c))
    d_dst_c = R.token_case(T, D, T, "none")[0]                # other values to send back
    back = full((n_src, D), R.SENTINEL, BF)
    ops.scatter_token_rows(dev(d_dst_c), idx, back, T, D)
    want = R.scatter_token_rows_ref(d_dst_c, idx_c, torch.full((n_src, D), R.SENTINEL, dtype=BF))
    assert same_bits(back, want)                              # the rows no index names keep the sentinel
    report("gather/scatter_token_rows", (T, D, kind), 0.0, " (bit-equal)")
