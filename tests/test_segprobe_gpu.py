"""GPU: the segmentation-probe kernels (csrc/segprobe.hip: vtp_seg_ce / vtp_seg_dlogits / vtp_seg_sgd, exact fp32) and
vtp_amd.SegProbe against fp64 (tests/seg_ref.py, itself pinned to torch's CPU ops by tests/test_segprobe_host.py).

Bounds.  gamma_n = n u / (1 - n u), u = 2^-24, bounds a chain of n fp32 roundings in any order.  The low-resolution logits obey
|err| <= gamma_{K+1} (|X| |W|^T + |b|) (tests/test_probe_gpu.py); the bilinear blend has non-negative weights that sum to one, so
that bound is carried to a pixel by interpolating it, and the blend's own 7 roundings add gamma_8 times the interpolated |Z|:
    bz(p, c) = up(gamma_{K+1} (|X| |W|^T + |b|))(p, c) + gamma_8 up(|Z|)(p, c).
lse is 1-Lipschitz in the sup norm, its sum of C exponentials, the exp and log and the final addition round: gamma_{C+4} relative,
    blse(p) = max_c bz(p, c) + gamma_{C+4} (1 + |lse(p)|).
1e-5 (relative; Frobenius for tensors) is the project's bar for fp32 arithmetic against fp64 (tests/test_losses_gpu.py)."""
import functools
import os

import pytest
import torch

import seg_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
NCASE = len(R.CASES)


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


@functools.lru_cache(maxsize=None)
def _reference(i, H, all_ignored):
    """the case's operands and, per head, the fp64 results and the bounds of the module docstring; computed once and never written"""
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, labels = R.make_case(i, H, all_ignored)
    heads = []
    for hh in range(H):
        Wh, bh = W[hh * C:(hh + 1) * C].double(), b[hh * C:(hh + 1) * C].double()
        z = (X.double() @ Wh.T + bh).view(B, h, w, C)
        r = R.loss_and_grad(z, labels)
        bz_cells = R.gamma(K + 1) * (X.double().abs() @ Wh.abs().T + bh.abs()).view(B, h, w, C)
        r["bz"] = R.upsample(bz_cells, Hl, Wl) + R.gamma(8) * R.upsample(z.abs(), Hl, Wl)
        r["blse"] = r["bz"].amax(-1) + R.gamma(C + 4) * (1.0 + r["lse"].abs())
        top2 = r["up"].topk(2, dim=-1).values
        r["keep"] = (top2[..., 0] - top2[..., 1]) >= 2.0 * r["bz"].amax(-1)  # the argmax cannot change within the bound
        heads.append(r)
    return X, W, b, labels, heads


def _pixel_pass(i, H, all_ignored, with_lse=True, with_conf=True):
    """low-resolution logits from vtp_probe_logits (NaN columns past H C), then vtp_seg_ce on poisoned outputs"""
    from vtp_amd import ops
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, labels, _ = _reference(i, H, all_ignored)
    M, N = B * h * w, H * C
    z = torch.full((M, N + 3), float("nan"), device=DEV, dtype=F32)
    ops.probe_logits(_sliced(X), W.to(DEV), b.to(DEV), z, M, N, K)
    y = labels.to(DEV)
    out = dict(z=z, y=y, loss=torch.full((H,), float("nan"), device=DEV), cc=torch.full((2,), -7, device=DEV, dtype=torch.int32),
               lse=torch.full((H, B, Hl, Wl), float("nan"), device=DEV) if with_lse else None,
               conf=torch.full((H, C, C), 3, device=DEV, dtype=torch.int64) if with_conf else None,
               totals=torch.tensor([5, 7], device=DEV, dtype=torch.int64))
    nbytes = ops.seg_ce_workspace_bytes(B, h, w, Hl, Wl, H, C)
    ws = torch.full((nbytes + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    ops.seg_ce(z, y, (h, w), H, C, 255, out["loss"], out["cc"], ws[:nbytes], lse=out["lse"], conf=out["conf"], totals=out["totals"])
    assert bool((ws[nbytes:] == 0xA5).all()), "wrote past the workspace"
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. pixel pass
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("i", range(NCASE))
def test_pixel_pass_lse_loss_counts_and_confusion(i, H):
    _gpu()
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, labels, heads = _reference(i, H, False)
    o = _pixel_pass(i, H, False)
    nv, oor = heads[0]["n_valid"], heads[0]["out_of_range"]
    assert o["cc"].tolist() == [nv, oor] and o["totals"].tolist() == [5 + nv, 7 + oor]
    left_out = 0
    for hh, r in enumerate(heads):
        err = (o["lse"][hh].cpu().double() - r["lse"]).abs()
        print(f"SEG-CE case {i} H={H} head {hh}: lse max err/bound {float((err / r['blse']).max()):.3f}")
        assert bool((err <= r["blse"]).all())
        rel = abs(float(o["loss"][hh]) - r["loss"]) / r["loss"]
        print(f"SEG-CE case {i} H={H} head {hh}: loss rel err {rel:.2e}")
        assert rel <= 1e-5
        # confusion: exact on the pixels whose fp64 top-2 margin is at least twice the bound; the others (at most 1 % of the case's
        # pixels) are left out of both sides: they may sit in any column of their target's row, and nowhere else
        n_out = int((~r["keep"] & r["valid"]).sum())
        left_out = max(left_out, int((~r["keep"]).sum()))
        extra = o["conf"][hh].cpu() - 3 - R.confusion(r["up"], labels, r["keep"])
        assert bool((extra >= 0).all()) and int(extra.sum()) == n_out
        assert torch.equal(extra.sum(1), torch.bincount(labels.long()[~r["keep"] & r["valid"]], minlength=C)[:C])
    print(f"SEG-CE case {i} H={H}: {left_out} of {B * Hl * Wl} pixels left out of the confusion check")
    assert left_out <= 0.01 * B * Hl * Wl, "more than 1 % of the pixels within the bound of a tie"
    # evaluation (no lse) and training (no confusion matrix) calls: the same losses bit for bit
    for kw in (dict(with_lse=False), dict(with_conf=False)):
        assert torch.equal(_pixel_pass(i, H, False, **kw)["loss"], o["loss"])


@pytest.mark.parametrize("i", range(NCASE))
def test_pixel_pass_without_a_valid_pixel(i):
    _gpu()
    H = 3
    o = _pixel_pass(i, H, True)
    assert o["loss"].tolist() == [0.0] * H and o["cc"].tolist() == [0, 0] and o["totals"].tolist() == [5, 7]
    assert bool((o["conf"] == 3).all())
    heads = _reference(i, H, True)[4]
    for hh, r in enumerate(heads):  # lse is still every pixel's
        assert bool(((o["lse"][hh].cpu().double() - r["lse"]).abs() <= r["blse"]).all())


# ---------------------------------------------------------------------------------------------------------------- 2. cell pass
def _cell_pass(i, H, all_ignored):
    from vtp_amd import ops
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    o = _pixel_pass(i, H, all_ignored, with_conf=False)
    G = torch.full((B * h * w, H * C + 5), float("nan"), device=DEV, dtype=F32)
    ops.seg_dlogits(o["z"], o["y"], (h, w), H, C, 255, o["lse"], o["cc"], G)
    assert bool(G[:, H * C:].isnan().all()), "wrote past column H * C"
    return o, G[:, :H * C]


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("i", range(NCASE))
def test_cell_pass_gradient(i, H):
    """G against fp64: 1e-5 relative Frobenius per head; cells no pixel touches are exactly 0; the classes of a cell sum to zero
    within what the fp32 evaluation allows.  That last bound: lse comes from the SAME interpolated fp32 logits (seg_blend is one
    function), so sum_c exp(z_c - lse) misses 1 only by the rounding of lse (gamma_{C+4} relative in the sum, u |lse| in the final
    addition), of the C arguments (u |z_c - lse| each), of exp (2 u) and of the sum over c; per pixel
        eps(p) = gamma_{C+8} + gamma_4 (|lse| + max_c |z_c - lse|),
    weighted like the pixel itself, plus gamma_{P+C} of the sum of the absolute terms for the accumulation over the P pixels."""
    _gpu()
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, labels, heads = _reference(i, H, False)
    _, G = _cell_pass(i, H, False)
    Ay, Ax = R.tap_matrix(Hl, h), R.tap_matrix(Wl, w)
    touched = (Ay.sum(0) > 0)[:, None] & (Ax.sum(0) > 0)[None, :]
    if i == 6:
        assert int((~touched).sum()) > 0
    for hh, r in enumerate(heads):
        g = G[:, hh * C:(hh + 1) * C].cpu().view(B, h, w, C)
        e = _relF(g, r["G"])
        print(f"SEG-DL case {i} H={H} head {hh}: G relF {e:.2e}")
        assert e <= 1e-5
        assert bool((g[:, ~touched] == 0).all()), "a cell without support must be exactly 0"
        n = r["n_valid"]
        eps = (R.gamma(C + 8) + R.gamma(4) * (r["lse"].abs() + (r["up"] - r["lse"][..., None]).abs().amax(-1))) * r["valid"]
        soft = torch.exp(r["up"] - r["lse"][..., None])
        onehot = torch.zeros_like(soft).scatter_(-1, labels.long().clamp_max(C - 1)[..., None], 1.0)
        terms = ((soft + onehot) * r["valid"][..., None]).sum(-1)
        bound = (torch.einsum("yi,xj,byx->bij", Ay, Ax, eps) + R.gamma(Hl * Wl + C) * torch.einsum("yi,xj,byx->bij", Ay, Ax, terms)) / n
        s = g.double().sum(-1).abs()
        print(f"SEG-DL case {i} H={H} head {hh}: class sums max/bound {float((s / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((s <= bound).all())


@pytest.mark.parametrize("i", [1, 3])
def test_cell_pass_without_a_valid_pixel(i):
    _gpu()
    _, G = _cell_pass(i, 3, True)
    assert bool((G == 0).all()), "no valid pixel: G is 0 everywhere, no NaN from 1 / 0"


# ---------------------------------------------------------------------------------------------------------------- 3. weight step
NHC = {2: (1, 2), 63: (3, 21), 150: (1, 150), 450: (3, 150)}


def _m_values():
    from vtp_amd import ops
    s = ops.seg_sgd_slice()
    return [1, 2, 3, s - 1, s, s + 1, 2 * s + 5]


@pytest.mark.parametrize("mi", range(7))
def test_weight_step_within_the_sliced_chain_bound(mi):
    """One vtp_seg_sgd step from non-zero momentum buffers against fp64.  dW[n, k] is a k-ordered fmaf chain per slice (at most
    `slice` roundings) and the S slices are added in order (S - 1 roundings): |dW - dW_ref| <= gamma_{M+S+3} (|G|^T |X|) =: bd.
    m = fmaf(momentum, m0, dW) rounds once: |m - m_ref| <= bd + 2 u (|m_ref| + bd) =: bm (momentum is the fp32 value the kernel gets),
    W = fmaf(-lr, m, W0) once more: |W - W_ref| <= lr bm + 2 u (|W_ref| + lr bm).  The bias likewise with |G| summed over the rows."""
    _gpu()
    from vtp_amd import ops
    M = _m_values()[mi]
    S = -(-M // ops.seg_sgd_slice())
    mom = float(torch.tensor(0.9, dtype=F32))
    for N, (H, C) in NHC.items():
        for K in (40, 132, 260):
            g = torch.Generator().manual_seed(1000 * mi + N + K)
            Gm, X = 0.1 * torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
            w0, b0 = 0.05 * torch.randn(N, K, generator=g), 0.05 * torch.randn(N, generator=g)
            m0, mb0 = 0.02 * torch.randn(N, K, generator=g), 0.02 * torch.randn(N, generator=g)
            lr = torch.tensor([0.1 * (hh + 1) for hh in range(H)], dtype=F32)
            lr_row = lr.double().repeat_interleave(C)
            Gd = torch.full((M, N + 5), float("nan"), dtype=F32)
            Gd[:, :N] = Gm
            Gd = Gd.to(DEV)[:, :N]

            def guarded(t):  # two rows (entries) of NaN after the tensor proper
                full = torch.full((N + 2, *t.shape[1:]), float("nan"), dtype=F32)
                full[:N] = t
                return full.to(DEV)

            Wd, bd_, mWd, mbd = guarded(w0), guarded(b0), guarded(m0), guarded(mb0)
            nbytes = ops.seg_sgd_workspace_bytes(M, N, K)
            ws = torch.full((nbytes + 64,), 0xA5, device=DEV, dtype=torch.uint8)
            ops.seg_sgd(Wd[:N], bd_[:N], mWd[:N], mbd[:N], Gd, _sliced(X), lr.to(DEV), M, H, C, K, mom, ws[:nbytes])
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
    print(f"SEG-SGD M={M} ({S} slices): within the bound for N in {sorted(NHC)} and K in (40, 132, 260)")


@pytest.mark.parametrize("mi", range(5))
def test_one_slice_has_the_bits_of_probe_sgd(mi):
    """Within one slice vtp_seg_sgd is vtp_probe_sgd: the same G^T X wave tile over the same rows, one partial to fold, the same two
    fmaf lines (csrc/wave_f32.h).  From non-zero momentum buffers, X a column slice of a wider matrix; N = 111 straddles the
    64-row tile and the head boundary."""
    _gpu()
    from vtp_amd import ops
    M = (1, 2, 7, 130, ops.seg_sgd_slice())[mi]
    mom = 0.9
    for H, C in ((1, 7), (3, 37)):
        N = H * C
        for K in (40, 132):
            g = torch.Generator().manual_seed(2000 * mi + N + K)
            Gm, X = 0.1 * torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
            state = [0.05 * torch.randn(N, K, generator=g), 0.05 * torch.randn(N, generator=g),
                     0.02 * torch.randn(N, K, generator=g), 0.02 * torch.randn(N, generator=g)]  # W, bias, mW, mb
            lr = torch.tensor([0.1 * (hh + 1) for hh in range(H)], dtype=F32).to(DEV)
            Gd, Xd = Gm.to(DEV), _sliced(X)
            seg, probe = [t.to(DEV) for t in state], [t.to(DEV) for t in state]
            ws = torch.empty(ops.seg_sgd_workspace_bytes(M, N, K), device=DEV, dtype=torch.uint8)
            ops.seg_sgd(*seg, Gd, Xd, lr, M, H, C, K, mom, ws)
            ops.probe_sgd(*probe, Gd, Xd, lr, M, H, C, K, mom)
            for name, a, b, t0 in zip(("W", "bias", "mW", "mb"), seg, probe, state):
                assert not torch.equal(a.cpu(), t0), (name, "the step changed nothing")
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, M, H, C, K)


# ---------------------------------------------------------------------------------------------------------------- 4. repeatability
def _probe(heads, C, D, seed=0, **kw):
    from vtp_amd import SegProbe
    torch.manual_seed(seed)
    return SegProbe(None, heads, C, embed_dim=D, **kw)


def _batch(B, h, w, Hl, Wl, C, width, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * h * w, width, generator=g)
    y = torch.randint(0, C, (B, Hl, Wl), generator=g)
    y[torch.rand(B, Hl, Wl, generator=g) < 0.1] = 255
    return x.to(DEV), y.to(DEV)


def _state(p):
    return [t.clone() for g in p.groups for t in (g.weight, g.bias, g.m_weight, g.m_bias)]


def test_kernels_repeat_bit_for_bit():
    _gpu()
    (o1, g1), (o2, g2) = _cell_pass(5, 3, False), _cell_pass(5, 3, False)
    assert torch.equal(o1["lse"], o2["lse"]) and torch.equal(o1["loss"], o2["loss"]) and torch.equal(g1, g2)


def test_a_step_repeats_bit_for_bit_and_chunks_of_heads_change_nothing():
    _gpu()
    B, h, w, Hl, Wl, C, D = 3, 4, 5, 40, 52, 21, 32
    heads = [("a", 1, 0.5), ("b", 1, 0.25), ("c", 1, 0.125)]
    runs = []
    for chunk in (None, None, 1, 2):
        p = _probe(heads, C, D, max_iter=10)
        p.head_chunk = chunk
        losses = [p.step_features(*_xyhw(B, h, w, Hl, Wl, C, D, 40 + s)) for s in range(2)]
        runs.append(losses + _state(p))
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


def _xyhw(B, h, w, Hl, Wl, C, width, seed):
    x, y = _batch(B, h, w, Hl, Wl, C, width, seed)
    return x, (h, w), y


def test_evaluation_does_not_depend_on_the_batch_split():
    _gpu()
    B, h, w, Hl, Wl, C, D = 3, 4, 5, 40, 52, 21, 32
    heads = [("a", 1, 0.5), ("b", 2, 0.25)]
    x, hw, y = _xyhw(B, h, w, Hl, Wl, C, 2 * D, 7)
    whole, parts = _probe(heads, C, D), _probe(heads, C, D)
    for p in (whole, parts):
        for g in p.groups:
            g.weight.mul_(30.0)  # away from the all-equal predictions of the 0.01 init
    whole.evaluate_features(x, hw, y)
    M1 = h * w
    parts.evaluate_features(x[:M1], hw, y[:1])
    parts.evaluate_features(x[M1:], hw, y[1:])
    a, b = whole.counts(), parts.counts()
    assert torch.equal(a["confusion"], b["confusion"]) and a["valid"] == b["valid"] == int((y != 255).sum()) and a["out_of_range"] == 0
    assert int(a["confusion"][0].sum()) == a["valid"] and len(set(a["confusion"][0].sum(0).nonzero().flatten().tolist())) > 1
    assert whole.miou() == parts.miou() and whole.best() == parts.best()
    whole.reset_eval()
    assert whole.counts()["valid"] == 0 and int(whole.counts()["confusion"].sum()) == 0


def test_equal_heads_stay_bit_identical():
    _gpu()
    B, h, w, Hl, Wl, C, D = 2, 3, 4, 24, 32, 21, 32
    p = _probe([("a", 1, 0.3), ("b", 1, 0.3), ("c", 1, 0.1)], C, D)
    p.groups[0].weight[1].copy_(p.groups[0].weight[0])
    for s in range(3):
        losses = p.step_features(*_xyhw(B, h, w, Hl, Wl, C, D, 60 + s))
        assert float(losses[0]) == float(losses[1])
    g = p.groups[0]
    for t in (g.weight, g.bias, g.m_weight, g.m_bias):
        assert torch.equal(t[0], t[1]) and not torch.equal(t[0], t[2])


# ---------------------------------------------------------------------------------------------------------------- 5. memory
def test_a_step_allocates_a_fraction_of_the_upsampled_logits():
    """B = 2, 8 x 8 cells, 128 x 128 labels, C = 150, H = 1: the [B, C, Hl, Wl] fp32 tensor torch would hold is 19.7 MB; one step
    may raise the peak by less than a quarter of it (its own arrays -- lse, Z, G, the workspaces -- total well under 2 MB)"""
    _gpu()
    B, h, w, Hl, Wl, C, D = 2, 8, 8, 128, 128, 150, 64
    p = _probe([("a", 1, 0.1)], C, D)
    x, hw, y = _xyhw(B, h, w, Hl, Wl, C, D, 3)
    y = y.to(torch.uint8)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    p.step_features(x, hw, y)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"SEG-MEM: peak rise {rise / 1e6:.2f} MB of {B * C * Hl * Wl * 4 / 1e6:.1f} MB")
    assert rise < B * C * Hl * Wl * 4 / 4


# ---------------------------------------------------------------------------------------------------------------- 6. class level
def test_three_steps_follow_the_fp64_trajectory():
    _gpu()
    B, h, w, Hl, Wl, C, D = 2, 3, 4, 24, 32, 21, 32
    heads = [("one_a", 1, 0.5), ("two", 2, 0.25), ("one_b", 1, 0.1)]
    p = _probe(heads, C, D, max_iter=10)
    assert p.keys == ["one_a", "one_b", "two"] and [g.K for g in p.groups] == [D, 2 * D]
    ref = R.RefSeg(heads, {k: (g.weight[j].cpu(), g.bias[j].cpu()) for g in p.groups for j, k in enumerate(g.keys)}, D, 0.9, 10)
    for s in range(3):
        x, hw, y = _xyhw(B, h, w, Hl, Wl, C, 2 * D, 80 + s)
        if s == 1:
            y = y.to(torch.int32)
            y[0, 0, :4] = torch.tensor([-1, 256, 70000, C], device=DEV)  # no byte: ignored; C: out of range, skipped as well
        got = p.step_features(x, hw, y)
        y_ref = y.cpu().long()
        y_ref[(y_ref < 0) | (y_ref > 255)] = 255
        want = ref.step(x.cpu(), hw, y_ref)
        assert p.learning_rates(s)["two"] == pytest.approx(R.cosine_lr(0.25, s, 10), rel=1e-15)
        for j, k in enumerate(p.keys):
            assert float(got[j]) == pytest.approx(want[k], rel=1e-5), (s, k)
    for g in p.groups:
        for j, k in enumerate(g.keys):
            eW, eb = _relF(g.weight[j], ref.W[k]), _relF(g.bias[j], ref.b[k])
            print(f"SEG-TRAJ {k}: weight relF {eW:.2e} bias relF {eb:.2e}")
            assert eW <= 1e-5 and eb <= 1e-5


def test_planted_problem_is_learned_and_checkpoints_continue_bit_for_bit():
    _gpu()
    B, h, w, Hl, Wl, C, D = 2, 4, 4, 32, 32, 5, 32
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * h * w, D, generator=g)
    hidden = (x.double() @ torch.randn(D, C, generator=g).double()).view(B, h, w, C)
    y = R.upsample(hidden, Hl, Wl).argmax(-1).to(torch.uint8).to(DEV)  # the labels a linear head on these features can reach
    x = x.to(DEV)
    p = _probe([("a", 1, 0.5)], C, D)
    p.evaluate_features(x, (h, w), y)
    miou0 = p.miou()["a"]
    p.reset_eval()
    losses = [float(p.step_features(x, (h, w), y)[0]) for _ in range(20)]
    p.evaluate_features(x, (h, w), y)
    miou1, acc1 = p.miou()["a"], p.pixel_accuracy()["a"]
    print(f"SEG-PLANTED: loss {losses[0]:.4f} -> {losses[-1]:.4f}, mIoU {miou0:.1f} -> {miou1:.1f} %, pixel accuracy {acc1:.1f} %")
    assert losses[-1] < 0.5 * losses[0] and miou1 > miou0 and miou1 > 50.0
    assert set(p.per_class_iou()) == {"a"} and p.best() == ("a", miou1)
    q = _probe([("a", 1, 0.5)], C, D, seed=9)
    q.load_state_dict({k: v.cpu() for k, v in p.state_dict().items()})
    assert q.steps == p.steps == 20
    for _ in range(2):
        assert torch.equal(p.step_features(x, (h, w), y), q.step_features(x, (h, w), y))
    assert all(torch.equal(a, b) for a, b in zip(_state(p), _state(q)))


def test_through_the_tiny_model(golden, golden_sd):
    _gpu()
    from oracle.ref_stubs import TINY
    from vtp_amd import SegProbe, VTPConfig, VTPModel
    model = VTPModel(VTPConfig(**TINY))
    model.load_state_dict(golden_sd, strict=True)
    model = model.to(DEV).eval()
    D, C = TINY["vision_embed_dim"], 7
    images = golden["in.image"].to(DEV)
    B, _, Hi, Wi = images.shape
    h, w = Hi // 16, Wi // 16
    labels = torch.randint(0, C, (B, Hi, Wi), generator=torch.Generator().manual_seed(0)).to(DEV)
    p = SegProbe(model, [("one", 1, 0.1), ("two", 2, 0.1)], C)
    feats = p.features(images)
    outs = model.get_intermediate_layers_feature(images, n=2, norm=True)
    assert tuple(feats.shape) == (B * h * w, 2 * D)
    assert torch.equal(feats, torch.cat([o.reshape(-1, D) for o in outs], dim=1))
    loss = p.step(images, labels)
    ev = p.evaluate(images, labels[:, ::2, ::2].contiguous())  # evaluation at the labels' own size
    assert loss.shape == ev.shape == (2,) and bool(loss.isfinite().all()) and bool(ev.isfinite().all())
    assert p.counts()["valid"] == B * (Hi // 2) * (Wi // 2) and 0.0 <= p.miou()["one"] <= 100.0
