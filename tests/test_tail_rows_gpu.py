"""Tail rows of the trunk's last block (engine.Stack.forward `tail`): the row-map kernels, the norm backward with a mapped residual
gradient, the grouped weight-gradient launch with a token count per problem, and the training step with the plan on and off.

Kernel level: the row kernels are copies -- bit-exact against torch indexing; vtp_norm_bwd_rows against vtp_norm_bwd fed the expanded
residual gradient (bit-exact rows; the atomically summed dw / db / column sums at the bar of test_kernels_gpu.test_norm_fwd_bwd); the
grouped launch against one ops.gemm_tn per problem at the measure and bar of tests/test_gemm4w_tn_gpu.py.
Step level: the configuration of tests/test_parity_ssl_gpu.py (its Case, its oracle, its bars), one eager step and two graph replays
with fresh masks, VTP_TAIL_ROWS on and off from identical state."""
import os

import numpy as np
import pytest
import torch

from test_kernels_gpu import DEV, bf, check, ops  # noqa: F401  (same helpers / tolerance)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------------------- row kernels
def _plan(M, L, T, g, n_pad):
    """T distinct rows of [0, M - L), the last full row first and the others in random order, n_pad of the others set to -1"""
    rows = torch.cat([torch.tensor([M - L - 1]), torch.randperm(M - L - 1, generator=g)[:T - 1]]).to(torch.int32)
    if n_pad:
        rows[torch.randperm(T - 1, generator=g)[:n_pad] + 1] = -1
    return rows


@pytest.mark.parametrize("M,L,T,D,n_pad", [(300, 37, 41, 256, 5), (70, 0, 9, 768, 2), (515, 257, 258, 384, 0), (64, 63, 1, 128, 0)])
def test_row_map_gather_expand_bit_exact(M, L, T, D, n_pad):
    o = ops()
    g = torch.Generator().manual_seed(M + T)
    idx_h = _plan(M, L, T, g, n_pad)
    idx = idx_h.to(DEV)
    Mc = L + T
    src = torch.cat([torch.arange(L), torch.where(idx_h >= 0, idx_h.long() + L, torch.full((T,), -1))]).to(DEV)  # compact -> full row
    xo = bf(torch.randn(M, D, generator=g)).to(DEV)
    xf = torch.randn(M, D, generator=g).to(DEV)
    # gather: bf16 and f32 rows in one launch, zero rows for the padding
    o_c = torch.full((Mc, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    x_c = torch.full((Mc, D), float("nan"), device=DEV)
    o.gather_tail_rows(xo, xf, idx, o_c, x_c, T, L, M, D)
    keep = (src >= 0)[:, None]
    ref_o = torch.where(keep, xo[src.clamp_min(0)], torch.zeros((), dtype=torch.bfloat16, device=DEV))
    ref_x = torch.where(keep, xf[src.clamp_min(0)], torch.zeros((), device=DEV))
    assert torch.equal(o_c.view(torch.int16), ref_o.view(torch.int16)) and torch.equal(x_c.view(torch.int32), ref_x.view(torch.int32))
    only = torch.full((Mc, D), float("nan"), dtype=torch.bfloat16, device=DEV)  # either pair alone
    o.gather_tail_rows(xo, None, idx, only, None, T, L, M, D)
    assert torch.equal(only.view(torch.int16), ref_o.view(torch.int16))
    # row map: the inverse of `src`, built on the device from the index array alone
    row_map = torch.full((M,), 12345, dtype=torch.int32, device=DEV)
    o.tail_row_map(idx, row_map, T, L, M)
    ref_map = torch.full((M,), -1, dtype=torch.int32, device=DEV)
    ref_map[src[src >= 0]] = torch.arange(Mc, dtype=torch.int32, device=DEV)[src >= 0]
    assert torch.equal(row_map, ref_map)
    assert int(row_map[M - 1]) >= 0, "the case maps the last row"
    from vtp_amd.ssl_engine import tail_row_map
    assert np.array_equal(tail_row_map(idx_h.numpy(), L, M), ref_map.cpu().numpy())
    # expand: every row of dst written in one pass, zeros where nothing maps
    d_c = bf(torch.randn(Mc, D, generator=g)).to(DEV)
    dst = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    o.expand_rows_bf16(d_c, row_map, dst, M, Mc, D)
    ref_d = torch.where((ref_map >= 0)[:, None], d_c[ref_map.clamp_min(0).long()], torch.zeros((), dtype=torch.bfloat16, device=DEV))
    assert torch.equal(dst.view(torch.int16), ref_d.view(torch.int16))


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("D", [256, 768, 1024, 772])  # 1024, 772: four chunks (full, ragged) -- the mapped row is read after the reductions
def test_norm_bwd_mapped_residual_gradient(kind, D):
    """M = 70 rows of which 9 take a residual-gradient row of the compact buffer"""
    o = ops()
    M, Mc = 70, 9
    g = torch.Generator(device=DEV).manual_seed(D + kind)
    x = torch.randn(M, D, device=DEV, generator=g) * 2 + 0.3
    w = torch.rand(D, device=DEV, generator=g) + 0.5
    b = torch.randn(D, device=DEV, generator=g) * 0.1 if kind else None
    y = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    st = torch.empty(M, 2, device=DEV)
    o.norm_fwd(x, w, b, y, st, M, D, 1e-5, kind)
    dy = bf(torch.randn(M, D, device=DEV, generator=g))
    dres_c = torch.randn(Mc, D, device=DEV, generator=g)
    rows = torch.full((M,), -1, dtype=torch.int32)
    rows[torch.tensor([0, 3, 4, 17, 33, 34, 35, 68, 69])] = torch.randperm(Mc, generator=torch.Generator().manual_seed(D)).to(torch.int32)
    rows = rows.to(DEV)
    dres_full = torch.zeros(M, D, device=DEV)
    dres_full[rows >= 0] = dres_c[rows[rows >= 0].long()]
    res = []
    for mapped in (False, True):
        dx = torch.full((M, D), float("nan"), device=DEV)
        dxb = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=DEV)
        dw = torch.zeros(D, device=DEV)
        db = torch.zeros(D, device=DEV) if kind else None
        dxs = torch.full((D,), 3.0, device=DEV)
        if mapped:
            o.norm_bwd_rows(dy, x, w, st, dres_c, rows, dx, dxb, dw, db, M, D, kind, dx_colsum=dxs)
        else:
            o.norm_bwd(dy, x, w, st, dres_full, dx, dxb, dw, db, M, D, kind, dx_colsum=dxs)
        res.append((dx, dxb, dw, db, dxs))
    (dx0, dxb0, dw0, db0, dxs0), (dx1, dxb1, dw1, db1, dxs1) = res
    assert torch.equal(dx1.view(torch.int32), dx0.view(torch.int32)), "dx must be bit-identical"
    assert torch.equal(dxb1.view(torch.int16), dxb0.view(torch.int16)), "the bf16 copy must be bit-identical"
    check(dw1, dw0, "norm_bwd_rows dw", bf16_out=False, scale=1e-4)
    check(dxs1, dxs0, "norm_bwd_rows dx_colsum", bf16_out=False, scale=1e-4)
    if kind:
        check(db1, db0, "norm_bwd_rows db", bf16_out=False, scale=1e-4)


@pytest.mark.parametrize("bias", [False, True])
def test_grouped_wgrad_token_count_per_problem(bias):
    """four problems over (1280, 448, 448, 72) token rows in ONE launch against one ops.gemm_tn each.  Every operand carries NaN rows
    behind its own token count: a k row staged from beyond it would poison the result."""
    o = ops()
    g = torch.Generator(device=DEV).manual_seed(11 + bias)
    shapes = [(512, 256, 1280), (256, 512, 448), (512, 512, 448), (256, 256, 72)]  # (N, K, token rows)
    grp = o.WgradGroup(1280)
    probs = []
    for N, K, kt in shapes:
        a = torch.full((kt + 136, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        x = torch.full((kt + 136, K), float("nan"), dtype=torch.bfloat16, device=DEV)
        a[:kt] = bf(torch.randn(kt, N, device=DEV, generator=g))
        x[:kt] = bf(torch.randn(kt, K, device=DEV, generator=g))
        gw0 = torch.randn(N * K, device=DEV, generator=g)
        gb0 = torch.randn(N, device=DEV, generator=g) if bias else None
        gw, gb = gw0.clone(), None if gb0 is None else gb0.clone()
        grp.add(a, x, gw, gb, N, K, Ktok=kt)
        probs.append((a, x, N, K, kt, gw0, gb0, gw, gb))
    scratch = {}
    grp.finalize(DEV, scratch)
    assert grp.mixed and grp.kernel == 1
    with pytest.raises(ValueError):
        grp.launch(kernel=0)  # the uniform-grid kernel takes one token count
    grp.launch()
    torch.cuda.synchronize()
    if grp.slots > 1:
        assert int(scratch["ticket"].abs().sum()) == 0, "tickets must return to zero"
    for a, x, N, K, kt, gw0, gb0, gw, gb in probs:
        ref = torch.zeros(N, K, device=DEV)
        cs = torch.zeros(N, device=DEV)
        o.gemm_tn(a, x, ref, M=N, N=K, K=kt, lda=N, ldb=K, ldc=K, epi=o.EPI_F32, a_colsum=cs)
        check(gw.view(N, K), gw0.view(N, K) + ref, f"mixed grouped dW N={N} K={K} rows={kt}", bf16_out=False, scale=1e-4)
        if bias:
            check(gb, gb0 + cs, f"mixed grouped db N={N} rows={kt}", bf16_out=False, scale=1e-4)


# ------------------------------------------------------------------------------------------------------------- the step
def _regrouped(model):
    """the sums over rows whose grouping the plan changes: the last block's proj / w12 / w3 weight and bias gradients, its norm2 and
    the final norm"""
    last = f"trunk.blocks.{model.config.vision_depth - 1}."
    names = [n for n, _ in model.named_parameters()]
    return [n for n in names if n.startswith("trunk.norm.") or (n.startswith(last) and (
        n.startswith(last + "attn.proj.") or n.startswith(last + "mlp.") or n.startswith(last + "norm2.")))]


def _snapshot(c, tr, ssl):
    torch.cuda.synchronize()
    Ts, Tt, K = ssl["plan"]["Ts"], 4 + ssl["plan"]["Tm"], tr.ssl_head.K
    snap = {"loss.rec": tr.loss_sum.clone(), "loss.clip": tr.clip_loss_sum.clone(), "loss.ssl": tr.ssl_loss_sum.clone(),
            "logits.student": c.model._head.workspace(Ts, "student").get("logits", (Ts, K), torch.bfloat16).clone(),
            "logits.teacher": c.model._t_head.workspace(Tt, "teacher").get("logits", (Tt, K), torch.bfloat16).clone()}
    for n, p in c.model.named_parameters():
        if p.grad is not None and not n.startswith("teacher_"):
            snap["grad." + n] = p.grad.detach().clone()
    return snap


def _run(c, tail: bool, graphs: bool, mask_seeds):
    """steps from identical state (lr 0, EMA momentum 1, the Case's centres): [snapshot per step]"""
    from test_parity_ssl_gpu import _trainer
    from vtp_amd.data import collate_ssl_masks
    os.environ["VTP_TAIL_ROWS"] = "1" if tail else "0"
    try:
        tr, ssl0 = _trainer(c, use_graphs=graphs)
        out = []
        for seed in mask_seeds:
            if seed is None:
                ssl = ssl0
            else:
                col = collate_ssl_masks(4, (16, 16), 0.5, (0.1, 0.5), np.random.default_rng(seed))
                assert col["upperbound"] == c.col["upperbound"]
                ssl = tr.prepare_ssl(c.gc.to(DEV), c.lc.to(DEV), col["masks"], upperbound=col["upperbound"])
            tr.center_dino.copy_(c.c_d)
            tr.center_ibot.copy_(c.c_i)
            tr.step(c.img.to(DEV), c.txt.to(DEV), ssl)
            used = c.model._trunk.ctx().Mc < c.model._trunk.ctx().M
            assert used == tail, "the plan must be taken exactly when the switch is on"
            out.append(_snapshot(c, tr, ssl))
        return out
    finally:
        os.environ.pop("VTP_TAIL_ROWS", None)


def test_step_with_and_without_tail_rows():
    from test_parity_ssl_gpu import _compare_grads, case
    c = case()
    regrouped = {"grad." + n for n in _regrouped(c.model)}
    assert len(regrouped) >= 10
    full_a, full_b, tail = _run(c, False, False, [None])[0], _run(c, False, False, [None])[0], _run(c, True, False, [None])[0]
    # Deterministic today, by construction: the logits (GEMM chains without split-K) and the weight gradients of the linear layers -- at
    # this token count no weight-gradient tile has more than two K slices, and the sum of two partials does not depend on which
    # arrives last.  Bias / gain / token / embedding gradients and the loss values are sums of atomics in launch order: they differ
    # from run to run on the full path already.  Two runs of the full path confirm the classification.
    stable = [k for k in full_a if torch.equal(full_a[k], full_b[k])]
    print(f"TAIL ROWS: {len(stable)} of {len(full_a)} step outputs repeat bit for bit on the full path")
    linear = [k for k, t in full_a.items() if k.startswith("grad.") and k.endswith(".weight") and t.ndim == 2 and "embedding" not in k]
    must = [k for k in ["logits.student", "logits.teacher"] + linear if k not in regrouped]
    assert len(must) > 100 and not [k for k in must if k not in stable], [k for k in must if k not in stable][:5]

    def same(a, b, what):
        bad = [k for k in must if not torch.equal(a[k], b[k])]
        assert not bad, f"{what}: {len(bad)} outputs differ with the row plan on, e.g. {bad[:5]}"

    same(full_a, tail, "eager step")
    # the losses: the same addends (the logits are bit-identical), all of one sign, summed by atomics in launch order -- two orders of n
    # positive fp32 addends differ by at most 2 (n - 1) 2^-24 of the sum; n <= 4096 rows / workgroups here
    for k in ("loss.rec", "loss.clip", "loss.ssl"):
        a, b = float(full_a[k]), float(tail[k])
        print(f"TAIL ROWS {k}: full {a!r} tail {b!r}")
        assert abs(a - b) <= 2 * 4096 * 2.0 ** -24 * abs(a), k
    # the regrouped sums of BOTH paths against the oracle, at the bars of the parity test
    params = dict(c.model.named_parameters())
    keys = sorted(k[5:] for k in regrouped if k[5:] in c.grads_full["f32"])
    for tag, snap in (("full path", full_a), ("tail rows", tail)):
        holder = {k: type("G", (), {"grad": snap["grad." + k]})() for k in params if "grad." + k in snap}
        _compare_grads(f"TAIL ROWS {tag}", holder, keys, c.grads_full)
    # two graph replays with fresh masks
    g_full, g_tail = _run(c, False, True, [101, 102]), _run(c, True, True, [101, 102])
    for i in range(2):
        same(g_full[i], g_tail[i], f"graph replay {i}")
    assert not torch.equal(g_tail[0]["logits.student"], g_tail[1]["logits.student"]), "the replays saw different masks"
