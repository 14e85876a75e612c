"""GPU: the linear-probe kernels (csrc/probe.hip: vtp_probe_logits / vtp_probe_ce / vtp_probe_sgd, exact fp32 on the f32-input MFMA)
and vtp_amd.LinearProbe against fp64 (tests/probe_ref.py), and through the model against the fixture of the real tool.

Bounds.  gamma_n = n u / (1 - n u), u = 2^-24, is the a-priori error of a chain of n fp32 roundings in ANY order: a product summed
over K terms plus a bias obeys |err| <= gamma_{K+1} (|X| |W|^T + |bias|) elementwise.  It is derived, not measured; torch's own
fp32 product sits at a few percent of it and operands rounded to bf16 exceed it several hundred times, so it rejects a wrong
operand layout and a silent precision drop alike.  1e-5 (relative, Frobenius for tensors) is the project's bar for fp32 arithmetic
against fp64 (tests/test_losses_gpu.py)."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

import probe_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
HC = [(1, 7), (3, 37), (2, 1000)]
BS = [1, 5, 33, 130]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _sliced(x, pad=8, off=4):
    """x on the GPU as a column slice (offset `off`, row stride K + pad) of a wider poisoned matrix"""
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=F32)
    wide[:, off:off + x.shape[1]] = x
    return wide.to(DEV)[:, off:off + x.shape[1]]


def _relF(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _ulp(x):
    """spacing of fp32 at x (towards larger magnitude)"""
    far = torch.where(x >= 0, torch.full_like(x, float("inf")), torch.full_like(x, float("-inf")))
    return (torch.nextafter(x, far) - x).abs().double()


# ---------------------------------------------------------------------------------------------------------------- 1. logits
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H,C", HC)
def test_logits_within_the_fp32_chain_bound(B, H, C):
    _gpu()
    from vtp_amd import ops
    N = H * C
    for K in (40, 132, 260):
        x, w, b = _rand(B, K, seed=K + B), _rand(N, K, seed=K + N + 1, scale=0.3), _rand(N, seed=N + 2)
        xs = _sliced(x)
        assert xs.stride(0) == K + 8 and xs.storage_offset() == 4
        out = torch.full((B, N + 3), float("nan"), device=DEV, dtype=F32)
        ops.probe_logits(xs, w.to(DEV), b.to(DEV), out, B, N, K)
        got = out.cpu()
        ref = x.double() @ w.double().T + b.double()
        bound = R.gamma(K + 1) * (x.double().abs() @ w.double().abs().T + b.double().abs())
        err = (got[:, :N].double() - ref).abs()
        print(f"LOGITS B={B} K={K} H={H} C={C}: max err/bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (B, K, H, C, float((err / bound).max()))
        assert bool(got[:, N:].isnan().all()), "wrote past column N"


# ---------------------------------------------------------------------------------------------------------------- 2. cross-entropy
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H,C", HC)
def test_cross_entropy_counts_and_gradient(B, H, C):
    _gpu()
    from vtp_amd import ops
    N, ldl = H * C, H * C + 5
    z = _rand(B, N, seed=B + N, scale=3.0)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(B + C))
    for h in {0, H - 1}:  # row 0: two equal maxima, the label on the LOWER index -> counted; row 1: the label on the higher -> not
        for row, lab in ((0, 2), (1, 5)):
            if row < B:
                z[row, h * C + 2] = z[row, h * C + 5] = z[row, h * C:(h + 1) * C].max() + 1.0
                y[row] = lab
    if B > 2:  # one plain row whose label is its argmax in head 0
        y[2] = int(z[2, :C].argmax())
    zd = torch.full((B, ldl), float("nan"), dtype=F32)
    zd[:, :N] = z
    zd = zd.to(DEV)
    z3 = z.double().view(B, H, C)
    logp = torch.log_softmax(z3, dim=2)
    idx = torch.arange(B)
    loss_ref = -logp[idx, :, y].mean(dim=0)  # [H]
    d_ref = logp.exp()
    d_ref[idx, :, y] -= 1.0
    d_ref = (d_ref / B).reshape(B, N)
    first_max = torch.stack([torch.tensor([int((z3[b, h] == z3[b, h].max()).nonzero()[0]) for h in range(H)]) for b in range(B)])
    correct_ref = (first_max == y[:, None]).sum(dim=0)
    if B > 1:
        assert int(first_max[0, 0]) == 2 and int(y[0]) == 2 and int(first_max[1, 0]) == 2 and int(y[1]) == 5
    loss = torch.full((H,), 1.0, device=DEV, dtype=F32)  # accumulated on top of what is there
    correct = torch.full((H,), 5, device=DEV, dtype=torch.int32)
    dl = torch.full((B, ldl), float("nan"), device=DEV, dtype=F32)
    ops.probe_ce(zd, y.to(DEV), B, H, C, 1.0 / B, loss, correct, None)  # evaluation: no gradient buffer at all
    assert bool(dl.isnan().all())
    assert torch.equal(correct.cpu().long() - 5, correct_ref), (correct.cpu(), correct_ref)
    loss2 = torch.zeros(H, device=DEV, dtype=F32)
    ops.probe_ce(zd, y.to(DEV), B, H, C, 1.0 / B, loss2, None, dl)
    for got in (loss.cpu().double() - 1.0, loss2.cpu().double()):
        rel = ((got - loss_ref).abs() / loss_ref.abs()).max()
        print(f"CE B={B} H={H} C={C}: loss rel err {float(rel):.2e}")
        assert float(rel) <= 1e-5
    assert torch.equal(correct.cpu().long() - 5, correct_ref), "the training call must not count"
    e = _relF(dl[:, :N], d_ref)
    print(f"CE B={B} H={H} C={C}: dlogits relF {e:.2e}")
    assert e <= 1e-5
    assert bool(dl[:, N:].isnan().all()), "wrote past column H * C"


# ---------------------------------------------------------------------------------------------------------------- 3. SGD
def _sgd_case(B, K, H, C, seed=0):
    N = H * C
    x, dl = _rand(B, K, seed=seed + 1), _rand(B, N, seed=seed + 2, scale=0.1)
    w0, b0 = _rand(N, K, seed=seed + 3, scale=0.05), _rand(N, seed=seed + 4, scale=0.05)
    return x, dl, w0, b0


@pytest.mark.parametrize("B,K,H,C", [(1, 40, 1, 7), (5, 132, 3, 37), (33, 260, 3, 37), (130, 40, 3, 37), (130, 132, 2, 1000)])
def test_sgd_gradient_bound_then_fmaf_lines(B, K, H, C):
    _gpu()
    from vtp_amd import ops
    N = H * C
    x, dl, w0, b0 = _sgd_case(B, K, H, C)
    lr = torch.tensor([0.1 * (h + 1) for h in range(H)], dtype=F32)
    lr_row = lr.repeat_interleave(C)
    xs = _sliced(x)
    dld = torch.full((B, N + 5), float("nan"), dtype=F32)
    dld[:, :N] = dl
    dld = dld.to(DEV)[:, :N]
    W, bias = w0.to(DEV).clone(), b0.to(DEV).clone()
    mW, mb = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    # momentum 0 on zeroed buffers: the momentum buffers ARE the gradients
    ops.probe_sgd(W, bias, mW, mb, dld, xs, lr.to(DEV), B, H, C, K, 0.0)
    dW, db = mW.cpu(), mb.cpu()
    dW_ref, db_ref = dl.double().T @ x.double(), dl.double().sum(0)
    eW = (dW.double() - dW_ref).abs()
    bW = R.gamma(B) * (dl.double().abs().T @ x.double().abs())
    eb = (db.double() - db_ref).abs()
    bb = R.gamma(B + 1) * dl.double().abs().sum(0)
    print(f"SGD B={B} K={K} H={H} C={C}: dW err/bound {float((eW / bW).max()):.3f}  db err/bound {float((eb / bb.clamp_min(1e-300)).max()):.3f}")
    assert bool((eW <= bW).all()) and bool((eb <= bb).all())
    W1, b1 = W.cpu(), bias.cpu()
    for got, p0, g, r in ((W1, w0, dW, lr_row[:, None]), (b1, b0, db, lr_row)):
        want = (p0.double() - r.double() * g.double()).float()
        assert bool(((got.double() - want.double()).abs() <= _ulp(want)).all())
    # momentum 0.9 on the kernel's own results: the two fmaf lines in fp64, rounded
    mom = 0.9
    mom32 = float(torch.tensor(mom, dtype=F32))
    ops.probe_sgd(W, bias, mW, mb, dld, xs, lr.to(DEV), B, H, C, K, mom)
    for got_m, got_p, m1, g, p1, r in ((mW.cpu(), W.cpu(), dW, dW, W1, lr_row[:, None]), (mb.cpu(), bias.cpu(), db, db, b1, lr_row)):
        m_want = (mom32 * m1.double() + g.double()).float()
        p_want = (p1.double() - r.double() * m_want.double()).float()
        assert bool(((got_m.double() - m_want.double()).abs() <= _ulp(m_want)).all())
        assert bool(((got_p.double() - p_want.double()).abs() <= _ulp(p_want)).all())


def test_sgd_learning_rate_is_per_head_not_per_tile():
    _gpu()
    from vtp_amd import ops
    B, K, H, C = 5, 132, 3, 37
    x, dl, w0, b0 = _sgd_case(B, K, H, C, seed=7)
    W, bias = w0.to(DEV).clone(), b0.to(DEV).clone()
    mW, mb = torch.zeros(H * C, K, device=DEV), torch.zeros(H * C, device=DEV)
    lr = torch.tensor([0.5, 0.0, 0.25], device=DEV)
    ops.probe_sgd(W, bias, mW, mb, dl.to(DEV), x.to(DEV), lr, B, H, C, K, 0.9)
    W, bias, mW, mb = (t.cpu().view(H, C, -1) for t in (W, bias, mW, mb))
    w0, b0 = w0.view(H, C, K), b0.view(H, C, 1)
    assert torch.equal(W[1], w0[1]) and torch.equal(bias[1], b0[1]), "head 1 has rate 0: its parameters must not change by a bit"
    assert bool((mW[1] != 0).all()) and bool((mb[1] != 0).all()), "its momentum still moves"
    for h in (0, 2):
        assert bool((W[h] != w0[h]).float().mean() > 0.99) and bool((bias[h] != b0[h]).float().mean() > 0.9), h


def test_equal_heads_stay_bit_identical():
    _gpu()
    from vtp_amd import ops
    B, K, H, C = 33, 132, 2, 37
    N = H * C
    x = _rand(B, K, seed=11).to(DEV)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(12)).to(DEV)
    w1, b1 = _rand(C, K, seed=13, scale=0.05), _rand(C, seed=14, scale=0.05)
    W, bias = torch.cat([w1, w1]).to(DEV), torch.cat([b1, b1]).to(DEV)
    mW, mb = torch.zeros_like(W), torch.zeros_like(bias)
    lr = torch.tensor([0.3, 0.3], device=DEV)
    logits, dl, loss = torch.empty(B, N, device=DEV), torch.empty(B, N, device=DEV), torch.zeros(H, device=DEV)
    for _ in range(2):
        ops.probe_logits(x, W, bias, logits, B, N, K)
        ops.probe_ce(logits, y, B, H, C, 1.0 / B, loss, None, dl)
        ops.probe_sgd(W, bias, mW, mb, dl, x, lr, B, H, C, K, 0.9)
    for t in (W, bias, mW, mb, logits.T.contiguous(), dl.T.contiguous()):
        t = t.cpu().view(H, C, -1)
        assert torch.equal(t[0], t[1])
    assert not torch.equal(W.cpu()[:C], w1)


# ---------------------------------------------------------------------------------------------------------------- 4. the sweep
SWEEP_HEADS = [(f"g{n}_lr{i}", n, True, lr) for n in (1, 2) for i, lr in enumerate((0.1, 0.5, 2.0))]
SW = dict(B=8, D=16, C=7, steps=4)


def _sweep_probe(max_iter=SW["steps"], heads=SWEEP_HEADS, group=None):
    from vtp_amd import probe
    p = probe.LinearProbe(None, heads, SW["C"], momentum=0.9, max_iter=max_iter, group=group, embed_dim=SW["D"])
    torch.manual_seed(0)
    init = probe.init_heads(heads, SW["D"], SW["C"])
    p.load_state_dict({f"classifiers_dict.{k}.linear.{n}": t for k, (w, b) in init.items() for n, t in (("weight", w), ("bias", b))})
    return p, init


def _sweep_batch(s):
    x = _rand(SW["B"], 3 * SW["D"], seed=100 + s)
    y = torch.randint(0, SW["C"], (SW["B"],), generator=torch.Generator().manual_seed(200 + s))
    return x, y


def _stacked(ref, attr):
    return torch.cat([getattr(ref, attr)[k].reshape(-1) for k, *_ in ref.heads])


def test_sweep_matches_the_fp64_restatement():
    _gpu()
    p, init = _sweep_probe()
    assert p.keys == [h[0] for h in SWEEP_HEADS] and [g.K for g in p.groups] == [32, 48] and [g.col0 for g in p.groups] == [16, 0]
    ref = R.RefProbe(SWEEP_HEADS, init, SW["D"], 0.9, SW["steps"])
    saved = None
    for s in range(SW["steps"]):
        if s == 2:
            saved = p.state_dict()
        x, y = _sweep_batch(s)
        losses = p.step_features(x.to(DEV), y.to(DEV))
        assert losses.is_cuda and losses.dtype == F32 and losses.shape == (6,)
        want = ref.step(x, y)
        for k, got in zip(p.keys, losses.cpu().tolist()):
            assert got == pytest.approx(want[k], rel=1e-5), (s, k)
        assert p.learning_rates(s) == pytest.approx({k: R.cosine_lr(lr, s, SW["steps"]) for k, _, _, lr in SWEEP_HEADS}, rel=1e-12)
    for mine, theirs in (("weight", "W"), ("bias", "b"), ("m_weight", "mW"), ("m_bias", "mb")):
        got = torch.cat([getattr(g, mine).reshape(-1) for g in p.groups])
        e = _relF(got, _stacked(ref, theirs))
        print(f"SWEEP {mine}: relF {e:.2e}")
        assert e <= 1e-5, mine
    # evaluation: device counts against the restatement's, over two batches; reset clears them
    total = {k: 0 for k in p.keys}
    for s in (7, 8):
        x, y = _sweep_batch(s)
        p.evaluate_features(x.to(DEV), y.to(DEV))
        for k, c in ref.evaluate(x, y).items():
            total[k] += c
    assert p.accuracies() == pytest.approx({k: 100.0 * c / 16 for k, c in total.items()})
    assert p.best()[1] == max(p.accuracies().values())
    p.reset_eval()
    assert int(p.counts()[0].sum()) == 0 and p.counts()[1] == 0
    # checkpoint after two steps -> a fresh object -> the same two further steps: bit-identical to having continued
    assert set(saved) >= {f"classifiers_dict.{k}.linear.{n}" for k in p.keys for n in ("weight", "bias")}
    q, _ = _sweep_probe()
    q.load_state_dict(saved)
    assert q.steps == 2
    for s in (2, 3):
        x, y = _sweep_batch(s)
        q.step_features(x.to(DEV), y.to(DEV))
    for gp, gq in zip(p.groups, q.groups):
        for a in ("weight", "bias", "m_weight", "m_bias"):
            assert torch.equal(getattr(gp, a), getattr(gq, a)), a
    with pytest.raises(ValueError, match="CPU"):
        p.step_features(x, y.to(DEV))


def test_key_collision_keeps_the_later_head():
    _gpu()
    from vtp_amd import probe
    heads = [("k", 1, True, 0.1), ("j", 1, True, 0.2), ("k", 1, True, 0.3)]
    torch.manual_seed(4)
    p = probe.LinearProbe(None, heads, SW["C"], embed_dim=SW["D"])
    torch.manual_seed(4)
    draws = [torch.nn.Linear(2 * SW["D"], SW["C"]).weight.data.normal_(0.0, 0.01).clone() for _ in heads]
    assert p.keys == ["k", "j"] and p.learning_rates() == {"k": 0.3, "j": 0.2}
    assert len(p.groups) == 1 and p.groups[0].weight.shape == (2, SW["C"], 2 * SW["D"])
    assert torch.equal(p.groups[0].weight[0].cpu(), draws[2]) and torch.equal(p.groups[0].weight[1].cpu(), draws[1])
    sweep = probe.LinearProbe.from_sweep(None, num_classes=3, embed_dim=4)
    assert len(sweep.keys) == 24 and [g.H for g in sweep.groups] == [12, 12] and [g.K for g in sweep.groups] == [8, 20]
    assert sweep.learning_rates()["classifier_1_blocks_avgpool_True_lr_0_00001"] == pytest.approx(1e-5)


# ---------------------------------------------------------------------------------------------------------------- 5. through the model
def test_probe_through_the_model_against_the_tool_fixture(golden_sd):
    """the lp.losses / lp.w_after part of tests/test_tools_gpu.py with LinearProbe in place of nn.Linear + torch.optim.SGD: same
    inputs, same seeded classifier weights, same four batches, same bars (the model's bf16 noise dominates)."""
    _gpu()
    from safetensors.torch import load_file
    from oracle import tools_oracle as T
    from oracle.ref_stubs import TINY
    from vtp_amd import LinearProbe, VTPConfig, VTPModel
    tg = load_file(os.path.join(ROOT, "tests", "golden", "tools_tiny.safetensors"))
    images, targets = tg["in.images"], tg["in.targets"]
    D, C = TINY["vision_embed_dim"], len(T.CLASSNAMES)

    def seeded():
        torch.manual_seed(0)
        return {"blocks_1_avgpool_True": T.LinearClassifier(2 * D, 1, True, C), "blocks_2_avgpool_False": T.LinearClassifier(2 * D, 2, False, C)}

    def batches(dev):
        return [(images[:4].to(dev), targets[:4].to(dev)), (images[4:].to(dev), targets[4:].to(dev))] * 2

    model = VTPModel(VTPConfig(**TINY))
    model.load_state_dict(golden_sd, strict=True)
    model = model.to(DEV).eval()
    probe = LinearProbe(model, [("blocks_1_avgpool_True", 1, True, 0.1), ("blocks_2_avgpool_False", 2, False, 0.1)], C, max_iter=None)
    probe.load_state_dict({f"classifiers_dict.{k}.{n}": v for k, m in seeded().items() for n, v in m.state_dict().items()})
    ours_losses = torch.tensor([float(probe.step(im, lb).sum()) for im, lb in batches(DEV)])
    ours_w = probe.state_dict()["classifiers_dict.blocks_1_avgpool_True.linear.weight"].cpu()
    # E_ref: the same plumbing on the oracle model under CPU bf16 autocast, the classifiers' arithmetic in fp32
    noisy_clfs = seeded()
    fe = T.FeatureExtractor(T.OracleModel(golden_sd, 2, 2, 2, autocast_dtype=torch.bfloat16), n_last_blocks=2)
    noisy_losses = torch.tensor(T.probe_train_steps(fe, noisy_clfs, batches("cpu")))
    noisy_w = noisy_clfs["blocks_1_avgpool_True"].linear.weight.detach()
    ref_w, ref_losses = tg["out.lp.w_after"], tg["out.lp.losses"]
    e, e_ref = _relF(ours_w, ref_w), _relF(noisy_w, ref_w)
    print(f"PROBE lp.w_after: E_ours={e:.3e} E_ref={e_ref:.3e} ratio={e / e_ref:.2f}")
    assert ours_w.shape == ref_w.shape and e <= 1.5 * e_ref, (e, e_ref)
    e, e_ref = float((ours_losses - ref_losses).abs().max()), float((noisy_losses - ref_losses).abs().max())
    print(f"PROBE lp.losses: max|err| ours={e:.3e} ref={e_ref:.3e}  values ours={[round(float(v), 4) for v in ours_losses]}")
    assert e <= max(2.0 * e_ref, 5e-4), (e, e_ref)
    with pytest.raises(ValueError, match="MI355X"):
        probe.step(images[:4], targets[:4].to(DEV))


# ---------------------------------------------------------------------------------------------------------------- 6. two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    p, _ = _sweep_probe(max_iter=None, group=dist.group.WORLD)
    x, y = _sweep_batch(0)
    half = SW["B"] // world
    sl = slice(rank * half, (rank + 1) * half)
    loss = p.step_features(x[sl].to(DEV), y[sl].to(DEV))
    p.evaluate_features(x[sl].to(DEV), y[sl].to(DEV))
    correct, total = p.counts()
    out[rank] = (loss.cpu(), {k: v.cpu() for k, v in p.state_dict().items()}, correct, total)
    dist.destroy_process_group()


def test_two_ranks_match_one_process_on_the_whole_batch():
    """each rank holds half of a batch of 8; X_all and dlogits are all-gathered and every rank runs the full-batch update: replicas
    bit-identical, and equal to the one-process step within the reordering bound of the weight gradient (2 gamma_B |dlogits|^T |X|
    times the learning rate, plus the rounding of the parameter itself)."""
    _gpu()
    p, init = _sweep_probe(max_iter=None)
    x, y = _sweep_batch(0)
    loss = p.step_features(x.to(DEV), y.to(DEV)).cpu()
    p.evaluate_features(x.to(DEV), y.to(DEV))
    one = {k: v.cpu() for k, v in p.state_dict().items()}
    one_correct, one_total = p.counts()
    ref = R.RefProbe(SWEEP_HEADS, init, SW["D"], 0.9, None)
    z = ref.logits(x)
    del p
    torch.cuda.empty_cache()
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    (l0, s0, c0, t0), (l1, s1, c1, t1) = out[0], out[1]
    for k in s0:
        assert torch.equal(s0[k], s1[k]), f"ranks diverged in {k}"
    assert torch.equal(l0, l1) and torch.allclose(l0, loss, rtol=1e-6, atol=0)
    assert torch.equal(c0, c1) and torch.equal(c0, one_correct) and t0 == t1 == one_total == SW["B"]
    B = SW["B"]
    for key, n, ap, lr in SWEEP_HEADS:
        dz = torch.softmax(z[key], dim=1)
        dz[torch.arange(B), y] -= 1.0
        dz = (dz / B).abs()
        xa = R.head_input(x.double(), 2, SW["D"], n, ap).abs()
        for name, g_abs in (("weight", dz.T @ xa), ("bias", dz.sum(0))):
            a, b = s0[f"classifiers_dict.{key}.linear.{name}"], one[f"classifiers_dict.{key}.linear.{name}"]
            bound = 2 * lr * R.gamma(B + 1) * g_abs + _ulp(b)
            assert bool(((a.double() - b.double()).abs() <= bound).all()), (key, name)
