"""VTPTrainer(skip_nonfinite=True): a step whose global gradient norm is inf or NaN updates nothing.  The guarded finalize (decision,
counters, device-side Adam bias corrections) and the guarded AdamW / EMA kernels on flat buffers, then the trainer: good / bad / good
steps (eager and hipGraphs), guard on against guard off, the SSL step, the checkpoint, and two gloo ranks with the sharded optimizer
where only one rank's batch is bad.  "Unchanged" and "equal" mean the same bits.

The tests that compare two separate trainers bit for bit take rec-only steps on ONE 48 x 48 image, as tests/test_param_groups_gpu.py
does: no address of the backward's float atomics has more than two contributors there, so two runs of a step give the same bits (on
4 images of 64 x 64 they do not, guard or no guard)."""
import math

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_ddp_gpu import _build, _data, _free_port
from test_grad_clip_gpu import _ssl_inputs
from test_ssl_gpu import DEV, build_vtp, sslg  # noqa: F401  (fixture + helpers)

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cpu, cuda = torch.get_rng_state(), torch.cuda.get_rng_state()  # model construction draws from the global generators
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(cuda)


def _bits(t):
    """the tensor's bits as integers: NaN payloads and the sign of zero count"""
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ulps(a: np.float32, b: np.float32) -> int:
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ---- 1. the finalize decision -------------------------------------------------------------------------------------------------
N_FIN = 8192 + 4  # two partials, the second from a 4-element tail


def _partials(x):
    from vtp_amd import ops
    cnt = ops.sumsq_partials_count(x.numel())
    parts = torch.zeros(cnt, dtype=torch.float64, device=DEV)
    ops.sumsq_partials(x, x.numel(), parts)
    return parts, cnt


def _fin_x():
    return torch.randn(N_FIN, device=DEV, generator=torch.Generator(device=DEV).manual_seed(21)) * 3e-2


def _guarded(parts, cnt, gs, max_norm, state0, betas=(0.9, 0.95)):
    from vtp_amd import ops
    hyper = torch.zeros(16, device=DEV)
    hyper[5], hyper[6], hyper[7], hyper[10] = 0.125, 0.25, gs, max_norm
    norm, coef = torch.full((1,), -1.0, device=DEV), torch.full((1,), -1.0, device=DEV)
    state = torch.tensor(state0, dtype=torch.int32, device=DEV)
    ops.grad_clip_finalize_guarded(parts, cnt, hyper, norm, coef, state, betas)
    torch.cuda.synchronize()
    return hyper, norm, coef, state.tolist()


@pytest.mark.parametrize("gs,max_norm", [(1.0, 1e-2), (0.5, INF)])
def test_finalize_finite_is_the_unguarded_finalize(gs, max_norm):
    from vtp_amd import ops
    parts, cnt = _partials(_fin_x())
    assert cnt == 2
    hyper, norm, coef, state = _guarded(parts, cnt, gs, max_norm, [5, 2, 1, 0])
    ref_h = torch.zeros(16, device=DEV)
    ref_h[7], ref_h[10] = gs, max_norm
    ref_norm, ref_coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ops.grad_clip_finalize(parts, cnt, ref_h, ref_norm, ref_coef)
    torch.cuda.synchronize()
    assert state == [6, 2, 0, 0]
    assert math.isfinite(float(norm)) and float(norm) > 0
    assert _same(norm, ref_norm) and _same(coef, ref_coef) and _same(hyper[7:8], ref_h[7:8])
    assert _ulps(hyper[5].cpu().numpy(), np.float32(1 - 0.9 ** 6)) <= 1  # t = applied_steps after the increment
    assert _ulps(hyper[6].cpu().numpy(), np.float32((1 - 0.95 ** 6) ** 0.5)) <= 1
    assert (max_norm == INF) == (float(coef) == 1.0)


@pytest.mark.parametrize("case", ["nan_last", "inf_first", "neg_inf_mid", "f32_overflow"])
def test_finalize_non_finite_skips(case):
    x, gs = _fin_x(), 0.5
    if case == "nan_last":
        x[N_FIN - 1] = float("nan")
    elif case == "inf_first":
        x[0] = INF
    elif case == "neg_inf_mid":
        x[N_FIN // 2] = -INF
    else:  # every element and the fp64 sum are finite; gs * sqrt(sum) is not an f32
        gs = 3e38
    parts, cnt = _partials(x)
    if case == "f32_overflow":
        assert math.isfinite(float(parts.sum())) and float(parts.sum()) > 4.0
    hyper, norm, coef, state = _guarded(parts, cnt, gs, 1.0, [5, 2, 0, 0])
    assert state == [5, 3, 1, 0]
    assert not math.isfinite(float(norm))
    assert _same(hyper[7:8], torch.tensor([gs], device=DEV)), "a skipped step must leave the gradient multiplier alone"
    assert math.isnan(float(coef)) if case == "nan_last" else float(coef) == 0.0  # reported as torch would


# ---- 2. Adam's bias corrections from the device counter -----------------------------------------------------------------------
@pytest.mark.parametrize("betas", [(0.5, 0.75), (0.9, 0.95)])
def test_bias_corrections_follow_the_applied_count(betas):
    """t = 1 .. 40 with one skipped call after t = 20: the call behind it produces t = 21.  (0.5, 0.75): 0.5^t is exact in fp64, so
    hyper[5] is the host value bit for bit.  Otherwise device and host round fp64 values that agree to a few fp64 ulps (the power by
    squaring against libm's pow; sqrt against ** 0.5) to f32: at most 1 f32 ulp apart."""
    from vtp_amd import ops
    good, cnt = _partials(_fin_x())
    x = _fin_x()
    x[7] = float("nan")
    bad, _ = _partials(x)
    hyper = torch.zeros(16, device=DEV)
    hyper[7], hyper[10] = 1.0, INF
    norm, coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    got = []
    for t in range(1, 41):
        ops.grad_clip_finalize_guarded(good, cnt, hyper, norm, coef, state, betas)
        got.append(hyper[5:7].clone())
        if t == 20:
            ops.grad_clip_finalize_guarded(bad, cnt, hyper, norm, coef, state, betas)
            skipped_state = state.clone()
    torch.cuda.synchronize()
    assert skipped_state.tolist() == [20, 1, 1, 0] and state.tolist() == [40, 1, 0, 0]
    assert float(hyper[7]) == 1.0
    b1, b2 = betas
    for t, h in enumerate(torch.stack(got).cpu().numpy(), start=1):
        bc1, bc2 = np.float32(1.0 - b1 ** t), np.float32((1.0 - b2 ** t) ** 0.5)
        if b1 == 0.5:
            assert h[0].view(np.int32) == bc1.view(np.int32), (t, h[0], bc1)
        assert _ulps(h[0], bc1) <= 1 and _ulps(h[1], bc2) <= 1, (t, h, bc1, bc2)


# ---- 3. the guarded update kernels ---------------------------------------------------------------------------------------------
def _opt_inputs(n):
    g = torch.Generator(device=DEV).manual_seed(100 + n)
    p, grad, m = (torch.randn(n, device=DEV, generator=g) for _ in range(3))
    v = torch.rand(n, device=DEV, generator=g) * 1e-2
    teacher = torch.randn(n, device=DEV, generator=g)
    p[1], teacher[0], m[3] = -0.0, -0.0, -0.0
    grad[2] = float("nan")
    pb = p.to(torch.bfloat16)
    hyper = torch.zeros(16, device=DEV)
    hyper[:10] = torch.tensor([1e-3, 0.9, 0.95, 1e-8, 0.05, 1 - 0.9 ** 3, (1 - 0.95 ** 3) ** 0.5, 0.5, 0.0, 0.99])
    flags = (torch.arange(n // 4, device=DEV) % 3 == 0).to(torch.uint8)
    group4 = (torch.arange(n // 4, device=DEV) % 3).to(torch.uint8)
    tab = torch.tensor([[1.0, 1.0], [0.5, 0.0], [0.0, 2.0]], device=DEV)
    return dict(p=p, g=grad, m=m, v=v, teacher=teacher, pb=pb, hyper=hyper, flags=flags, group4=group4, tab=tab)


def _run_update(kind, table, n, skip):
    """skip None: the unguarded entry point; else the guarded one with that value in the device word.  Returns the buffers it may write."""
    from vtp_amd import ops
    d = _opt_inputs(n)
    p, g, m, v, hyper = d["p"], d["g"], d["m"], d["v"], d["hyper"]
    idx4, tab, ng = (d["group4"], d["tab"], 3) if table else (d["flags"], None, 0)
    word = None if skip is None else torch.tensor([skip], dtype=torch.int32, device=DEV)
    if kind == "bf16":
        if skip is not None:
            ops.adamw_dev_guarded(p, g, m, v, d["pb"], n, hyper, word, idx4, tab, ng)
        elif table:
            ops.adamw_dev_grouped(p, g, m, v, d["pb"], n, hyper, idx4, tab, ng)
        else:
            ops.adamw_dev(p, g, m, v, d["pb"], n, hyper, idx4)
    else:
        teacher = d["teacher"] if kind == "ema" else None
        if skip is not None:
            ops.adamw_ema_dev_guarded(p, g, m, v, teacher, n, hyper, word, idx4, tab, ng)
        elif table:
            ops.adamw_ema_dev_grouped(p, g, m, v, teacher, n, hyper, idx4, tab, ng)
        else:
            ops.adamw_ema_dev(p, g, m, v, teacher, n, hyper, idx4)
    torch.cuda.synchronize()
    return [p, m, v, d["pb"], d["teacher"]]


NS = [4, 4096 + 4, 8192]  # one float4; two workgroups of the short-lived kernel, the second nearly empty; two full ones


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", ["bf16", "ema", "no_teacher"])
def test_guarded_adamw_stores_nothing_or_everything(kind, table, n):
    d = _opt_inputs(n)
    before = [d["p"], d["m"], d["v"], d["pb"], d["teacher"]]
    names = ["p", "m", "v", "p_bf16", "teacher"]
    for name, a, b in zip(names, _run_update(kind, table, n, 1), before):
        assert _same(a, b), f"skip = 1 changed {name}"
    plain, guarded = _run_update(kind, table, n, None), _run_update(kind, table, n, 0)
    for name, a, b in zip(names, guarded, plain):
        assert _same(a, b), f"skip = 0: {name} differs from the unguarded entry point"
    assert not _same(plain[0], before[0]) and not _same(plain[1], before[1])  # (the update does move p and m)
    if kind == "ema":
        assert not _same(plain[4], before[4])


@pytest.mark.parametrize("n", NS)
def test_guarded_ema_stores_nothing_or_everything(n):
    from vtp_amd import ops
    out = {}
    for skip in (None, 0, 1):
        d = _opt_inputs(n)
        d["p"][2] = float("nan")
        if skip is None:
            ops.ema_dev(d["teacher"], d["p"], n, d["hyper"][9:10])
        else:
            ops.ema_dev_guarded(d["teacher"], d["p"], n, d["hyper"][9:10], torch.tensor([skip], dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        out[skip] = d["teacher"]
    before = _opt_inputs(n)["teacher"]
    assert _same(out[1], before)
    assert _same(out[0], out[None]) and not _same(out[None], before)


# ---- 4. - 7. the trainer ---------------------------------------------------------------------------------------------------------
def _images(one=True):
    """good, bad, good.  one: ONE 48 x 48 image (two runs of a rec-only step on it agree bit for bit, see the module docstring);
    else the four 64 x 64 images that go with _data()'s captions"""
    img, _ = _data()
    good0 = (img[:1, :, :48, :48].contiguous() if one else img).cuda()
    good1 = good0 + 0.01
    bad = good0.clone()
    bad[-1, 2, 17, 5] = float("nan")  # one pixel: NaN activations meet finite dY in the weight-gradient GEMMs (NaN * 0 = NaN)
    return good0, bad, good1


def _trainer(m, **kw):
    from vtp_amd import VTPTrainer
    kw.setdefault("max_grad_norm", INF)
    kw.setdefault("skip_nonfinite", True)
    return VTPTrainer(m, lr=1e-3, weight_decay=0.01, **kw)  # (stochastic depth and RoPE augmentation off: no host RNG)


def _snapshot(tr):
    st = tr.store
    return [st.flat_p.clone(), tr.m.clone(), tr.v.clone(), st.flat_bf16.clone()]


SNAP_NAMES = ["flat_p (student + teacher)", "exp_avg", "exp_avg_sq", "bf16 weight copies"]


def _assert_snap(now, ref, what):
    for name, a, b in zip(SNAP_NAMES, now, ref):
        assert _same(a, b), f"{what}: {name}: {int((_bits(a) != _bits(b)).sum())} elements differ"


def _assert_skipped(tr, total):
    norm = float(tr.grad_norm)
    assert not math.isfinite(norm), f"the bad batch gave a finite gradient norm ({norm}): nothing was tested"
    assert int(tr.step_skipped) == 1 and int(tr.skipped_steps) == total
    assert not math.isfinite(float(tr.grad_clip_coef)) or float(tr.grad_clip_coef) == 0.0


def _host_bias_corrections(t, betas=(0.9, 0.95)):
    """_set_hyper's expressions for Adam step t, as the f32 values it uploads"""
    return torch.tensor([1.0 - betas[0] ** t, (1.0 - betas[1] ** t) ** 0.5], dtype=torch.float32, device=DEV)


def _assert_step_is_unguarded_adamw(tr, before, t, what):
    """The step tr just took against the UNGUARDED AdamW entry point run on the gradient that step left in flat_g, from the state
    `before`, with the host's hyper block for Adam step t: same bits in parameters and moments.
    (Beside the comparisons of two trainers: this one names the step and the Adam step count when they fail.)"""
    from vtp_amd import ops
    st = tr.store
    hyper = tr.hyper.clone()
    assert _same(hyper[5:7], _host_bias_corrections(t)), (what, t, hyper[5:7].tolist(), _host_bias_corrections(t).tolist())
    assert float(hyper[7]) == 1.0 / tr.world  # max_grad_norm = inf: coefficient 1
    p0, m0, v0 = (x.clone() for x in before[:3])
    for lo, hi in tr.ranges_rec:
        ops.adamw_dev(p0[lo:hi], st.flat_g[lo:hi], m0[lo:hi], v0[lo:hi], None, hi - lo, hyper, tr.nodecay4[lo // 4:hi // 4])
    torch.cuda.synchronize()
    assert not _same(p0, before[0])
    _assert_snap([p0, m0, v0], [st.flat_p, tr.m, tr.v], what)


def _good_bad_good(golden_sd, use_graphs):
    good0, bad, good1 = _images()
    tr = _trainer(_build(golden_sd), use_graphs=use_graphs)
    tr.step(good0)
    torch.cuda.synchronize()
    assert int(tr.step_skipped) == 0 and int(tr.skipped_steps) == 0 and math.isfinite(float(tr.grad_norm))
    before = _snapshot(tr)
    tr.step(bad)
    torch.cuda.synchronize()
    _assert_skipped(tr, 1)
    _assert_snap(_snapshot(tr), before, "skipped step")
    tr.step(good1)
    torch.cuda.synchronize()
    assert int(tr.step_skipped) == 0 and int(tr.skipped_steps) == 1 and math.isfinite(float(tr.grad_norm))
    # the third step is Adam step 2 from the state the first step left: as if the bad step had never happened
    _assert_step_is_unguarded_adamw(tr, before, 2, "the step behind the skipped one")
    assert torch.isfinite(tr.store.flat_p).all() and torch.isfinite(tr.m).all() and torch.isfinite(tr.v).all()
    return tr


@pytest.mark.parametrize("use_graphs", [False, True])
def test_bad_step_is_skipped_and_the_run_continues_as_if_it_never_happened(golden_sd, use_graphs):
    """Without the guard the second step leaves NaN in flat_p (this is the test that fails without the feature).  After good, bad,
    good everything equals, bit for bit, a second trainer that ran good, good."""
    tr = _good_bad_good(golden_sd, use_graphs)
    good0, _, good1 = _images()
    ref = _trainer(_build(golden_sd), use_graphs=use_graphs)
    ref.step(good0)
    ref.step(good1)
    torch.cuda.synchronize()
    assert _same(tr.hyper, ref.hyper), "the third step must use the hyper block of Adam step 2"
    assert tr.step_no == 3 and ref.step_no == 2  # attempted steps
    assert tr._skip_state.tolist() == [2, 1, 0, 0] and ref._skip_state.tolist() == [2, 0, 0, 0]
    _assert_snap(_snapshot(tr), _snapshot(ref), "good, bad, good against good, good")


def test_logit_scale_clamp_is_idempotent_on_a_skipped_step(golden_sd):
    """the clamp behind the updates is not guarded: on a skipped step logit_scale still holds what the previous applied step left,
    which the clamp does not move"""
    good0, bad, _ = _images(one=False)
    _, txt = _data()
    txt = txt.cuda()
    tr = _trainer(_build(golden_sd))
    ls = tr.store.p("logit_scale")
    ls.fill_(math.log(100.0) + 0.5)  # above the bound: the first applied step clamps it
    tr.step(good0, txt)
    torch.cuda.synchronize()
    assert float(ls) == float(torch.tensor(math.log(100.0), dtype=torch.float32))
    before = _snapshot(tr)
    tr.step(bad, txt)
    torch.cuda.synchronize()
    _assert_skipped(tr, 1)
    _assert_snap(_snapshot(tr), before, "skipped step with the contrastive objective")


def test_guard_on_and_off_agree_on_finite_batches(golden_sd):
    """three steps, default betas: parameters, moments and bf16 copies of the guarded and the unguarded trainer are equal bit for
    bit.  The run is deterministic; a failure would be a one-ulp bias correction (the hyper blocks are printed and compared first)."""
    good0, _, good1 = _images()
    trs = [_trainer(_build(golden_sd), skip_nonfinite=flag) for flag in (True, False)]
    hypers = []
    for tr in trs:
        hs = []
        for t, img in enumerate((good0, good1, good0), start=1):
            before = _snapshot(tr)
            tr.step(img)
            torch.cuda.synchronize()
            hs.append(tr.hyper.clone())
            _assert_step_is_unguarded_adamw(tr, before, t, f"step {t}, guard {'on' if tr.skip_nonfinite else 'off'}")
        hypers.append(torch.stack(hs).cpu())
    print("hyper[5:7] per step, guard on :", hypers[0][:, 5:7].tolist())
    print("hyper[5:7] per step, guard off:", hypers[1][:, 5:7].tolist())
    assert _same(hypers[0], hypers[1]), "device and host bias corrections differ: fix the device formula, not a tolerance"
    assert trs[0]._skip_state.tolist() == [3, 0, 0, 0] and trs[1].step_skipped is None and trs[1].skipped_steps is None
    _assert_snap(_snapshot(trs[0]), _snapshot(trs[1]), "guard on against guard off")
    # the betas are baked into the guarded finalize: a change is refused before anything moves, not half applied
    trs[0].betas = (0.8, 0.95)
    with pytest.raises(ValueError, match="betas"):
        trs[0].step(good0)
    assert trs[0].step_no == 3


@pytest.mark.parametrize("lane", [True, False])
def test_ssl_step_is_skipped_with_the_teacher(sslg, lane):
    """rec + DINO/iBOT step without captions.  Optimizer lane: the fused AdamW + EMA launches and the EMA of the pairs this step's
    buckets do not cover; serial leg: AdamW, then the EMA loop over every pair.  Either way student, teacher, moments and bf16
    copies (the weight-norm hooks' outputs included) are left alone on the skipped step"""
    from vtp_amd.train import merge_ranges, uncovered
    from vtp_amd.vtp import _range
    g, sd = sslg
    m = build_vtp(sd)
    tr = _trainer(m, teacher_momentum=0.9)
    assert tr.overlap_opt
    tr.overlap_opt = lane
    st = tr.store
    img, _, ssl = _ssl_inputs(tr, g)
    tr.step(img, None, ssl)
    torch.cuda.synchronize()
    assert int(tr.step_skipped) == 0
    before = _snapshot(tr)
    bad = img.clone()
    bad[0, 1, 9, 30] = float("nan")
    tr.step(bad, None, ssl)
    torch.cuda.synchronize()
    _assert_skipped(tr, 1)
    now = _snapshot(tr)
    done = merge_ranges(list(tr.ranges_rec) + list(tr.ranges_ssl))
    left = 0
    for t_pref, s_pref in m.ema_pairs():
        (tlo, thi), (slo, shi) = _range(st, t_pref), _range(st, s_pref)
        assert _same(now[0][tlo:thi], before[0][tlo:thi]), f"teacher range {t_pref} moved"
        left += sum(b - a for a, b in uncovered(slo, shi, done))
    assert left > 0, "no EMA pair outside this step's buckets: the lane's guarded EMA launch never ran"
    _assert_snap(now, before, "skipped SSL step")
    tr.step(img, None, ssl)
    torch.cuda.synchronize()
    assert int(tr.step_skipped) == 0 and int(tr.skipped_steps) == 1
    assert not _same(st.flat_p, before[0]) and torch.isfinite(st.flat_p).all()


def test_checkpoint_carries_applied_and_skipped_counts(golden_sd):
    tr = _good_bad_good(golden_sd, False)
    sd = tr.state_dict()
    assert sd["step"] == 2 and sd["skipped_steps"] == 1
    weights = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    m2 = _build(golden_sd)
    m2.load_state_dict(weights)
    tr2 = _trainer(m2)
    tr2.load_state_dict(sd)
    assert tr2._skip_state.tolist() == [2, 1, 0, 0] and tr2.step_no == 3
    _assert_snap(_snapshot(tr2)[:3], _snapshot(tr)[:3], "restored trainer")
    # one more good step on both: the restored trainer's result is the original's, bit for bit
    good0 = _images()[0]
    for t in (tr, tr2):
        before = _snapshot(t)
        t.step(good0)
        torch.cuda.synchronize()
        _assert_step_is_unguarded_adamw(t, before, 3, "the step after the restore")
    _assert_snap(_snapshot(tr2), _snapshot(tr), "the step after the restore")
    assert _same(tr2.hyper, tr.hyper) and tr2.state_dict()["step"] == 3 and tr2.state_dict()["skipped_steps"] == 1
    # a checkpoint written without the guard: every step counts as applied
    plain = dict(sd)
    del plain["skipped_steps"]
    tr2.load_state_dict(plain)
    assert tr2._skip_state.tolist() == [2, 0, 0, 0]


# ---- 8. two ranks, sharded optimizer, only rank 1's batch is bad ---------------------------------------------------------------
def _skip_worker(rank, world, port, out):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from safetensors.torch import load_file
    from vtp_amd import VTPTrainer
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = load_file(os.path.join(root, "tests", "golden", "vtp_tiny.safetensors"))
    m = _build({k[3:]: v for k, v in g.items() if k.startswith("sd.")})
    tr = VTPTrainer(m, lr=1e-3, weight_decay=0.01, bucket_blocks=1, shard_optimizer=True, max_grad_norm=INF, skip_nonfinite=True)
    img, txt = _data()
    sl = slice(rank * 2, rank * 2 + 2)
    img, txt = img[sl].cuda(), txt[sl].cuda()
    tr.step(img, txt)
    torch.cuda.synchronize()
    before = m._engine().flat_p.detach().clone()
    if rank == 1:
        img = img.clone()
        img[0, 0, 3, 3] = float("nan")
    tr.step(img, txt)
    torch.cuda.synchronize()
    out[rank] = (int(tr.step_skipped), int(tr.skipped_steps), float(tr.grad_norm), before.cpu().view(torch.int32),
                 m._engine().flat_p.detach().cpu().view(torch.int32), tr.state_dict()["step"])
    dist.destroy_process_group()


def test_two_sharded_ranks_skip_together_when_one_batch_is_bad():
    out = mp.Manager().dict()
    mp.spawn(_skip_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    for rank in (0, 1):
        skipped, total, norm, before, after, applied = out[rank]
        assert not math.isfinite(norm), f"rank {rank}: finite norm {norm}: nothing was tested"
        assert (skipped, total, applied) == (1, 1, 1), (rank, skipped, total, applied)
        assert torch.equal(before, after), f"rank {rank}: parameters moved on the skipped step"
    assert torch.equal(out[0][4], out[1][4]), "ranks diverged"
