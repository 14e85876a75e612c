"""Global gradient-norm clipping of VTPTrainer (max_grad_norm; torch.nn.utils.clip_grad_norm_, norm_type 2): the sum-of-squares
partials + finalize kernels against fp64 torch, the clipped step against the existing AdamW / EMA kernels replayed on the recorded
gradient (optimizer lane on and off, eager and hipGraphs), the semantics against torch's clip_grad_norm_ + AdamW, and two gloo ranks
(all-reduce, sharded fp32 / bf16; eager and graphs) that must agree bit for bit."""
import math

import pytest
import torch
import torch.multiprocessing as mp

from test_ddp_gpu import _build, _data, _free_port
from test_ssl_gpu import DEV, build_vtp, sslg  # noqa: F401  (fixture + helpers)

pytestmark = pytest.mark.gpu
CHUNK = 8192  # elements per partial (csrc/gradnorm.hip)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    # model construction draws from the global CPU generator: the tests that run after this module see the generator states they
    # would have seen without it
    cpu, cuda = torch.get_rng_state(), torch.cuda.get_rng_state()
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(cuda)


def _finalize_ref(norm, max_norm):
    """torch's clip_grad_norm_ tail in fp32 on the kernel's own norm"""
    c = torch.tensor(max_norm, dtype=torch.float32, device=norm.device) / (norm + 1e-6)
    return torch.clamp(c, max=1.0)


def _run(x, n, max_norm, gs=1.0):
    from vtp_amd import ops
    cnt = ops.sumsq_partials_count(n)
    parts = torch.full((cnt + 3,), float("nan"), dtype=torch.float64, device=DEV)
    ops.sumsq_partials(x, n, parts)
    hyper = torch.zeros(16, device=DEV)
    hyper[7], hyper[10] = gs, max_norm
    norm, coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ops.grad_clip_finalize(parts, cnt, hyper, norm, coef)
    torch.cuda.synchronize()
    return parts, cnt, hyper, norm, coef


@pytest.mark.parametrize("n", [4, 260, 4096 * 3 + 148, (1 << 24) + 4])
def test_partials_and_finalize_match_fp64_torch(n):
    from vtp_amd import ops
    assert ops.sumsq_partials_count(n) == (n + CHUNK - 1) // CHUNK
    x = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)) * 3e-3
    parts, cnt, hyper, norm, coef = _run(x, n, 1e-2)
    # one partial per chunk, nothing written behind the last one
    pad = torch.zeros(cnt * CHUNK, dtype=torch.float64, device=DEV)
    pad[:n] = x.double().square()
    ref_parts = pad.view(cnt, CHUNK).sum(1)
    assert torch.allclose(parts[:cnt], ref_parts, rtol=1e-12, atol=0)
    assert torch.isnan(parts[cnt:]).all()
    ref = float(torch.linalg.vector_norm(x.double()))
    assert abs(float(norm) - ref) <= 1e-6 * ref
    assert torch.equal(coef, _finalize_ref(norm, 1e-2))
    assert torch.equal(hyper[7:8], coef)
    # bitwise reproducible
    parts2, _, hyper2, norm2, coef2 = _run(x, n, 1e-2)
    assert torch.equal(parts2[:cnt], parts[:cnt]) and torch.equal(norm2, norm) and torch.equal(coef2, coef) and torch.equal(hyper2, hyper)


def test_several_ranges_in_one_partials_buffer_and_gradient_multiplier():
    from vtp_amd import ops
    lens = [260, 4096 * 3 + 148, 4, 2 * CHUNK]
    x = torch.randn(sum(lens) + 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    parts = torch.zeros(sum(ops.sumsq_partials_count(n) for n in lens), dtype=torch.float64, device=DEV)
    base, off, pieces = 0, 0, []
    for n in lens:
        ops.sumsq_partials(x[off:off + n], n, parts[base:])
        pieces.append(x[off:off + n])
        base += ops.sumsq_partials_count(n)
        off += n + 16  # gaps between the ranges stay out of the norm
    assert base == parts.numel()
    total = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.sum_partials(parts, base, total)
    for gs, max_norm in ((0.5, 1.0), (0.5, 1e4)):
        hyper = torch.zeros(16, device=DEV)
        hyper[7], hyper[10] = gs, max_norm
        norm, coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        ops.grad_clip_finalize(parts, base, hyper, norm, coef)
        torch.cuda.synchronize()
        full = torch.cat(pieces).double()
        ref = gs * float(torch.linalg.vector_norm(full))
        assert abs(float(norm) - ref) <= 1e-6 * ref
        assert abs(float(total) - float(full.square().sum())) <= 1e-12 * float(total)
        exp_coef = min(1.0, max_norm / (ref + 1e-6))
        assert abs(float(coef) - exp_coef) <= 1e-6 * exp_coef
        assert torch.equal(coef, _finalize_ref(norm, max_norm))
        assert float(hyper[7]) == float(torch.tensor(gs, dtype=torch.float32) * coef.cpu())
        assert (exp_coef < 1) == (max_norm == 1.0)


def test_non_finite_gradients_propagate_like_torch():
    for bad in (float("inf"), float("nan")):
        x = torch.randn(1000, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
        x[123] = bad
        _, _, hyper, norm, coef = _run(x, 1000, 1.0, gs=0.5)
        p = torch.zeros(1000, device=DEV, requires_grad=True)
        p.grad = x.clone()
        ref_norm = torch.nn.utils.clip_grad_norm_([p], 1.0)
        if bad == float("inf"):
            assert math.isinf(float(norm)) and math.isinf(float(ref_norm))
            assert float(coef) == 0.0 and float(hyper[7]) == 0.0
        else:
            assert math.isnan(float(norm)) and math.isnan(float(ref_norm))
            assert math.isnan(float(coef)) and math.isnan(float(hyper[7])) and torch.isnan(p.grad).all()


# ---- the clipped step ---------------------------------------------------------------------------------------------------------
def _ssl_inputs(tr, g):
    from oracle.make_golden_ssl import SSL_CFG as C
    img = torch.randn(C["B"], 3, C["R"], C["R"], device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    txt = torch.randint(1, 60, (C["B"], 8), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    txt[:, 5] = 63
    ssl = tr.prepare_ssl(g["in.global_crops"].to(DEV), g["in.local_crops"].to(DEV), g["in.masks"].bool())
    return img, txt, ssl


def _ranges_norm(flat_g, ranges, scale=1.0):
    return scale * math.sqrt(sum(float(flat_g[lo:hi].double().square().sum()) for lo, hi in ranges))


@pytest.mark.parametrize("lane,use_graphs", [(True, False), (False, False), (True, True), (False, True)])
def test_clipped_step_is_adamw_on_the_recorded_gradient(sslg, lane, use_graphs):
    """rec + clip + DINO/iBOT step with a small max_grad_norm: the trainer's norm / multiplier follow the recorded gradient, and the
    existing AdamW + EMA kernels replayed on it with the step's hyper block reproduce student, teacher and moments bit for bit"""
    from vtp_amd import VTPTrainer, ops
    from vtp_amd.train import merge_ranges
    from vtp_amd.vtp import _range
    g, sd = sslg
    m = build_vtp(sd)
    st = m._engine()
    max_norm = 1e-3
    tr = VTPTrainer(m, lr=5e-4, weight_decay=0.05, use_graphs=use_graphs, teacher_momentum=0.9, max_grad_norm=max_norm)
    tr.overlap_opt = lane
    img, txt, ssl = _ssl_inputs(tr, g)
    tr.step(img, txt, ssl)  # a first step: the moments are not zero in the replayed one
    torch.cuda.synchronize()
    p0, m0, v0 = st.flat_p.clone(), tr.m.clone(), tr.v.clone()
    tr.step(img, txt, ssl)
    torch.cuda.synchronize()
    flat_g, hyper = st.flat_g.clone(), tr.hyper.clone()
    ranges = merge_ranges(list(tr.ranges_all) + list(tr.ranges_ssl))
    ref = _ranges_norm(flat_g, ranges, 1.0 / tr.world)
    norm = float(tr.grad_norm)
    assert abs(norm - ref) <= 1e-6 * ref, (norm, ref)
    coef = min(1.0, max_norm / (ref + 1e-6))
    assert coef < 0.5
    assert abs(float(hyper[7]) - coef) <= 1e-6 * coef
    assert float(tr.grad_clip_coef) == float(hyper[7])  # one rank: multiplier = 1/world * coef = coef
    for lo, hi in ranges:
        ops.adamw_dev(p0[lo:hi], flat_g[lo:hi], m0[lo:hi], v0[lo:hi], None, hi - lo, hyper, tr.nodecay4[lo // 4:hi // 4])
    lo, hi = st.offsets["logit_scale"][0], st.offsets["logit_scale"][0] + 1
    p0[lo:hi].clamp_(max=math.log(100.0))
    for t_pref, s_pref in m.ema_pairs():
        (tlo, thi), (slo, shi) = _range(st, t_pref), _range(st, s_pref)
        ops.ema_dev(p0[tlo:thi], p0[slo:shi], thi - tlo, hyper[9:10])
    torch.cuda.synchronize()
    for a, b, name in ((p0, st.flat_p, "student + teacher"), (m0, tr.m, "exp_avg"), (v0, tr.v, "exp_avg_sq")):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ"


def test_semantics_match_torch_clip_grad_norm_and_adamw(golden_sd):
    """rec-only steps without decay exemptions: torch's clip_grad_norm_ + AdamW (foreach=False) on the trainer's gradient of every
    step give the trainer's norm, moments and parameter updates"""
    from vtp_amd import VTPTrainer
    m = _build(golden_sd)
    st = m._engine()
    max_norm, lr, betas, eps, wd = 1e-3, 1e-3, (0.9, 0.95), 1e-8, 0.05
    tr = VTPTrainer(m, lr=lr, betas=betas, eps=eps, weight_decay=wd, no_decay=None, max_grad_norm=max_norm)
    img, _ = _data()
    ranges = tr.ranges_rec
    params = [torch.nn.Parameter(st.flat_p[lo:hi].detach().clone()) for lo, hi in ranges]
    p_start = [p.detach().clone() for p in params]
    opt = torch.optim.AdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    clipped = False
    for i in range(3):
        tr.step((img + 0.01 * i).cuda())
        torch.cuda.synchronize()
        for p, (lo, hi) in zip(params, ranges):
            p.grad = st.flat_g[lo:hi].detach().clone()
        total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        clipped |= total > max_norm
        opt.step()
        assert abs(float(tr.grad_norm) - total) <= 1e-5 * total, (i, float(tr.grad_norm), total)
        ours_m = torch.cat([tr.m[lo:hi] for lo, hi in ranges])
        ref_m = torch.cat([opt.state[p]["exp_avg"] for p in params])
        ours_v = torch.cat([tr.v[lo:hi] for lo, hi in ranges])
        ref_v = torch.cat([opt.state[p]["exp_avg_sq"] for p in params])
        assert float((ours_m - ref_m).norm() / ref_m.norm()) <= 1e-5, i
        assert float((ours_v - ref_v).norm() / ref_v.norm()) <= 1e-5, i
        d_ours = torch.cat([st.flat_p[lo:hi] - p0 for (lo, hi), p0 in zip(ranges, p_start)])
        d_ref = torch.cat([p.detach() - p0 for p, p0 in zip(params, p_start)])
        assert float((d_ours - d_ref).norm() / d_ref.norm()) <= 1e-5, i
        # both sides continue from the trainer's parameters (the next gradient is the trainer's)
        with torch.no_grad():
            for p, (lo, hi), p0 in zip(params, ranges, p_start):
                p.copy_(st.flat_p[lo:hi])
                p0.copy_(p)
    assert clipped


def test_infinite_max_norm_leaves_the_multiplier_exact(golden_sd):
    from vtp_amd import VTPTrainer
    tr = VTPTrainer(_build(golden_sd), lr=1e-3, max_grad_norm=float("inf"))
    img, _ = _data()
    tr.step(img.cuda())
    torch.cuda.synchronize()
    assert float(tr.grad_clip_coef) == 1.0 and float(tr.hyper[7]) == 1.0 / tr.world
    assert 0 < float(tr.grad_norm) < float("inf")


def test_graph_replay_tracks_every_step_and_a_new_max_norm(golden_sd):
    """under hipGraph replay grad_norm is a static buffer that each replay rewrites from that step's gradient; max_grad_norm changes
    between replays without a re-capture"""
    from vtp_amd import VTPTrainer
    m = _build(golden_sd)
    st = m._engine()
    tr = VTPTrainer(m, lr=1e-3, use_graphs=True, max_grad_norm=1e-2)
    img, txt = _data()
    norms = []
    for i in range(3):
        tr.step((img + 0.05 * i).cuda(), txt.cuda())
        torch.cuda.synchronize()
        ref = _ranges_norm(st.flat_g, tr.ranges_all)
        norms.append(float(tr.grad_norm))
        assert abs(norms[-1] - ref) <= 1e-6 * ref, (i, norms[-1], ref)
        assert abs(float(tr.hyper[7]) - min(1.0, 1e-2 / (ref + 1e-6))) <= 1e-6
    assert len(set(norms)) == 3
    assert len(tr._graphs) == 1
    for new in (1e3, 2e-3):
        tr.max_grad_norm = new
        tr.step(img.cuda(), txt.cuda())
        torch.cuda.synchronize()
        ref = _ranges_norm(st.flat_g, tr.ranges_all)
        exp = min(1.0, new / (ref + 1e-6))
        assert abs(float(tr.grad_clip_coef) - exp) <= 1e-6 * exp and abs(float(tr.hyper[7]) - exp) <= 1e-6 * exp
    assert len(tr._graphs) == 1, "a new max_grad_norm must not re-capture"


def test_none_allocates_nothing_and_bad_values_raise(golden_sd):
    from vtp_amd import VTPTrainer
    m = _build(golden_sd)
    tr = VTPTrainer(m, lr=1e-3)
    assert tr.max_grad_norm is None and tr.grad_norm is None and tr.grad_clip_coef is None and tr._clip_partials is None
    img, _ = _data()
    tr.step(img.cuda())
    assert tr.grad_norm is None and float(tr.hyper[10]) == 0.0
    with pytest.raises(ValueError):
        tr.max_grad_norm = 1.0
    for bad in (0, 0.0, -1.0, float("nan"), float("-inf"), "big", True):
        with pytest.raises(ValueError):
            VTPTrainer(m, lr=1e-3, max_grad_norm=bad)
    tr = VTPTrainer(m, lr=1e-3, max_grad_norm=2)
    assert tr.max_grad_norm == 2.0
    with pytest.raises(ValueError):
        tr.max_grad_norm = None
    with pytest.raises(ValueError):
        tr.max_grad_norm = -3.0
    assert tr.max_grad_norm == 2.0


# ---- two data-parallel ranks (gloo, one GPU) ----------------------------------------------------------------------------------
MAX_NORM = 1e-3


def _clip_worker(rank, world, port, use_graphs, shard, grad_dtype, out):
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
    tr = VTPTrainer(m, lr=1e-3, weight_decay=0.01, use_graphs=use_graphs, bucket_blocks=1, shard_optimizer=shard, grad_dtype=grad_dtype,
                    max_grad_norm=MAX_NORM)
    img, txt = _data()
    sl = slice(rank * 2, rank * 2 + 2)
    norms, coefs = [], []
    for i in range(3):
        tr.step((img[sl] + 0.01 * i).cuda(), txt[sl].cuda())
        norms.append(tr.grad_norm.clone())
        coefs.append(tr.grad_clip_coef.clone())
    torch.cuda.synchronize()
    out[rank] = (torch.cat(norms).cpu(), torch.cat(coefs).cpu(), m._engine().flat_p.detach().cpu().clone())
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def single_clipped(golden_sd):
    from vtp_amd import VTPTrainer
    m = _build(golden_sd)
    tr = VTPTrainer(m, lr=1e-3, weight_decay=0.01, max_grad_norm=MAX_NORM)
    img, txt = _data()
    norms = []
    for i in range(3):
        tr.step((img + 0.01 * i).cuda(), txt.cuda())
        norms.append(float(tr.grad_norm))
    torch.cuda.synchronize()
    out = (norms, m._engine().flat_p.detach().cpu().clone())
    del tr, m
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("use_graphs", [False, True])
@pytest.mark.parametrize("shard,grad_dtype", [(False, "fp32"), (True, "fp32"), (True, "bf16")])
def test_two_ranks_clip_in_lockstep(single_clipped, use_graphs, shard, grad_dtype):
    ref_norms, ref_p = single_clipped
    out = mp.Manager().dict()
    mp.spawn(_clip_worker, args=(2, _free_port(), use_graphs, shard, grad_dtype, out), nprocs=2, join=True)
    (n0, c0, p0), (n1, c1, p1) = out[0], out[1]
    assert torch.equal(n0, n1) and torch.equal(c0, c1), "ranks computed different norms"
    assert torch.equal(p0, p1), "ranks diverged"
    assert (c0 < 1).all(), f"clipping was not active: {c0.tolist()}"
    rel = float((p0 - ref_p).norm() / ref_p.norm())
    print(f"clip world 2 (shard={shard}, {grad_dtype}, graphs={use_graphs}): norms {n0.tolist()} vs single {ref_norms}, "
          f"weights rel {rel:.3e}")
    for a, b in zip(n0.tolist(), ref_norms):
        assert abs(a - b) < 5e-3 * b
    assert rel < (2e-4 if grad_dtype == "fp32" else 3e-3)
