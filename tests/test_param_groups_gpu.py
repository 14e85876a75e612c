"""Per-parameter-group learning-rate / weight-decay scales of VTPTrainer (param_groups) on the GPU: the two grouped AdamW kernels
against the masked ones (degenerate table, bit for bit) and against torch.optim.AdamW(param_groups, foreach=False); the trainer against
torch with layerwise_lr_decay and a frozen group; the four optimizer paths (lane on / off, eager / hipGraphs, with and without gradient
clipping) against the grouped kernels replayed on the recorded gradient; a scale schedule under graph replay; two gloo ranks,
replicated and sharded; the checkpoint; and param_groups=None.

Tolerances are the project's own (tests/test_grad_clip_gpu.py compares the same kernels with torch's AdamW at relative L2 <= 1e-5).
Inputs of the kernel tests are weight-like (|p| ~ 0.02): the update of a step is ~lr = 1e-3 and is measured as p_new - p_old, so a
parameter of magnitude 1 would put its own fp32 rounding (6e-8 / 1e-3) above the bar whatever the kernel does.  The tests that compare
two separate runs bit for bit take rec-only steps on ONE 48 x 48 image (10 trunk rows, 9 decoder rows): the backward sums a gain /
bias gradient with one fp32 atomic per workgroup and column, the norm backward at 8 rows per workgroup, so no address has more than
two contributors and a + b = b + a -- the atomics cannot reorder the result between the runs (at 17 rows, three workgroups, the
norm-gain gradients of two identical runs differ in their last bit, with or without groups)."""
import math

import pytest
import torch
import torch.multiprocessing as mp

from test_ddp_gpu import _build, _data, _free_port
from test_ssl_gpu import DEV, build_vtp, sslg  # noqa: F401  (fixture + helpers)

pytestmark = pytest.mark.gpu
HYPER = [1e-3, 0.9, 0.95, 1e-8, 0.05]  # lr, beta1, beta2, eps, weight decay
SCALES5 = [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.3, 2.0), (2.5, 0.5)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cpu, cuda = torch.get_rng_state(), torch.cuda.get_rng_state()
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(cuda)


def _hyper(step, gs=1.0, mom=0.994):
    lr, b1, b2, eps, wd = HYPER
    h = torch.zeros(16, device=DEV)
    h[:10] = torch.tensor([lr, b1, b2, eps, wd, 1 - b1 ** step, (1 - b2 ** step) ** 0.5, gs, 0.0, mom])
    return h


def _state(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    p, gr = torch.randn(n, device=DEV, generator=g) * 0.02, torch.randn(n, device=DEV, generator=g) * 1e-2
    m, v = torch.randn(n, device=DEV, generator=g) * 1e-2, torch.rand(n, device=DEV, generator=g) * 1e-4
    t = torch.randn(n, device=DEV, generator=g) * 0.02
    return p, gr, m, v, t, g


def _rel(a, b):
    """relative L2 of a against b; two all-zero tensors agree"""
    nb = float(b.double().norm())
    if nb == 0.0:
        return 0.0 if float(a.double().norm()) == 0.0 else math.inf
    return float((a.double() - b.double()).norm()) / nb


# ---- the kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 260, 4096 * 3 + 148, (1 << 24) + 4])
def test_degenerate_table_is_the_masked_kernels_bit_for_bit(n):
    """rows {(1,1), (1,0)} with group4 = nodecay4: vtp_adamw_dev_masked and vtp_adamw_ema_dev, bit for bit"""
    from vtp_amd import ops
    p, gr, m, v, t, g = _state(n, n)
    nd = (torch.rand(n // 4, device=DEV, generator=g) < 0.3).to(torch.uint8)
    tab = torch.tensor([[1.0, 1.0], [1.0, 0.0]], device=DEV)
    hyper = _hyper(3, gs=0.5)
    guard = gr.clone()
    a = [x.clone() for x in (p, m, v)]
    ops.adamw_dev(a[0], gr, a[1], a[2], None, n, hyper, nd)
    b = [x.clone() for x in (p, m, v)]
    ops.adamw_dev_grouped(b[0], gr, b[1], b[2], None, n, hyper, nd, tab, 2)
    torch.cuda.synchronize()
    for x, y, name in zip(a, b, ("p", "m", "v")):
        assert torch.equal(x, y), f"adamw_dev_grouped {name}: {int((x != y).sum())} of {n} elements differ"
    for teacher in (True, False):
        a = [x.clone() for x in (p, m, v, t)]
        ops.adamw_ema_dev(a[0], gr, a[1], a[2], a[3] if teacher else None, n, hyper, nd)
        b = [x.clone() for x in (p, m, v, t)]
        ops.adamw_ema_dev_grouped(b[0], gr, b[1], b[2], b[3] if teacher else None, n, hyper, nd, tab, 2)
        torch.cuda.synchronize()
        for x, y, name in zip(a, b, ("p", "m", "v", "teacher")):
            assert torch.equal(x, y), f"adamw_ema_dev_grouped {name}: {int((x != y).sum())} of {n} elements differ"
        assert teacher == (not torch.equal(b[3], t))
    assert torch.equal(gr, guard)


def _segments(n4, k, gen):
    """k segments of [0, n4) with boundaries at random float4 indices: [(lo4, hi4)]"""
    cuts = sorted((torch.randperm(n4 - 1, generator=gen)[:k - 1] + 1).tolist())
    edges = [0] + cuts + [n4]
    return list(zip(edges, edges[1:]))


@pytest.mark.parametrize("fused", [False, True])
def test_grouped_kernels_match_torch_adamw_param_groups(fused):
    """5 groups with distinct scales (one with lr_scale 0, one with wd_scale 0), boundaries at random multiples of 4, 3 steps against
    fp32 torch.optim.AdamW(param_groups, foreach=False): moments and parameter update at relative L2 <= 1e-5 per group; the frozen
    group's parameters keep their bits while its moments (and the fused EMA teacher) move"""
    from vtp_amd import ops
    lr, b1, b2, eps, wd = HYPER
    n = 4096 * 5 + 148
    p, _, _, _, t, g = _state(n, 77)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    segs = _segments(n // 4, 5, torch.Generator().manual_seed(5))
    order = [3, 1, 4, 0, 2]  # the group of each segment: not in table order
    group4 = torch.zeros(n // 4, dtype=torch.uint8, device=DEV)
    for (lo, hi), gi in zip(segs, order):
        group4[lo:hi] = gi
    tab = torch.tensor(SCALES5, device=DEV)
    params = [torch.nn.Parameter(p[4 * lo:4 * hi].clone()) for lo, hi in segs]
    opt = torch.optim.AdamW([{"params": [q], "lr": lr * SCALES5[gi][0], "weight_decay": wd * SCALES5[gi][1]}
                             for q, gi in zip(params, order)], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    mom = 0.9
    for step in range(1, 4):
        gr = torch.randn(n, device=DEV, generator=g) * 1e-2
        p_old, t_old = p.clone(), t.clone()
        hyper = _hyper(step, mom=mom)
        if fused:
            ops.adamw_ema_dev_grouped(p, gr, m, v, t, n, hyper, group4, tab, 5)
        else:
            ops.adamw_dev_grouped(p, gr, m, v, None, n, hyper, group4, tab, 5)
        for q, (lo, hi) in zip(params, segs):
            q.grad = gr[4 * lo:4 * hi].clone()
        opt.step()
        torch.cuda.synchronize()
        for q, (lo, hi), gi in zip(params, segs, order):
            sl = slice(4 * lo, 4 * hi)
            em, ev = _rel(m[sl], opt.state[q]["exp_avg"]), _rel(v[sl], opt.state[q]["exp_avg_sq"])
            eu = _rel(p[sl] - p_old[sl], q.detach() - p_old[sl])
            print(f"step {step} group {gi} {SCALES5[gi]} [{4 * lo}, {4 * hi}): exp_avg {em:.2e} exp_avg_sq {ev:.2e} update {eu:.2e}")
            assert em <= 1e-5 and ev <= 1e-5 and eu <= 1e-5, (step, gi)
            assert float(m[sl].abs().max()) > 0 and float(v[sl].max()) > 0
            if SCALES5[gi][0] == 0.0:
                assert torch.equal(p[sl], p_old[sl]) and torch.equal(q.detach(), p_old[sl]), "lr_scale = 0 must leave p bit-unchanged"
            else:
                assert not torch.equal(p[sl], p_old[sl])
        if fused:  # the teacher follows the freshly updated student everywhere, the frozen group included
            assert _rel(t, mom * t_old + (1 - mom) * p) <= 1e-5
            assert not torch.equal(t, t_old)
        else:
            assert torch.equal(t, t_old)
        with torch.no_grad():  # both sides continue from the kernel's parameters
            for q, (lo, hi) in zip(params, segs):
                q.copy_(p[4 * lo:4 * hi])


def test_out_of_range_group_index_is_clamped_and_torch_op():
    """an index >= ngroups reads the LAST row, never past the table; torch.ops.vtp_hip.adamw_grouped is the same kernel"""
    import vtp_amd.torch_ops  # noqa: F401  (registers the library)
    from vtp_amd import ops
    n = 4096 + 36
    p, gr, m, v, _, _ = _state(n, 9)
    tab = torch.tensor([[1.0, 1.0], [0.5, 0.0], [2.0, 3.0]], device=DEV)
    hyper = _hyper(2)
    last = torch.full((n // 4,), 2, dtype=torch.uint8, device=DEV)
    a = [x.clone() for x in (p, m, v)]
    ops.adamw_dev_grouped(a[0], gr, a[1], a[2], None, n, hyper, last, tab, 3)
    for bad in (3, 200, 255):
        idx = torch.full((n // 4,), bad, dtype=torch.uint8, device=DEV)
        b = [x.clone() for x in (p, m, v)]
        ops.adamw_dev_grouped(b[0], gr, b[1], b[2], None, n, hyper, idx, tab, 3)
        c = [x.clone() for x in (p, m, v)]
        ops.adamw_ema_dev_grouped(c[0], gr, c[1], c[2], None, n, hyper, idx, tab, 3)
        torch.cuda.synchronize()
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z), bad
    d = [x.clone() for x in (p, m, v)]
    torch.ops.vtp_hip.adamw_grouped(d[0], gr, d[1], d[2], n, hyper, last, tab)
    torch.cuda.synchronize()
    for x, y in zip(a, d):
        assert torch.equal(x, y)


# ---- the trainer --------------------------------------------------------------------------------------------------------------
def _tiny_groups(model, frozen):
    """a frozen group, DINOv2's layer-wise decay over the trunk, the text tower on its own rate and decay"""
    from vtp_amd.train import layerwise_lr_decay
    names = list(model._engine().offsets)
    pg = [{"name": "frozen", "match": frozen, "lr_scale": 0.0}]
    pg += layerwise_lr_decay(names, model.config.vision_depth, decay=0.75, patch_embed_lr_mult=0.2)
    if any(n.startswith("text_transformer.") for n in names):
        pg.append({"name": "text", "match": ("text_transformer.", "token_embedding."), "lr_scale": 0.5, "wd_scale": 2.0})
    return pg


def _members(tr, names=None):
    """group name -> [parameter name] as the trainer resolved them (from its float4 index table)"""
    st = tr.store
    idx = tr._group4.cpu()
    out = {}
    for name, (o, k) in st.offsets.items():
        if names is None or name in names:
            out.setdefault(tr.param_groups[int(idx[o // 4]) // 2]["name"], []).append(name)
    return out


def test_trainer_matches_torch_adamw_with_layerwise_decay_and_a_frozen_group(golden_sd):
    """rec-only steps, no_decay=None, layerwise_lr_decay(0.75, patch_embed_lr_mult=0.2) plus one frozen group: torch's
    AdamW(param_groups, foreach=False) fed the trainer's gradient of every step gives the trainer's moments and parameter updates,
    group by group"""
    from vtp_amd import VTPTrainer
    m = _build(golden_sd)
    st = m._engine()
    lr, betas, eps, wd = 1e-3, (0.9, 0.95), 1e-8, 0.05
    tr = VTPTrainer(m, lr=lr, betas=betas, eps=eps, weight_decay=wd, no_decay=None,
                    param_groups=_tiny_groups(m, ("pixel_decoder.proj_out.",)))
    assert tr.group_tab is not None and tr.nodecay4 is None
    trained = [n for n, (o, k) in st.offsets.items() if any(lo <= o and o + k <= hi for lo, hi in tr.ranges_rec)]
    members = _members(tr, set(trained))
    L = m.config.vision_depth
    assert set(members) >= {"frozen", "default"} and len(members) >= L + 4, sorted(members)
    scales = {g["name"]: (g["lr_scale"], g["wd_scale"]) for g in tr.param_groups}
    assert scales["frozen"] == (0.0, 1.0) and sorted(s[0] for s in scales.values())[1] == 0.75 ** (L + 1) * 0.2
    sl = {n: slice(st.offsets[n][0], st.offsets[n][0] + st.offsets[n][1]) for n in trained}
    params = {n: torch.nn.Parameter(st.flat_p[sl[n]].detach().clone()) for n in trained}
    opt = torch.optim.AdamW([{"params": [params[n] for n in ns], "lr": lr * scales[gname][0], "weight_decay": wd * scales[gname][1]}
                             for gname, ns in members.items()], lr=lr, betas=betas, eps=eps, foreach=False)
    img, _ = _data()
    for i in range(3):
        p_old = st.flat_p.detach().clone()
        tr.step((img + 0.01 * i).cuda())
        torch.cuda.synchronize()
        for n in trained:
            params[n].grad = st.flat_g[sl[n]].detach().clone()
        opt.step()
        for gname, ns in members.items():
            cat = lambda f: torch.cat([f(n) for n in ns])  # noqa: E731
            em = _rel(cat(lambda n: tr.m[sl[n]]), cat(lambda n: opt.state[params[n]]["exp_avg"]))
            ev = _rel(cat(lambda n: tr.v[sl[n]]), cat(lambda n: opt.state[params[n]]["exp_avg_sq"]))
            eu = _rel(cat(lambda n: st.flat_p[sl[n]] - p_old[sl[n]]), cat(lambda n: params[n].detach() - p_old[sl[n]]))
            print(f"step {i} group {gname} {scales[gname]} ({len(ns)} parameters): exp_avg {em:.2e} exp_avg_sq {ev:.2e} update {eu:.2e}")
            assert em <= 1e-5 and ev <= 1e-5 and eu <= 1e-5, (i, gname)
            if gname == "frozen":
                assert all(torch.equal(st.flat_p[sl[n]], p_old[sl[n]]) for n in ns), "lr_scale = 0 must leave p bit-unchanged"
                assert float(cat(lambda n: tr.m[sl[n]]).abs().max()) > 0
        with torch.no_grad():  # both sides continue from the trainer's parameters (the next gradient is the trainer's)
            for n in trained:
                params[n].copy_(st.flat_p[sl[n]])


def _ssl_inputs(tr, g):
    from oracle.make_golden_ssl import SSL_CFG as C
    img = torch.randn(C["B"], 3, C["R"], C["R"], device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    txt = torch.randint(1, 60, (C["B"], 8), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    txt[:, 5] = 63
    ssl = tr.prepare_ssl(g["in.global_crops"].to(DEV), g["in.local_crops"].to(DEV), g["in.masks"].bool())
    return img, txt, ssl


@pytest.mark.parametrize("lane,use_graphs,max_norm", [(True, False, None), (False, False, None), (True, True, None), (False, True, None),
                                                      (True, True, 1e-3), (False, False, 1e-3)])
def test_every_optimizer_path_is_the_grouped_kernel_on_the_recorded_gradient(sslg, lane, use_graphs, max_norm):
    """rec + clip + DINO/iBOT step with groups and the default no_decay: the grouped kernels replayed on the recorded gradient with the
    step's hyper block and table reproduce student, teacher and moments bit for bit -- optimizer lane on and off, eager and hipGraphs,
    and behind gradient clipping"""
    from vtp_amd import VTPTrainer, ops
    from vtp_amd.train import merge_ranges
    from vtp_amd.vtp import _range
    g, sd = sslg
    m = build_vtp(sd)
    st = m._engine()
    tr = VTPTrainer(m, lr=5e-4, weight_decay=0.05, use_graphs=use_graphs, teacher_momentum=0.9, max_grad_norm=max_norm,
                    param_groups=_tiny_groups(m, ("dino_head.last_layer.",)))
    tr.overlap_opt = lane
    assert tr.nodecay4 is not None and int(tr._group4.max()) % 2 == 1, "the default no_decay must put parameters on exempt rows"
    img, txt, ssl = _ssl_inputs(tr, g)
    tr.step(img, txt, ssl)  # a first step: the moments are not zero in the replayed one
    torch.cuda.synchronize()
    p0, m0, v0 = st.flat_p.clone(), tr.m.clone(), tr.v.clone()
    start = p0.clone()
    tr.step(img, txt, ssl)
    torch.cuda.synchronize()
    flat_g, hyper, tab = st.flat_g.clone(), tr.hyper.clone(), tr.group_tab.clone()
    assert tab.shape == (2 * len(tr.param_groups), 2) and float(hyper[7]) == (1.0 if max_norm is None else float(tr.grad_clip_coef))
    if max_norm is not None:
        assert float(tr.grad_clip_coef) < 0.5
    ranges = merge_ranges(list(tr.ranges_all) + list(tr.ranges_ssl))
    for lo, hi in ranges:
        ops.adamw_dev_grouped(p0[lo:hi], flat_g[lo:hi], m0[lo:hi], v0[lo:hi], None, hi - lo, hyper, tr._group4[lo // 4:hi // 4], tab,
                              tab.shape[0])
    lo, hi = st.offsets["logit_scale"][0], st.offsets["logit_scale"][0] + 1
    p0[lo:hi].clamp_(max=math.log(100.0))
    for t_pref, s_pref in m.ema_pairs():
        (tlo, thi), (slo, shi) = _range(st, t_pref), _range(st, s_pref)
        ops.ema_dev(p0[tlo:thi], p0[slo:shi], thi - tlo, hyper[9:10])
    torch.cuda.synchronize()
    for a, b, name in ((p0, st.flat_p, "student + teacher"), (m0, tr.m, "exp_avg"), (v0, tr.v, "exp_avg_sq")):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ"
    # the groups did something: the frozen last layer kept its bits, and the masked kernel would have moved it
    members = _members(tr)
    for n in members["frozen"]:
        o, k = st.offsets[n]
        assert torch.equal(st.flat_p[o:o + k], start[o:o + k]) and float(tr.m[o:o + k].abs().max()) > 0, n
    o, k = st.offsets[members["text"][0]]
    assert not torch.equal(st.flat_p[o:o + k], start[o:o + k])
    assert len(members) >= 5


def _one_image():
    img, _ = _data()
    return img[:1, :, :48, :48].contiguous().cuda()


def test_scale_schedule_under_graph_replay_needs_no_recapture(golden_sd):
    """one group's lr_scale goes 0 -> 1 and another's wd_scale 1 -> 3 between replayed steps: one captured graph, and after 4 steps the
    parameters of an eager trainer on the same schedule, bit for bit"""
    from vtp_amd import VTPTrainer
    res = []
    for use_graphs in (True, False):
        m = _build(golden_sd)
        st = m._engine()
        pg = [{"name": "decoder", "match": ("pixel_decoder.",), "lr_scale": 0.0}, {"name": "trunk", "match": ("trunk.",), "lr_scale": 0.5}]
        tr = VTPTrainer(m, lr=1e-3, weight_decay=0.05, use_graphs=use_graphs, param_groups=pg)
        assert [g["name"] for g in tr.param_groups] == ["decoder", "trunk", "default"]
        lo, hi = tr.ranges_rec[0][0], tr.ranges_rec[-1][1]
        dec = [st.offsets[n] for n in st.offsets if n.startswith("pixel_decoder.")]
        img = _one_image()
        hist = []
        for i in range(4):
            if i == 2:
                tr.param_groups[0]["lr_scale"] = 1.0
            if i == 1:
                tr.param_groups[1]["wd_scale"] = 3.0
            before = st.flat_p.clone()
            tr.step(img + 0.01 * i)
            torch.cuda.synchronize()
            moved = any(not torch.equal(st.flat_p[o:o + k], before[o:o + k]) for o, k in dec)
            assert moved == (i >= 2), f"step {i}: the decoder group is {'not ' if i >= 2 else ''}frozen"
            assert tr.group_tab.cpu().tolist()[:4] == [[float(i >= 2), 1.0], [float(i >= 2), 0.0], [0.5, 3.0 if i >= 1 else 1.0], [0.5, 0.0]]
            hist.append(st.flat_p[lo:hi].clone())
        if use_graphs:
            assert len(tr._graphs) == 1, "a new scale must not re-capture"
        res.append(hist)
    for i, (a, b) in enumerate(zip(*res)):
        print(f"step {i}: graphs vs eager rel {_rel(a, b):.3e}, {int((a != b).sum())} of {a.numel()} elements differ")
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), f"step {i}: {int((a != b).sum())} elements differ between the replayed and the eager schedule"


def test_checkpoint_restores_the_scales_and_the_next_step(golden_sd):
    from vtp_amd import VTPTrainer
    groups = lambda m: _tiny_groups(m, ("pixel_decoder.proj_out.",))  # noqa: E731
    m = _build(golden_sd)
    tr = VTPTrainer(m, lr=1e-3, param_groups=groups(m))
    img = _one_image()
    for i in range(2):
        tr.step(img + 0.01 * i)
    tr.param_groups[0]["lr_scale"] = 0.25  # what a schedule left behind: the checkpoint carries it
    tr.param_groups[-1]["wd_scale"] = 1.5
    torch.cuda.synchronize()
    osd, msd = tr.state_dict(), {k: v.clone() for k, v in m.state_dict().items()}
    assert osd["param_groups"] == [{k: g[k] for k in ("name", "lr_scale", "wd_scale")} for g in tr.param_groups]
    assert osd["param_groups"][0] == {"name": "frozen", "lr_scale": 0.25, "wd_scale": 1.0}
    tr.step(img + 0.02)
    torch.cuda.synchronize()
    ref_p, ref_m, ref_v = m._engine().flat_p.clone(), tr.m.clone(), tr.v.clone()
    m2 = _build(golden_sd)
    m2.load_state_dict(msd)
    tr2 = VTPTrainer(m2, lr=1e-3, param_groups=groups(m2))
    assert tr2.param_groups[0]["lr_scale"] == 0.0
    tr2.load_state_dict(osd)
    assert [dict(g) for g in tr2.param_groups] == osd["param_groups"]
    tr2.step(img + 0.02)
    torch.cuda.synchronize()
    for a, b, name in ((m2._engine().flat_p, ref_p, "parameters"), (tr2.m, ref_m, "exp_avg"), (tr2.v, ref_v, "exp_avg_sq")):
        print(f"resumed vs uninterrupted {name}: rel {_rel(a, b):.3e}, {int((a != b).sum())} elements differ")
    for a, b, name in ((m2._engine().flat_p, ref_p, "parameters"), (tr2.m, ref_m, "exp_avg"), (tr2.v, ref_v, "exp_avg_sq")):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ"
    # other group names: refused, in either direction
    other = VTPTrainer(_build(golden_sd), lr=1e-3, param_groups=[{"name": "trunk", "match": ("trunk.",), "lr_scale": 0.5}])
    with pytest.raises(ValueError, match="param groups"):
        other.load_state_dict(osd)
    plain = VTPTrainer(_build(golden_sd), lr=1e-3)
    with pytest.raises(ValueError, match="param groups"):
        plain.load_state_dict(osd)
    psd = plain.state_dict()
    assert "param_groups" not in psd
    plain.load_state_dict(psd)  # a state dict without the key loads into a trainer without groups as before


def test_no_groups_allocates_nothing_and_steps_as_before(golden_sd):
    from vtp_amd import VTPTrainer
    res = []
    for kw in ({}, {"param_groups": None}):
        m = _build(golden_sd)
        tr = VTPTrainer(m, lr=1e-3, **kw)
        assert tr.group_tab is None and tr.param_groups is None and tr._group4 is None and tr._group_ring is None
        tr.step(_one_image())
        torch.cuda.synchronize()
        assert tr.group_tab is None and tr._group_ring is None
        res.append((m._engine().flat_p.clone(), tr.m.clone(), tr.v.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b), f"{int((a != b).sum())} elements differ"
    with pytest.raises(ValueError):
        VTPTrainer(_build(golden_sd), lr=1e-3, param_groups=[{"name": "none", "match": ("no_such_prefix.",)}])
    tr = VTPTrainer(_build(golden_sd), lr=1e-3, param_groups=[{"name": "trunk", "match": ("trunk.",)}])
    tr.param_groups[0]["lr_scale"] = float("nan")  # a broken schedule raises at the step, before anything moves
    with pytest.raises(ValueError, match="lr_scale"):
        tr.step(_one_image())
    assert tr.step_no == 0


# ---- two data-parallel ranks (gloo, one GPU) ----------------------------------------------------------------------------------
def _group_worker(rank, world, port, use_graphs, shard, grad_dtype, out):
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
                    param_groups=_tiny_groups(m, ("pixel_decoder.proj_out.",)))
    img, txt = _data()
    sl = slice(rank * 2, rank * 2 + 2)
    for i in range(3):
        tr.step((img[sl] + 0.01 * i).cuda(), txt[sl].cuda())
    torch.cuda.synchronize()
    osd = tr.state_dict()  # sharded mode: moments are gathered from their owners
    mom = torch.cat([osd["exp_avg"][n].reshape(-1) for n in sorted(osd["exp_avg"])])
    out[rank] = (m._engine().flat_p.detach().cpu().clone(), mom)
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def single_grouped(golden_sd):
    from vtp_amd import VTPTrainer
    m = _build(golden_sd)
    st = m._engine()
    start = st.flat_p.detach().cpu().clone()
    tr = VTPTrainer(m, lr=1e-3, weight_decay=0.01, param_groups=_tiny_groups(m, ("pixel_decoder.proj_out.",)))
    img, txt = _data()
    for i in range(3):
        tr.step((img + 0.01 * i).cuda(), txt.cuda())
    torch.cuda.synchronize()
    frozen = [st.offsets[n] for n in _members(tr)["frozen"]]
    out = (st.flat_p.detach().cpu().clone(), start, frozen)
    del tr, m
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("use_graphs", [False, True])
@pytest.mark.parametrize("shard,grad_dtype", [(False, "fp32"), (True, "fp32"), (True, "bf16")])
def test_two_ranks_with_groups_in_lockstep(single_grouped, use_graphs, shard, grad_dtype):
    """replicated and rank-sharded AdamW with groups: the replicas agree bit for bit, and with the single-process run on the whole batch
    to the bars of tests/test_grad_clip_gpu.py::test_two_ranks_clip_in_lockstep"""
    ref_p, start, frozen = single_grouped
    out = mp.Manager().dict()
    mp.spawn(_group_worker, args=(2, _free_port(), use_graphs, shard, grad_dtype, out), nprocs=2, join=True)
    (p0, m0), (p1, m1) = out[0], out[1]
    assert torch.equal(p0, p1), "ranks diverged"
    assert torch.equal(m0, m1), "gathered moments differ between ranks"
    for o, k in frozen:
        assert torch.equal(p0[o:o + k], start[o:o + k]), "the frozen group moved"
    rel = float((p0 - ref_p).norm() / ref_p.norm())
    print(f"groups world 2 (shard={shard}, {grad_dtype}, graphs={use_graphs}): weights rel {rel:.3e}")
    assert rel < (2e-4 if grad_dtype == "fp32" else 3e-3)
