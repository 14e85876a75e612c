"""vision_clip_feat='pooled' and vision_bottleneck_ae_only=False on the fused path (modeling_vtp.py:261-276, vtp.py:215-293,418-463):
the patch-row pooling kernel and the final-norm backward that takes the pooled gradient vs torch fp32; the VTPTrainer rec + clip step
of every new mode vs the fp32 oracle (E_ours <= 1.25 E_ref, the protocol of test_parity_ssl_gpu.py), vs the autograd path and
hipGraph vs eager; the legacy VTP with bottlenecked heads: SSL outputs and the rec + clip + ssl step vs the oracle composition."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
MODES = [("pooled", True), ("cls", False), ("pooled", False)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def relF(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------------------------------- kernels
def test_pool_patch_rows_ragged_items():
    from vtp_amd import ops
    D = 768
    items = [(2, 257), (3, 37), (1, 1025), (2, 13 * 7 + 1)]  # the last one a non-square 13 x 7 grid
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(sum(B * N for B, N in items), D, device=DEV, generator=g).to(BF)
    r0 = 0
    for B, N in items:
        xi = x[r0:r0 + B * N]
        out = torch.full((B, D), float("nan"), device=DEV)
        ops.pool_patch_rows(xi, out, B, N, D)
        ref = xi.float().view(B, N, D)[:, 1:].mean(1)
        err = float((out - ref).abs().max())
        print(f"pool B={B} N={N}: max err {err:.2e}")
        assert err <= 1e-5 * float(ref.abs().max()) + 1e-6
        r0 += B * N


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("D,seg", [(512, 1), (768, 1), (1024, 1), (768, 3)])
def test_norm_bwd_pvec_vs_torch(kind, D, seg):
    """D = 512 / 768 / 1024: the two-, three- and four-chunk rows; ragged items N = 37, 257, a 13 x 7 grid and 1025, the vector on item
    `seg`"""
    from vtp_amd import ops
    items = [(2, 37), (3, 257), (1, 13 * 7 + 1), (1, 1025)]
    M = sum(B * N for B, N in items)
    B, N = items[seg]
    row0 = sum(b * n for b, n in items[:seg])
    g = torch.Generator(device=DEV).manual_seed(2 + kind)
    x = torch.randn(M, D, device=DEV, generator=g)
    w = 1 + 0.1 * torch.randn(D, device=DEV, generator=g)
    b = 0.1 * torch.randn(D, device=DEV, generator=g) if kind == 1 else None
    eps = 1e-5 if kind == 0 else 1e-6
    y, stats = torch.empty(M, D, dtype=BF, device=DEV), torch.empty(M, 2, device=DEV)
    ops.norm_fwd(x, w, b, y, stats, M, D, eps, kind)
    dy = torch.randn(M, D, device=DEV, generator=g).to(BF)
    pvec = 0.05 * torch.randn(B, D, device=DEV, generator=g)
    dx, dxb = torch.empty(M, D, device=DEV), torch.empty(M, D, dtype=BF, device=DEV)
    dw, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV) if kind == 1 else None
    ops.norm_bwd_pvec(dy, x, w, stats, None, dx, dxb, dw, db, M, D, kind, pvec, row0, B, N)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    if kind == 0:
        yr = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + eps) * wr
        leaves = [xr, wr]
    else:
        br = b.clone().requires_grad_()
        yr = F.layer_norm(xr, (D,), wr, br, eps)
        leaves = [xr, wr, br]
    gt = dy.float().clone()
    gt[row0:row0 + B * N].view(B, N, D)[:, 1:] += pvec[:, None]
    ref = torch.autograd.grad(yr, leaves, gt)
    print(f"kind {kind} D {D} item {seg}: dx {relF(dx, ref[0]):.2e} dw {relF(dw, ref[1]):.2e}")
    assert relF(dx, ref[0]) < 1e-5 and relF(dw, ref[1]) < 1e-5
    assert torch.equal(dxb, dx.to(BF))
    if kind == 1:
        assert relF(db, ref[2]) < 1e-5
    # a zero vector reproduces vtp_norm_bwd exactly
    dx0, dxz = torch.empty_like(dx), torch.empty_like(dx)
    ops.norm_bwd(dy, x, w, stats, None, dx0, None, None, None, M, D, kind)
    ops.norm_bwd_pvec(dy, x, w, stats, None, dxz, None, None, None, M, D, kind, torch.zeros_like(pvec), row0, B, N)
    assert torch.equal(dx0, dxz)

# ------------------------------------------------------------------------------------------------------------------------- oracle
SMALL = 4096
REC_W = 100.0  # (the tiny model's L1 gradient is ~1e-3 of its contrastive one: weighted up so that every dW_bott share is visible)


def _oracle_ssl_outputs(sd, gc, lc, masks, heads, bott=True):
    """VTP.get_teacher_forward_outputs + get_student_ssl_outputs (vtp.py:410-484), use_bottleneck = not ae_only (pinned to the real
    reference by tests/test_bottleneck_heads_oracle.py)"""
    from oracle import vtp_oracle as O
    idx = masks.flatten().nonzero().flatten()
    with torch.no_grad():
        t = O.trunk_forward(sd, gc, heads, use_bottleneck=bott, pre="teacher_trunk.")
        cls = t["x_norm_clstoken"].chunk(2)
        cls = torch.cat((cls[1], cls[0]))
        th = O.dino_head_forward(sd, "teacher_dino_head.", torch.cat([cls, t["x_norm_patchtokens"].flatten(0, 1)[idx]]))
    n = cls.shape[0]
    sg = O.trunk_forward(sd, gc, heads, use_bottleneck=bott, masks=masks)
    sl = O.trunk_forward(sd, lc, heads, use_bottleneck=bott)
    teacher = {"teacher_cls_tokens_after_head": th[:n], "masked_teacher_patch_tokens_after_head": th[n:]}
    student = {"student_local_cls_tokens_after_head": O.dino_head_forward(sd, "dino_head.", sl["x_norm_clstoken"]),
               "student_global_cls_tokens_after_head": O.dino_head_forward(sd, "dino_head.", sg["x_norm_clstoken"]),
               "student_global_cls_tokens": sg["x_norm_clstoken"],
               "student_global_masked_patch_tokens_after_head":
                   O.dino_head_forward(sd, "dino_head.", sg["x_norm_patchtokens"].flatten(0, 1)[idx])}
    return teacher, student


def _oracle(sd, img, txt, feat, ae_only, mode, rec_w=REC_W, ssl=None):
    """rec_w * L1 + InfoNCE (+ DINO / iBOT / KoLeo) through the oracle: mode 'f32' (CPU), 'cpu16' (CPU autocast), 'gpu16' (CUDA
    autocast).  Returns (losses, {name: f32 CPU gradient})."""
    import contextlib
    from oracle import vtp_oracle as O
    dev = DEV if mode == "gpu16" else "cpu"
    ctx = contextlib.nullcontext() if mode == "f32" else torch.autocast("cuda" if mode == "gpu16" else "cpu", dtype=torch.bfloat16)
    sdr = {k: v.clone().to(dev).requires_grad_(v.dtype == torch.float32 and not k.startswith("teacher_")) for k, v in sd.items()}
    mv = lambda t: t.to(dev)  # noqa: E731
    with ctx:
        l1 = O.rec_train_loss(sdr, mv(img), 2, 2)
        i = O.clip_image_feature(sdr, mv(img), 2, True, feat, ae_only)
        t = O.clip_text_feature(sdr, mv(txt), 2)
        lc = O.clip_loss(i, t, sdr["logit_scale"].exp())
        if ssl is not None:
            gc, lcr, masks, n_local, koleo, K = ssl
            t_o, s_o = _oracle_ssl_outputs(sdr, mv(gc), mv(lcr), mv(masks), 2, bott=not ae_only)
    total = rec_w * l1.float() + lc.float()
    losses = [float(l1.detach()), float(lc.detach())]
    if ssl is not None:  # (the loss builds its index tensors on the CPU: evaluated there on differentiable fp32 copies)
        ls = O.ssl_loss({k: v.float().cpu() for k, v in t_o.items()}, {k: v.float().cpu() for k, v in s_o.items()}, masks,
                        torch.zeros(K), torch.zeros(K), n_local=n_local, koleo_weight=koleo)
        total = total + ls.to(total.device)
        losses.append(float(ls.detach()))
    total.backward()
    return losses, {k: v.grad.detach().float().cpu() for k, v in sdr.items() if v.grad is not None}


def _judge(params, g32, grefs, keys):
    """E_ours <= 1.25 E_ref, E_ref = the larger of the CPU- and CUDA-autocast errors of the oracle; tensors below SMALL elements are
    pooled (the rule of tests/test_parity_ssl_gpu.py); no absolute floors"""
    pool, pref, den = 0.0, [0.0] * len(grefs), 0.0
    for k in keys:
        ours, ref = params[k].grad.detach().float().cpu(), g32[k]
        es = [relF(g[k], ref) for g in grefs]
        e = relF(ours, ref)
        print(f"  grad {k} ({ref.numel()}): E_ours={e:.3e} E_ref={max(es):.3e} (cpu16 {es[0]:.3e}, gpu16 {es[-1]:.3e}) ratio {e / max(es):.2f}")
        if ref.numel() >= SMALL:
            assert e <= 1.25 * max(es), k
        else:
            pool += float((ours - ref).norm() ** 2)
            den += float(ref.norm() ** 2)
            for j, g in enumerate(grefs):
                pref[j] += float((g[k] - ref).norm() ** 2)
    if den:
        e, e_ref = (pool / den) ** 0.5, (max(pref) / den) ** 0.5
        print(f"  pooled small tensors: E_ours={e:.3e} E_ref={e_ref:.3e}")
        assert e <= 1.25 * e_ref


# ------------------------------------------------------------------------------------------------------------------------- rec + clip
def _data():
    g = torch.Generator().manual_seed(5)
    img = torch.randn(4, 3, 64, 64, generator=g)
    txt = torch.randint(1, 500, (4, 16), generator=g)
    txt[:, 0] = 510
    txt[torch.arange(4), torch.tensor([5, 9, 12, 15])] = 511
    return img, txt


def _cfg(feat, ae_only):
    from oracle.ref_stubs import TINY
    from vtp_amd import VTPConfig
    return VTPConfig(**TINY, vision_clip_feat=feat, vision_bottleneck_ae_only=ae_only)


def _sd(feat, ae_only):
    from vtp_amd import VTPModel
    torch.manual_seed(11)
    return {k: v.clone() for k, v in VTPModel(_cfg(feat, ae_only)).state_dict().items()}


def _model(feat, ae_only, sd):
    from vtp_amd import VTPModel
    m = VTPModel(_cfg(feat, ae_only))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


KEYS = ["trunk.feature_bottleneck.weight", "visual_proj.weight", "trunk.blocks.0.attn.qkv.weight", "trunk.blocks.1.mlp.w3.weight",
        "trunk.patch_embed.proj.weight", "pixel_decoder.proj_in.weight", "trunk.norm.weight", "trunk.cls_token"]


@pytest.mark.parametrize("feat,ae_only", MODES)
def test_rec_clip_step_vs_oracle_and_autograd_path(feat, ae_only):
    from vtp_amd import VTPTrainer
    img, txt = _data()
    sd = _sd(feat, ae_only)
    m = _model(feat, ae_only, sd)
    tr = VTPTrainer(m, lr=0.0, weight_decay=0.0, rec_weight=REC_W)
    l_rec, l_clip = (float(v) for v in tr.step(img.to(DEV), txt.to(DEV)))
    torch.cuda.synchronize()
    g_tr = m._store.flat_g.clone()
    params = dict(m.named_parameters())
    (r1, rc), g32 = _oracle(sd, img, txt, feat, ae_only, "f32")
    grefs = [_oracle(sd, img, txt, feat, ae_only, mode)[1] for mode in ("cpu16", "gpu16")]
    _, g_norec = _oracle(sd, img, txt, feat, ae_only, "f32", rec_w=0.0)
    vis = relF(g_norec["trunk.feature_bottleneck.weight"], g32["trunk.feature_bottleneck.weight"])
    print(f"{feat}/{ae_only}: rec {l_rec:.5f} (fp32 {r1:.5f}) clip {l_clip:.5f} (fp32 {rc:.5f}); rec share of dW_bott {vis:.2f}")
    assert vis > 0.1  # the reconstruction's dW_bott share is visible in this comparison
    assert abs(l_rec - r1) < 5e-3 * r1 and abs(l_clip - rc) < 1e-2 * rc
    _judge(params, g32, grefs, KEYS)
    # the autograd path (model(...) + torch loss + backward) on an identical model: same gradients within bf16 noise
    m2 = _model(feat, ae_only, sd)
    m2.train()
    m2.zero_grad()
    i2, t2 = img.to(DEV), txt.to(DEV)
    rec = m2(image=i2, forward_type="rec")
    clip = m2(image=i2, text=t2, forward_type="clip")
    logits = clip["logit_scale"] * clip["image_features"] @ clip["text_features"].T
    lab = torch.arange(4, device=DEV)
    loss = REC_W * (rec["reconstructed_image"] - i2).abs().mean() + 0.5 * (F.cross_entropy(logits, lab) + F.cross_entropy(logits.T, lab))
    loss.backward()
    torch.cuda.synchronize()
    rel = relF(m2._store.flat_g, g_tr)
    print(f"  flat gradient: autograd path vs VTPTrainer rel diff {rel:.3e}")
    assert rel < 1.5e-2


def _steps(m, tr, img, txt, n, **kw):
    out = [tuple(float(v) for v in tr.step(img + 0.01 * i, txt, **kw)) for i in range(n)]
    torch.cuda.synchronize()
    return out, m._store.flat_p.clone()


@pytest.mark.parametrize("layout", ["shared", "separate_rec_segments"])
@pytest.mark.parametrize("feat,ae_only", MODES)
def test_rec_clip_graph_step_equals_eager(feat, ae_only, layout, monkeypatch):
    """one captured graph per step (shared rec / clip item), or a separate reconstruction_image (its own list item: the pooled vector
    goes to item 0) captured as one segment per bucket event (VTP_SINGLE_GRAPH=0); gradient clipping on.  Losses AND weights."""
    from vtp_amd import VTPTrainer
    img, txt = _data()
    img, txt = img.to(DEV), txt.to(DEV)
    kw = {}
    if layout != "shared":
        monkeypatch.setenv("VTP_SINGLE_GRAPH", "0")
        kw["reconstruction_image"] = torch.flip(img, dims=[-1]).contiguous()
    sd = _sd(feat, ae_only)
    res = []
    for use_graphs in (False, True):
        m = _model(feat, ae_only, sd)
        tr = VTPTrainer(m, lr=1e-3, weight_decay=0.0, use_graphs=use_graphs, max_grad_norm=1.0)
        if use_graphs and layout != "shared":
            assert not tr.single_graph
        res.append(_steps(m, tr, img, txt, 3, **kw))
    print("eager", res[0][0], "graph", res[1][0], "weights rel", relF(res[1][1], res[0][1]))
    for x, y in zip(res[0][0], res[1][0]):
        assert abs(x[0] - y[0]) < 1e-3 * abs(x[0]) and abs(x[1] - y[1]) < 5e-3 * abs(x[1]) + 1e-4
    # (the bar of tests/test_ssl_gpu.py.  The cases agree to ~1e-9, except (pooled, ae_only=True, separate rec input, segments), seen at
    # 2e-4 .. 6e-4 when it runs behind other tests in one process and at 8e-11 alone: an open finding)
    assert relF(res[1][1], res[0][1]) < 1e-3


# ------------------------------------------------------------------------------------------------------------------------- legacy VTP
def _vtp_cfg(feat, ae_only=False):
    from vtp_amd import VTPConfig
    return VTPConfig(image_size=64, vision_embed_dim=128, vision_depth=2, vision_num_heads=2, text_embed_dim=128, text_depth=1,
                     text_num_heads=2, text_vocab_size=64, text_context_length=8, decoder_embed_dim=128, decoder_depth=1,
                     decoder_num_heads=2, vision_clip_feat=feat, vision_bottleneck_ae_only=ae_only)


HEAD = dict(dino_out_dim=512, dino_hidden_dim=128, dino_bottleneck_dim=64)


def _vtp_sd(feat, ae_only=False):
    from vtp_amd import VTP
    torch.manual_seed(21)
    m = VTP(_vtp_cfg(feat, ae_only), **HEAD)
    with torch.no_grad():  # a teacher that differs from the student
        for p in m.teacher_trunk.parameters():
            p.add_(0.01 * torch.randn_like(p))
    return {k: v.clone() for k, v in m.state_dict().items()}


def _vtp(feat, sd, ae_only=False):
    from vtp_amd import VTP
    m = VTP(_vtp_cfg(feat, ae_only), **HEAD)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _ssl_data():
    g = torch.Generator().manual_seed(9)
    B, n_local = 3, 2
    gc = torch.randn(2 * B, 3, 64, 64, generator=g)
    lc = torch.randn(n_local * B, 3, 32, 32, generator=g)
    masks = torch.rand(2 * B, 16, generator=g) < 0.3
    masks[0, :3] = True
    img = torch.randn(B, 3, 64, 64, generator=g)
    txt = torch.randint(1, 60, (B, 8), generator=g)
    txt[:, 5] = 63
    return gc, lc, masks, img, txt, n_local


def _check_outputs(ours, r32, rbf):
    for k in r32:
        e, e_ref = relF(ours[k], r32[k]), relF(rbf[k], r32[k])
        print(f"{k}: E_ours={e:.3e} E_ref={e_ref:.3e} ratio {e / e_ref:.2f}")
        assert e <= 1.25 * e_ref, k


def test_vtp_tiny_ssl_and_clip_match_reference_fixture():
    """ours on the weights / inputs of the fixture recorded from the real reference (tests/golden/vtp_tiny_bottleneck_heads.safetensors,
    tools/record_bottleneck_heads.py): SSL output dicts and encode_image for cls and pooled; E_ref = the oracle under CUDA autocast"""
    import importlib.util
    import os
    from vtp_amd import VTP, VTPConfig
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("rbh", os.path.join(root, "tools", "record_bottleneck_heads.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g, meta, sd = tool.load()
    c = meta["cfg"]
    outs = {}
    for feat in ("cls", "pooled"):
        cfg = VTPConfig(image_size=c["R"], vision_embed_dim=c["embed_dim"], vision_depth=c["depth"], vision_num_heads=c["heads"],
                        text_embed_dim=c["embed_dim"], text_depth=c["text_layers"], text_num_heads=c["text_heads"],
                        text_vocab_size=c["vocab"], text_context_length=c["ctx"], decoder_embed_dim=c["embed_dim"],
                        decoder_depth=c["dec_depth"], decoder_num_heads=c["dec_heads"], vision_clip_feat=feat,
                        vision_bottleneck_ae_only=False)
        m = VTP(cfg, dino_out_dim=c["K"], dino_hidden_dim=c["hidden"], dino_bottleneck_dim=c["bott"])
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("pixel_decoder.") for k in missing), (missing, unexpected)
        m = m.to(DEV).eval()
        outs["enc." + feat] = m.encode_image(g["in.image"].to(DEV))
    masks = g["in.masks"].bool()
    nm = int(masks.sum())
    t_out, s_out = m(ssl_dict=dict(global_crops=g["in.global_crops"].to(DEV), n_global_crops=2, mask_indices_list=None,
                                   n_masked_patches=nm, upperbound=nm, local_crops=g["in.local_crops"].to(DEV), masks=masks.to(DEV)),
                     forward_type="ssl")
    outs.update({"teacher." + k: v for k, v in t_out.items() if torch.is_tensor(v)})
    outs.update({"student." + k: v for k, v in s_out.items()})
    sdd = {k: v.to(DEV) for k, v in sd.items()}
    sdd["visual_proj.weight"] = sdd["proj.weight"]
    from oracle import vtp_oracle as O
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        tb, sb = _oracle_ssl_outputs(sdd, g["in.global_crops"].to(DEV), g["in.local_crops"].to(DEV), masks.to(DEV), c["heads"])
        rbf = {"teacher." + k: v for k, v in tb.items()}
        rbf.update({"student." + k: v for k, v in sb.items()})
        for feat in ("cls", "pooled"):
            rbf["enc." + feat] = O.clip_image_feature(sdd, g["in.image"].to(DEV), c["heads"], False, feat, False)
    _check_outputs(outs, {k: g[k] for k in rbf}, rbf)


def test_vtp_b_ssl_outputs_at_bench_head():
    """VTP-B, K = 65 536, B = 2, vision_bottleneck_ae_only=False: the DINO head's K = 64 first layer and the bottleneck over hundreds of
    head rows at their real sizes; SSL output dicts vs the oracle composition (fp32, E_ref = CUDA autocast)"""
    from vtp_amd import VTP, VTPConfig
    from vtp_amd.data import collate_ssl_masks
    import numpy as np
    torch.manual_seed(31)
    m = VTP(VTPConfig(vision_bottleneck_ae_only=False), dino_out_dim=65536)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim <= 1 and n != "logit_scale" and not n.startswith("teacher_"):
                p.add_(0.05 * torch.randn_like(p))
        for p in m.teacher_trunk.parameters():
            p.add_(0.002 * torch.randn_like(p))
    assert tuple(m.dino_head.mlp[0].weight.shape) == (2048, 64)
    sd = {k: v.detach().to(DEV) for k, v in m.state_dict().items()}
    m = m.to(DEV).eval()
    B, n_local = 2, 2
    g = torch.Generator().manual_seed(7)
    gc = torch.randn(2 * B, 3, 224, 224, generator=g)
    lc = torch.randn(n_local * B, 3, 96, 96, generator=g)
    masks = torch.as_tensor(collate_ssl_masks(2 * B, (14, 14), 0.5, (0.1, 0.5), np.random.default_rng(11))["masks"]).bool()
    nm = int(masks.sum())
    t_out, s_out = m(ssl_dict=dict(global_crops=gc.to(DEV), n_global_crops=2, mask_indices_list=None, n_masked_patches=nm,
                                   upperbound=nm, local_crops=lc.to(DEV), masks=masks.to(DEV)), forward_type="ssl")
    ours = {**{k: v for k, v in t_out.items() if torch.is_tensor(v)}, **s_out}
    assert s_out["student_global_cls_tokens"].shape == (2 * B, 64)
    with torch.no_grad():
        t32, s32 = _oracle_ssl_outputs(sd, gc.to(DEV), lc.to(DEV), masks.to(DEV), 12)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            tbf, sbf = _oracle_ssl_outputs(sd, gc.to(DEV), lc.to(DEV), masks.to(DEV), 12)
    _check_outputs(ours, {**t32, **s32}, {**tbf, **sbf})


@pytest.mark.parametrize("feat,ae_only", [("cls", False), ("pooled", False), ("pooled", True)])
def test_vtp_full_step_vs_oracle(feat, ae_only):
    """rec + clip + ssl (KoLeo on the student global cls tokens -- 64-d with the bottleneck) in one VTPTrainer step: every bottleneck
    contribution reaches dW_bott; gradients vs the oracle (E_ours <= 1.25 E_ref, no floors)"""
    from vtp_amd import VTPTrainer
    gc, lc, masks, img, txt, n_local = _ssl_data()
    sd = _vtp_sd(feat, ae_only)
    m = _vtp(feat, sd, ae_only)
    tr = VTPTrainer(m, lr=0.0, weight_decay=0.0, koleo_weight=0.1, rec_weight=REC_W)
    tr.center_dino.zero_()
    tr.center_ibot.zero_()
    ssl = tr.prepare_ssl(gc.to(DEV), lc.to(DEV), masks)
    l_rec, l_clip = (float(v) for v in tr.step(img.to(DEV), txt.to(DEV), ssl))
    torch.cuda.synchronize()
    l_ssl = float(tr.ssl_loss_sum) + float(tr.koleo_loss_sum)
    params = dict(m.named_parameters())
    spec = (gc, lc, masks, n_local, 0.1, HEAD["dino_out_dim"])
    (r1, rc, rs), g32 = _oracle(sd, img, txt, feat, ae_only, "f32", ssl=spec)
    grefs = [_oracle(sd, img, txt, feat, ae_only, mode, ssl=spec)[1] for mode in ("cpu16", "gpu16")]
    print(f"{feat}/{ae_only}: rec {l_rec:.5f} ({r1:.5f}) clip {l_clip:.5f} ({rc:.5f}) ssl {l_ssl:.5f} ({rs:.5f})")
    assert abs(l_rec - r1) < 5e-3 * r1 and abs(l_clip - rc) < 1e-2 * rc and abs(l_ssl - rs) < 1e-2 * abs(rs)
    _judge(params, g32, grefs, ["trunk.feature_bottleneck.weight", "visual_proj.weight", "dino_head.mlp.0.weight",
                                "trunk.blocks.0.attn.qkv.weight", "trunk.blocks.1.mlp.w3.weight", "trunk.patch_embed.proj.weight",
                                "trunk.mask_token", "trunk.norm.weight"])


def test_vtp_full_step_graph_equals_eager():
    from vtp_amd import VTPTrainer
    gc, lc, masks, img, txt, _ = _ssl_data()
    sd = _vtp_sd("pooled")
    res = []
    for use_graphs in (False, True):
        m = _vtp("pooled", sd)
        tr = VTPTrainer(m, lr=5e-4, weight_decay=0.0, use_graphs=use_graphs, koleo_weight=0.1)
        ssl = tr.prepare_ssl(gc.to(DEV), lc.to(DEV), masks)
        hist = []
        for _ in range(3):
            r, c = tr.step(img.to(DEV), txt.to(DEV), ssl)
            hist.append((float(r), float(c), float(tr.ssl_loss_sum)))
        torch.cuda.synchronize()
        res.append((hist, m._store.flat_p.clone()))
    print("eager:", res[0][0])
    print("graph:", res[1][0], "weights rel", relF(res[1][1], res[0][1]))
    for a, b in zip(res[0][0], res[1][0]):
        for x, y in zip(a, b):
            assert abs(x - y) < 1e-2 * abs(x) + 2e-4
    assert relF(res[1][1], res[0][1]) < 1e-3
