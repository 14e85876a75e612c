"""The switchable fp32 inference forward (VTPModel.enable_fp32_forward) end to end.

Target: the reference with fp32 weights and no autocast = oracle/vtp_oracle.py on fp32 tensors, which reproduces the real reference's
outputs in tests/golden/vtp_tiny.safetensors.  For every output three figures (relF = relative Frobenius error, in fp64):
    E_ours = relF(ours, oracle evaluated in fp64)
    E_32   = relF(oracle in fp32, oracle in fp64)        the reference's own fp32 rounding error
    E_bf16 = relF(our bf16 path, oracle in fp64)
and the requirement  E_ours <= max(4 E_32, 2e-6)  and  E_ours <= 0.1 E_bf16.  The second inequality shows that fp32 is in effect.
The vision E_32 carry the heavy tail of apply_rope's cast to bf16 (an fp32 rounding difference becomes an occasional 2^-9 flip); the
factor 4 is the project's convention (tests/augment_ref.py).

Measured on one MI355X (E_ours / E_32 / E_bf16), tiny golden fixture, all three towers in fp32:
    see profiles/README.md, "fp32 inference forward" (copied from this file's output)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ("trunk", "decoder", "text")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(sd=None, seed=0, **over):
    from oracle.ref_stubs import TINY
    from vtp_amd import VTPConfig, VTPModel
    torch.manual_seed(seed)
    m = VTPModel(VTPConfig(**{**TINY, **over}))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def tiny(golden_sd):
    return _model(golden_sd)


def relF(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def to64(sd):
    return {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}  # (the RoPE periods stay bf16)


def cpu_sd(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def oracle_pair(fn, sd):
    """fn(sd, cast) evaluated by the oracle in fp32 and in fp64 on the CPU"""
    with torch.no_grad():
        return fn(sd, lambda t: t), fn(to64(sd), lambda t: t.double())


def check(name, ours, bf16, o32, o64):
    e_ours, e_32, e_bf = relF(ours, o64), relF(o32, o64), relF(bf16, o64)
    print(f"fp32 forward {name}: E_ours={e_ours:.3e} E_32={e_32:.3e} (x{e_ours / max(e_32, 1e-300):.2f}) E_bf16={e_bf:.3e}")
    assert ours.dtype == torch.float32 and torch.isfinite(ours).all()
    assert e_ours <= max(4 * e_32, 2e-6), f"{name}: E_ours {e_ours:.3e} > max(4 E_32, 2e-6), E_32 = {e_32:.3e}"
    assert e_ours <= 0.1 * e_bf, f"{name}: E_ours {e_ours:.3e} > 0.1 E_bf16 = {0.1 * e_bf:.3e}"


def run_all(model, img, text, heads=(2, 2, 2), towers=ALL, pool="argmax", causal=True, quick=False, tag=""):
    """every API output in bf16, then in fp32, against the oracle; returns the fp32 outputs"""
    from oracle import vtp_oracle as O
    vis, dec, txt = heads
    sd = cpu_sd(model)
    img_d, text_d = img.to(DEV), (text.to(DEV) if text is not None else None)

    def outputs():
        o = {}
        o["latents"] = model.get_reconstruction_latents(img_d)
        o["reconstruction"] = model.get_latents_decoded_images(o["latents"])
        f = model.get_last_layer_feature(img_d)
        o["last_cls"], o["last_patch"] = f["cls_token"], f["patch_tokens"]
        if text is not None:
            o["clip_image_feature"] = model.get_clip_image_feature(img_d)
            o["clip_text_feature"] = model.get_clip_text_feature(text_d)
            o["clip_logits"] = model.get_clip_logits(img_d, text_d)[0]
        return o

    model.disable_fp32_forward()
    b = outputs()
    model.enable_fp32_forward(towers)
    try:
        assert model.fp32_forward == tuple(t for t in ALL if t in towers)
        f = outputs()
    finally:
        model.disable_fp32_forward()

    def ref(s, c):
        r = {"latents": O.reconstruction_latents(s, c(img), vis)}
        r["reconstruction"] = O.decoder_forward(s, r["latents"], dec)
        t = O.trunk_forward(s, c(img), vis, use_bottleneck=False)
        r["last_cls"], r["last_patch"] = t["x_norm_clstoken"], t["x_norm_patchtokens"]
        if text is not None:
            r["clip_image_feature"] = O.clip_image_feature(s, c(img), vis)
            r["clip_text_feature"] = O.clip_text_feature(s, text, txt, pool_type=pool, causal=causal, quick_gelu=quick)
            r["clip_logits"] = s["logit_scale"].exp() * r["clip_image_feature"] @ r["clip_text_feature"].T
        return r

    r32, r64 = oracle_pair(ref, sd)
    for k in f:
        check(tag + k, f[k], b[k], r32[k], r64[k])
    return f, r32, r64


def test_against_the_real_reference(tiny, golden, golden_sd):
    from oracle import vtp_oracle as O
    img, text = golden["in.image"], golden["in.text"]
    f, r32, r64 = run_all(tiny, img, text, tag="golden ")
    for k in f:  # the oracle in fp32 is the real reference's output: ours against the recorded tensors themselves, for the record
        print(f"fp32 forward golden {k}: relF(ours, recorded reference) = {relF(f[k], golden['out.' + k]):.3e}; "
              f"relF(oracle fp32, recorded) = {relF(r32[k], golden['out.' + k]):.3e}")
    # the decoder alone: decoded from the golden latents
    lat = golden["out.latents"]
    bf = tiny.get_latents_decoded_images(lat.to(DEV))
    tiny.enable_fp32_forward(ALL)
    try:
        ours = tiny.get_latents_decoded_images(lat.to(DEV))
        out = tiny(image=img.to(DEV), forward_type="rec")
        assert torch.equal(out["latents"], f["latents"]) and torch.equal(out["reconstructed_image"], f["reconstruction"])
        clip = tiny(image=img.to(DEV), text=text.to(DEV), forward_type="clip")
        assert torch.equal(clip["image_features"], f["clip_image_feature"]) and torch.equal(clip["text_features"], f["clip_text_feature"])
    finally:
        tiny.disable_fp32_forward()
    o32, o64 = oracle_pair(lambda s, c: O.decoder_forward(s, c(lat), 2), golden_sd)
    check("golden decoder on golden latents", ours, bf, o32, o64)


def test_subsets_and_disable(tiny, golden, golden_sd):
    from oracle import vtp_oracle as O
    img, text = golden["in.image"].to(DEV), golden["in.text"].to(DEV)
    lat_b = tiny.get_reconstruction_latents(img)
    rec_b = tiny.get_latents_decoded_images(lat_b)
    fi_b, ft_b = tiny.get_clip_image_feature(img), tiny.get_clip_text_feature(text)
    try:
        tiny.enable_fp32_forward(("decoder",))  # tools/test_reconstruction_hf.py: bf16 encoder, fp32 decoder
        assert tiny.fp32_forward == ("decoder",)
        lat = tiny.get_reconstruction_latents(img)
        assert torch.equal(lat, lat_b), "('decoder',) changed the latents"
        rec = tiny.get_latents_decoded_images(lat)
        o32, o64 = oracle_pair(lambda s, c: O.decoder_forward(s, c(lat_b.cpu()), 2), golden_sd)
        check("decoder-only reconstruction", rec, rec_b, o32, o64)
        assert torch.equal(tiny.get_clip_text_feature(text), ft_b)
        tiny.enable_fp32_forward("text")
        assert tiny.fp32_forward == ("text",)
        assert torch.equal(tiny.get_clip_image_feature(img), fi_b), "('text',) changed the image feature"
        assert torch.equal(tiny.get_reconstruction_latents(img), lat_b)
        assert not torch.equal(tiny.get_clip_text_feature(text), ft_b)
    finally:
        tiny.disable_fp32_forward()
    assert tiny.fp32_forward == ()
    assert torch.equal(tiny.get_reconstruction_latents(img), lat_b) and torch.equal(tiny.get_latents_decoded_images(lat_b), rec_b)
    assert torch.equal(tiny.get_clip_image_feature(img), fi_b) and torch.equal(tiny.get_clip_text_feature(text), ft_b)


def test_resident_attention_sizes_mlp_layerscale():
    """256 x 256, B = 2: N = 257 in the trunk, 256 in the decoder; the decoder runs LayerNorm + Mlp + LayerScale"""
    m = _model(seed=3, decoder_ffn_layer="mlp", decoder_init_values=0.1, text_ls_init_value=0.5, text_no_causal_mask=True)
    g = torch.Generator().manual_seed(21)
    img = torch.randn(2, 3, 256, 256, generator=g)
    text = torch.randint(0, 512, (2, 16), generator=g)
    run_all(m, img, text, causal=False, tag="256x256 ")


def test_non_square_quick_gelu_last_pool_and_pooled_feature():
    m = _model(seed=4, text_quick_gelu=True, text_pool_type="last", vision_init_values=0.2)
    g = torch.Generator().manual_seed(22)
    img = torch.randn(3, 3, 64, 96, generator=g)
    text = torch.randint(0, 512, (3, 16), generator=g)
    run_all(m, img, text, pool="last", quick=True, tag="64x96 ")


def test_wide_trunks():
    """one tower at each wide preset's width (1152 / 18 heads / ratio 3.7778, 1280 / 20, 1536 / 24): norm_fwd_f32 in its 8-chunk
    instantiation, fp32 GEMMs with N and K tails"""
    m = _model(seed=6, vision_embed_dim=1152, vision_num_heads=18, vision_depth=1, vision_mlp_ratio=3.777777778, decoder_embed_dim=1280,
               decoder_num_heads=20, decoder_depth=1, text_embed_dim=1536, text_num_heads=24, text_depth=1)
    g = torch.Generator().manual_seed(24)
    img = torch.randn(2, 3, 64, 96, generator=g)
    text = torch.randint(0, 512, (2, 16), generator=g)
    run_all(m, img, text, heads=(18, 20, 24), tag="wide ")


def test_pooled_bottlenecked_feature_none_pool_and_intermediate_layers():
    from oracle import vtp_oracle as O
    m = _model(seed=5, vision_clip_feat="pooled", vision_bottleneck_ae_only=False, text_pool_type="none", text_embed_cls=True)
    sd = cpu_sd(m)
    g = torch.Generator().manual_seed(23)
    img = torch.randn(2, 3, 64, 64, generator=g)
    text = torch.randint(0, 512, (2, 17), generator=g)
    fi_b, ft_b = m.get_clip_image_feature(img.to(DEV)), m.get_clip_text_feature(text.to(DEV))
    il_b = m.get_intermediate_layers_feature(img.to(DEV), n=2, return_class_token=True)
    fb_b = m.get_last_layer_feature(img.to(DEV), use_bottleneck=True)
    m.enable_fp32_forward()
    try:
        fi, ft = m.get_clip_image_feature(img.to(DEV)), m.get_clip_text_feature(text.to(DEV))
        il = m.get_intermediate_layers_feature(img.to(DEV), n=2, return_class_token=True)
        fb = m.get_last_layer_feature(img.to(DEV), use_bottleneck=True)
    finally:
        m.disable_fp32_forward()
    o32, o64 = oracle_pair(lambda s, c: O.clip_image_feature(s, c(img), 2, clip_feat="pooled", ae_only=False), sd)
    check("pooled + bottleneck image feature", fi, fi_b, o32, o64)
    o32, o64 = oracle_pair(lambda s, c: O.clip_text_feature(s, text, 2, pool_type="none"), sd)
    assert ft.shape == (2, 17, 128)
    check("per-token text feature", ft, ft_b, o32, o64)
    o32, o64 = oracle_pair(lambda s, c: O.intermediate_layers(s, c(img), 2, n=2, return_class_token=True), sd)
    for j in range(2):
        check(f"intermediate layer {j} patch", il[j][0], il_b[j][0], o32[j][0], o64[j][0])
        check(f"intermediate layer {j} cls", il[j][1], il_b[j][1], o32[j][1], o64[j][1])
    o32, o64 = oracle_pair(lambda s, c: O.trunk_forward(s, c(img), 2, use_bottleneck=True), sd)
    check("bottlenecked cls", fb["cls_token"], fb_b["cls_token"], o32["x_norm_clstoken"], o64["x_norm_clstoken"])
    check("bottlenecked patch", fb["patch_tokens"], fb_b["patch_tokens"], o32["x_norm_patchtokens"], o64["x_norm_patchtokens"])


def test_weights_move(golden, golden_sd):
    """an in-place parameter change shows in the next fp32 forward; VTPTrainer.step keeps training in bf16 and the eval call behind it is
    fp32 on the updated weights"""
    from oracle import vtp_oracle as O
    from vtp_amd import VTPTrainer
    img, text = golden["in.image"], golden["in.text"]
    m, twin = _model(golden_sd), _model(golden_sd)
    m.enable_fp32_forward()
    ft0 = m.get_clip_text_feature(text.to(DEV))
    lat0 = m.get_reconstruction_latents(img.to(DEV))
    with torch.no_grad():
        m.text_projection.mul_(1.5)
        m.trunk.norm.weight.add_(0.25)
        m.trunk.blocks[1].mlp.w2.weight.mul_(0.5)
    sd = cpu_sd(m)
    ft, lat = m.get_clip_text_feature(text.to(DEV), normalize=False), m.get_reconstruction_latents(img.to(DEV))
    assert not torch.equal(lat, lat0)
    o32, o64 = oracle_pair(lambda s, c: O.clip_text_feature(s, text, 2, normalize=False), sd)
    assert relF(ft, o64) <= max(4 * relF(o32, o64), 2e-6), "text_projection's derived copy was not refreshed"
    o32, o64 = oracle_pair(lambda s, c: O.reconstruction_latents(s, c(img), 2), sd)
    assert relF(lat, o64) <= max(4 * relF(o32, o64), 2e-6)
    # a training step: bf16 whatever the switch says (the twin has it off), then an fp32 eval on the updated weights
    twin.load_state_dict(sd, strict=True)
    m.train(), twin.train()
    l1 = VTPTrainer(m, lr=1e-3).step_rec(img.to(DEV))
    l2 = VTPTrainer(twin, lr=1e-3).step_rec(img.to(DEV))
    # the loss is a sum of per-workgroup partials added with float atomics: its last bits depend on their order (a few 2^-24 of it), while
    # an fp32 forward would move the reconstruction by E_bf16 ~ 4e-3; and what the step saved for its backward is the bf16 path's
    print(f"weights move: training loss with the switch on {float(l1):.8f}, off {float(l2):.8f}")
    assert abs(float(l1) - float(l2)) <= 1e-5 * float(l2), "the training step changed with the fp32 switch on"
    assert m._trunk.stack.last_saved[0].qkv.dtype == torch.bfloat16 and m._decoder.stack.last_saved[0].qkv.dtype == torch.bfloat16
    m.eval()
    sd2 = cpu_sd(m)
    assert m.fp32_forward == ALL and not torch.equal(sd2["trunk.norm.weight"], sd["trunk.norm.weight"])
    lat = m.get_reconstruction_latents(img.to(DEV))
    rec = m.get_latents_decoded_images(lat)
    ft = m.get_clip_text_feature(text.to(DEV))
    twin.load_state_dict(sd2, strict=True)  # the bf16 path on the same updated weights
    twin.eval()
    ref = lambda s, c: O.decoder_forward(s, O.reconstruction_latents(s, c(img), 2), 2)
    o32, o64 = oracle_pair(ref, sd2)
    check("after a training step: reconstruction", rec, twin.get_latents_decoded_images(twin.get_reconstruction_latents(img.to(DEV))), o32, o64)
    o32, o64 = oracle_pair(lambda s, c: O.clip_text_feature(s, text, 2), sd2)
    check("after a training step: text feature", ft, twin.get_clip_text_feature(text.to(DEV)), o32, o64)
    assert ft0.shape == ft.shape


def test_batch_invariance_end_to_end(tiny, golden):
    img = golden["in.image"].to(DEV)
    tiny.enable_fp32_forward()
    try:
        lat3 = tiny.get_reconstruction_latents(img)
        rec3 = tiny.get_latents_decoded_images(lat3)
        lat1 = tiny.get_reconstruction_latents(img[:1])
        rec1 = tiny.get_latents_decoded_images(lat1)
        assert torch.equal(lat3, tiny.get_reconstruction_latents(img)), "two runs differ"
    finally:
        tiny.disable_fp32_forward()
    assert torch.equal(lat1, lat3[:1]) and torch.equal(rec1, rec3[:1]), "image 0 alone differs from image 0 in a batch of 3"


def test_recon_eval_runs_on_the_fp32_decoder(tiny, golden):
    from vtp_amd import ReconEval, ops
    img = golden["in.image"].to(DEV)
    tiny.enable_fp32_forward(("decoder",))
    try:
        ev = ReconEval(tiny)
        out = ev.update(img, want_u8=True)
        rec = tiny.get_latents_decoded_images(tiny.get_reconstruction_latents(img))
    finally:
        tiny.disable_fp32_forward()
    rec_bf = tiny.get_latents_decoded_images(tiny.get_reconstruction_latents(img))
    assert not torch.equal(rec, rec_bf)
    u8 = torch.empty(3, 64, 64, 3, dtype=torch.uint8, device=DEV)
    ops.images_to_u8(rec, u8, ev.sub, ev.div)
    assert torch.equal(out.rec_u8, u8) and torch.isfinite(out.psnr).all()


def test_patch_model_carries_the_switch(golden, golden_sd):
    from types import SimpleNamespace
    from oracle.ref_stubs import TINY
    from vtp_amd import VTPConfig, patch_model
    ref = SimpleNamespace(config=VTPConfig(**TINY), state_dict=lambda: golden_sd, training=False)
    p = patch_model(ref, DEV)
    assert p.fp32_forward == ()
    lat_b = p.get_reconstruction_latents(golden["in.image"].to(DEV))
    p.enable_fp32_forward(("trunk",))
    assert p.fp32_forward == ("trunk",) and p._vtp_amd.fp32_forward == ("trunk",)
    assert not torch.equal(p.get_reconstruction_latents(golden["in.image"].to(DEV)), lat_b)
    p.disable_fp32_forward()
    assert p.fp32_forward == () and torch.equal(p.get_reconstruction_latents(golden["in.image"].to(DEV)), lat_b)


def test_cases_that_must_raise(tiny, golden):
    img = golden["in.image"].to(DEV)
    with pytest.raises(ValueError, match="unknown tower"):
        tiny.enable_fp32_forward(("trunk", "teacher"))
    with pytest.raises(ValueError, match="at least one"):
        tiny.enable_fp32_forward(())
    assert tiny.fp32_forward == ()
    with pytest.raises(ValueError, match="pixel decoder"):
        _model(train_reconstruction=False).enable_fp32_forward(("decoder",))
    with pytest.raises(ValueError, match="text tower"):
        _model(train_clip=False).enable_fp32_forward(("trunk", "text"))
    qk = _model(vision_use_qk_norm=True, decoder_use_qk_norm=True)
    with pytest.raises(NotImplementedError, match="qk_norm"):
        qk.enable_fp32_forward(("trunk",))
    with pytest.raises(NotImplementedError, match="qk_norm"):
        qk.enable_fp32_forward(("decoder",))
    assert qk.fp32_forward == ()
    qk.enable_fp32_forward(("text",))  # the text tower has no QK norm
    # fp8 and fp32 on the same tower exclude each other, whichever comes first (widths at which the fp8 forward exists)
    wide = dict(vision_embed_dim=192, vision_num_heads=3, decoder_embed_dim=192, decoder_num_heads=3)
    m = _model(**wide)
    m.enable_fp8_forward(img)
    with pytest.raises(ValueError, match="fp8"):
        m.enable_fp32_forward(("decoder",))
    m.enable_fp32_forward(("text",))
    m.disable_fp8_forward()
    m.enable_fp32_forward(("trunk", "text"))
    with pytest.raises(ValueError, match="fp32"):
        m.enable_fp8_forward(img)
    assert m.fp32_forward == ("trunk", "text")
