"""Pins the oracle restatement against the REAL reference: its classes' outputs are recorded in tests/golden/ref_pins.safetensors
by oracle/make_golden_refpins.py, together with the weights and inputs they ran with (regenerated from seeds where that is exact),
so these checks need nothing outside the repository.  A large output is kept at fixed sampled positions: `_vs` compares the full
shape and those elements."""
import numpy as np
import pytest
import torch

from oracle import vtp_oracle as O
from oracle.make_golden_refpins import CLIP_FEAT, CROPS, EMBED_CLS, FFN, TEXT_POOL, YAML_DOC, crop_inputs, digest, load, pinned_state, seen
from oracle.ref_stubs import TINY


@pytest.fixture(scope="module")
def pins():
    return load()


def _sd(pins, case):
    g, meta = pins
    return pinned_state(g, meta, case)


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _vs(pins, name, got):
    """(got, recorded output `name`), both as the fixture keeps it, after checking got's full shape"""
    g, meta = pins
    case, out = name.split("/", 1)
    assert list(got.shape) == meta[case]["shapes"][out], (name, tuple(got.shape))
    ref = g[name]
    return seen(got, ref), ref


def _shapes(pins, case):
    return {k: tuple(shape) for k, shape, *_ in pins[1][case]["keys"]}


@pytest.fixture(scope="module")
def ref_sd(pins):
    return _sd(pins, "base")


@pytest.mark.parametrize("res", [(96, 96), (64, 128)])
def test_encode_decode(pins, ref_sd, res):
    g = pins[0]
    p = f"base/ed{res[0]}x{res[1]}/"
    with torch.no_grad():
        lat = O.reconstruction_latents(ref_sd, g[p + "img"], 2)
        rec = O.decoder_forward(ref_sd, lat, 2)
    torch.testing.assert_close(*_vs(pins, p + "lat", lat), rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(*_vs(pins, p + "rec", rec), rtol=2e-4, atol=2e-5)


def test_clip(pins, ref_sd):
    g = pins[0]
    with torch.no_grad():
        lo = O.clip_logits(ref_sd, g["base/clip/img"], g["base/clip/text"], 2, 2)
    torch.testing.assert_close(*_vs(pins, "base/clip/logits", lo), rtol=1e-4, atol=1e-4)


def test_masked_trunk(pins, ref_sd):
    g = pins[0]
    with torch.no_grad():
        o = O.trunk_forward(ref_sd, g["base/masked/img"], 2, use_bottleneck=False, masks=g["base/masked/masks"])
    torch.testing.assert_close(*_vs(pins, "base/masked/patch", o["x_norm_patchtokens"]), rtol=2e-4, atol=2e-5)


def test_lpips(pins):
    """oracle LPIPS == the reference's LPIPS class (vtp/utils/lpips.py) on the same seeded weights, eval mode."""
    from oracle import lpips_oracle as L
    g = pins[0]
    sd = L.make_state(3)
    with torch.no_grad():
        torch.testing.assert_close(*_vs(pins, "lpips/out", L.lpips(sd, g["lpips/x0"], g["lpips/x1"])), rtol=1e-5, atol=1e-7)


def test_intermediate_layers(pins, ref_sd):
    g = pins[0]
    img = g["base/inter/img"]
    with torch.no_grad():
        got = O.intermediate_layers(ref_sd, img, 2, n=2, reshape=False, return_class_token=True, norm=True)
        assert len(got) == 2
        for i, g_ in enumerate(got):
            torch.testing.assert_close(*_vs(pins, f"base/inter/a{i}/0", g_[0]), rtol=2e-4, atol=2e-5)
            torch.testing.assert_close(*_vs(pins, f"base/inter/a{i}/1", g_[1]), rtol=2e-4, atol=2e-5)
        got = O.intermediate_layers(ref_sd, img, 2, n=[0, 2], reshape=True, return_class_token=False, norm=False)
        assert len(got) == 2
        for i, g_ in enumerate(got):
            torch.testing.assert_close(*_vs(pins, f"base/inter/b{i}", g_), rtol=2e-4, atol=2e-5)


def test_layerscale_and_stochastic_depth_branch(pins):
    """LayerScale (vision_init_values) and the training branch with sample drop (block.py:207-233) of the REAL trunk vs the
    oracle fed with the image subsets the reference drew (torch.randperm, replayed from the same seed in call order)."""
    g = pins[0]
    sd = _sd(pins, "ls")
    assert "trunk.blocks.0.ls1.gamma" in sd and "pixel_decoder.blocks.1.ls2.gamma" in sd
    img = g["ls/img"]
    with torch.no_grad():
        torch.testing.assert_close(*_vs(pins, "ls/lat", O.reconstruction_latents(sd, img, 2)), rtol=2e-4, atol=2e-5)
        torch.testing.assert_close(*_vs(pins, "ls/rec", O.decoder_forward(sd, g["ls/lat"], 2)), rtol=2e-4, atol=2e-5)
    # training branch: drop_ratio 0.4 on 5 images -> keep 3, alpha 5/3
    ratio, B = 0.4, 5
    torch.manual_seed(11)
    keep = max(int(B * (1 - ratio)), 1)
    drop = []
    for _ in range(3):
        i1 = torch.randperm(B)[:keep]
        i2 = torch.randperm(B)[:keep]
        drop.append((i1, B / keep, i2, B / keep))
    with torch.no_grad():
        o = O.trunk_forward(sd, img, 2, use_bottleneck=False, drop=drop)
    torch.testing.assert_close(*_vs(pins, "ls/drop/patch", o["x_norm_patchtokens"]), rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(*_vs(pins, "ls/drop/cls", o["x_norm_clstoken"]), rtol=2e-4, atol=2e-5)


def test_center_crop_arr_matches_reference(pins):
    """vtp_amd.tokenizer.center_crop_arr vs vtp/utils/image_utils.py:5-33 on the same images"""
    from vtp_amd.tokenizer import center_crop_arr
    for j, (im, size) in enumerate(crop_inputs()):
        a = np.asarray(center_crop_arr(im, size))
        assert a.shape == (size, size, 3) and digest(torch.from_numpy(np.array(a))) == pins[1]["crop"][str(j)], CROPS[j]


def test_from_vtp_yaml_matches_reference(pins, tmp_path):
    """VTPConfig.from_vtp_yaml against the reference classmethod (configuration_vtp.py:169-234) on a synthetic legacy YAML"""
    import json

    import yaml
    from vtp_amd import VTPConfig
    path = str(tmp_path / "legacy.yaml")
    with open(path, "w") as fh:
        yaml.safe_dump(YAML_DOC, fh)
    ours = VTPConfig.from_vtp_yaml(path)
    rd = pins[1]["yaml"]["to_dict"]
    for k, v in ours.to_dict().items():
        assert rd[k] == json.loads(json.dumps(v)), (k, rd[k], v)
    bad = dict(YAML_DOC)
    bad["data"] = {}
    with open(path, "w") as fh:
        yaml.safe_dump(bad, fh)
    with pytest.raises(KeyError):
        VTPConfig.from_vtp_yaml(path)


def test_qk_norm_branch_matches_reference(pins):
    """use_qk_norm (attention.py:67-68,119-120) in trunk and pixel decoder: oracle == reference, outputs and gradients"""
    g = pins[0]
    sd = {k: v.clone().requires_grad_(v.dtype == torch.float32) for k, v in _sd(pins, "qk").items()}
    assert any("q_norm.weight" in k for k in sd)
    img = g["qk/img"]
    lat = O.reconstruction_latents(sd, img, 2)
    rec = O.decoder_forward(sd, lat, 2)
    torch.testing.assert_close(*_vs(pins, "qk/lat", lat), rtol=2e-4, atol=2e-5)
    # the decoder's bf16 RoPE tables round a few entries differently when the recording host's and this host's fp32 arithmetic
    # differ in the last bit: compared as a whole, at the element tolerance of the rest of this file
    assert _rel(*_vs(pins, "qk/rec", rec)) < 2e-4
    (rec - img).abs().mean().backward()
    for k in ("trunk.blocks.0.attn.q_norm.weight", "trunk.blocks.1.attn.k_norm.weight", "pixel_decoder.blocks.0.attn.q_norm.weight",
              "trunk.blocks.0.attn.qkv.weight"):
        torch.testing.assert_close(*_vs(pins, f"qk/grad/{k}", sd[k].grad), rtol=2e-3, atol=1e-6)


def test_patch_model_config_and_keys_against_the_real_class(pins, ref_sd):
    """the host half of vtp_amd.patch_model on the reference instance's recorded config and state dict: its PretrainedConfig
    translates to our VTPConfig and its state_dict loads strict=True into our parameter tree (the device half runs in
    tests/test_boundary_gpu.py)"""
    from vtp_amd import VTPModel
    from vtp_amd.patch import API_METHODS, _our_config

    class RefConfig:  # the surface _our_config reads
        def __init__(self, d):
            self._d = d
            self.__dict__.update(d)

        def to_dict(self):
            return dict(self._d)

    rc = RefConfig(pins[1]["base"]["config"])
    cfg = _our_config(rc)
    assert cfg.vision_embed_dim == rc.vision_embed_dim and cfg.vision_depth == rc.vision_depth
    ours = VTPModel(cfg)
    ours.load_state_dict(ref_sd, strict=True)
    callable_on_ref = set(pins[1]["base"]["api_callable"])
    for name in API_METHODS:
        assert name in callable_on_ref and callable(getattr(ours, name)), name


@pytest.mark.parametrize("clip_feat,ae_only", CLIP_FEAT)
def test_clip_image_feature_variants_match_reference(pins, clip_feat, ae_only):
    """vision_clip_feat='pooled' (mean of the patch tokens, modeling_vtp.py:269) and vision_bottleneck_ae_only=False (the CLIP
    head sees the bottlenecked features, :252-262) -- the oracle branches behind vtp_amd's torch-head path -- plus the SigLIP
    logit bias (:330-331)"""
    case = f"clipfeat{CLIP_FEAT.index((clip_feat, ae_only))}"
    g = pins[0]
    sd = _sd(pins, case)
    img, text = g[case + "/img"], g[case + "/text"]
    with torch.no_grad():
        f = O.clip_image_feature(sd, img, 2, clip_feat=clip_feat, ae_only=ae_only)
        torch.testing.assert_close(*_vs(pins, case + "/feat", f), rtol=1e-4, atol=1e-5)
        t = O.clip_text_feature(sd, text, 2)
        lo = sd["logit_scale"].exp() * f @ t.T + sd["logit_bias"]
        torch.testing.assert_close(*_vs(pins, case + "/logits", lo), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("pool,no_causal,ls,quick", TEXT_POOL)
def test_text_pooling_and_mask_variants_match_reference(pins, pool, no_causal, ls, quick):
    """text_global_pool first / last, no_causal_mask, LayerScale and QuickGELU (text_transformer.py:213-228,285-288; block.py:388,399,
    425-426; layers/activation.py:5-12) --
    the oracle branches behind the round-4 text-tower variants, against the real class (state_dict keys / shapes of ours too)"""
    from vtp_amd import VTPConfig, VTPModel
    case = f"textpool{TEXT_POOL.index((pool, no_causal, ls, quick))}"
    g = pins[0]
    kw = dict(TINY, text_pool_type=pool, text_no_causal_mask=no_causal, text_ls_init_value=ls, text_quick_gelu=quick)
    assert {k: tuple(v.shape) for k, v in VTPModel(VTPConfig(**kw)).state_dict().items()} == _shapes(pins, case)
    sd = _sd(pins, case)
    with torch.no_grad():
        got = O.clip_text_feature(sd, g[case + "/text"], 2, pool_type=pool, causal=not no_causal, quick_gelu=quick)
    torch.testing.assert_close(*_vs(pins, case + "/feat", got), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("embed_cls,pool", EMBED_CLS)
def test_text_embed_cls_and_pool_none_match_reference(pins, embed_cls, pool):
    """text_embed_cls and text_pool_type = "none" AT THE CLASS BOUNDARY (round 5).  What the reference class does with them
    (modeling_vtp.py:142-170,296-310): it re-hangs TextTransformer's parts, so embed_cls leaves a positional table / causal mask of
    context_length + 1 positions but NO cls_emb and no padding mask (text_transformer.py:340-357 is never reached) -- captions must then
    carry context_length + 1 ids (the stock length fails in `x + positional_embedding`); pool "none" returns every token's projected,
    normalised feature [B, T, D] and get_clip_logits fails in its matmul.  Pinned here: state_dict keys / shapes of ours, the oracle
    against the real class, and the error cases (recorded from the real class; the oracle fails on the other length too)."""
    from vtp_amd import VTPConfig, VTPModel
    case = f"embedcls{EMBED_CLS.index((embed_cls, pool))}"
    g, meta = pins
    kw = dict(TINY, text_embed_cls=embed_cls, text_pool_type=pool)
    ours = VTPModel(VTPConfig(**kw))
    shapes = _shapes(pins, case)
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == shapes
    L = TINY["text_context_length"]
    T = L + 1 if embed_cls else L
    assert ours.config.text_num_pos == T == shapes["positional_embedding"][0] and not any("cls_emb" in k for k in shapes)
    sd = _sd(pins, case)
    text = g[case + "/text"]
    assert text.shape == (3, T)
    with torch.no_grad():
        got = O.clip_text_feature(sd, text, 2, pool_type=pool)
    assert meta[case]["shapes"]["feat"] == ([3, T, TINY["text_embed_dim"]] if pool == "none" else [3, TINY["text_embed_dim"]])
    torch.testing.assert_close(*_vs(pins, case + "/feat", got), rtol=1e-4, atol=1e-5)
    assert meta[case]["other_length_raises"]  # the other caption length does not fit the positional table
    with pytest.raises(RuntimeError):
        O.clip_text_feature(sd, torch.randint(1, 500, (3, L if embed_cls else L + 1)), 2, pool_type=pool)
    assert meta[case]["clip_logits_raises"] == (pool == "none")


def test_rope_train_time_augmentations_match_reference(pins):
    """RopePositionEmbedding's shift / jitter / rescale of the patch coordinates in training mode (embeddings.py:155-171): the oracle's
    augmented tables and where the towers draw them -- the trunk inside its block loop (vision_transformer.py:228-233: new coordinates
    per block), the pixel decoder once per forward (pixel_decoder.py:144) -- against the real class consuming the same global RNG
    stream"""
    g = pins[0]
    sd = _sd(pins, "rope")
    img, lat_ref = g["rope/img"], g["rope/lat"]
    torch.manual_seed(11)
    draws = [O.rope_aug_draw(0.1, 1.2, 1.5) for _ in range(TINY["vision_depth"])]
    with torch.no_grad():
        pt = O.trunk_forward(sd, img, 2, rope_aug=draws)["x_norm_patchtokens"]
        lat = pt.transpose(1, 2).reshape(2, -1, 4, 4)
        plain = O.reconstruction_latents(sd, img, 2)
    # bit-identical on the host that recorded the fixture; on another CPU the bf16 RoPE tables can round a few entries the other way
    torch.testing.assert_close(lat, lat_ref, rtol=2e-4, atol=2e-5)
    assert not torch.allclose(plain, lat_ref, atol=1e-5)
    torch.manual_seed(12)
    d = O.rope_aug_draw(0.1, 1.2, 1.5)
    with torch.no_grad():
        rec = O.decoder_forward(sd, lat_ref, 2, rope_aug=d)
    assert _rel(*_vs(pins, "rope/rec", rec)) < 2e-4
    torch.testing.assert_close(*_vs(pins, "rope/lat_eval", plain), rtol=1e-4, atol=1e-5)  # evaluation mode: no augmentation


@pytest.mark.parametrize("vis,dec", FFN)
def test_ffn_layer_variants_match_reference(pins, vis, dec):
    """ffn_layer = "mlp" (GELU Mlp, ffn.py:21-48) and the aligned SwiGLU widths (vision_transformer.py:22-28): parameter names /
    shapes of vtp_amd.VTPModel against the real class, and the oracle's FFN branch against its encode -> decode"""
    from vtp_amd import VTPConfig, VTPModel
    case = f"ffn{FFN.index((vis, dec))}"
    g = pins[0]
    ours = VTPModel(VTPConfig(**dict(TINY, vision_ffn_layer=vis, decoder_ffn_layer=dec))).state_dict()
    assert {k: tuple(v.shape) for k, v in ours.items()} == _shapes(pins, case)
    sd = _sd(pins, case)
    with torch.no_grad():
        lat = O.reconstruction_latents(sd, g[case + "/img"], 2)
        rec = O.decoder_forward(sd, lat, 2)
    torch.testing.assert_close(*_vs(pins, case + "/lat", lat), rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(*_vs(pins, case + "/rec", rec), rtol=2e-4, atol=2e-5)
