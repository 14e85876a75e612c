"""bottleneck_ae_only=False pinned to the REAL reference: tests/golden/vtp_tiny_bottleneck_heads.safetensors holds the legacy VTP's
teacher / student SSL dicts and encode_image (cls, pooled) recorded by tools/record_bottleneck_heads.py.  The oracle composition
that the GPU tests compare against -- trunk_forward(use_bottleneck=True) of the teacher and the student, dino_head_forward on the
64-d latents, the CLIP feature through the bottleneck -- matches it here; where the reference itself is importable, it is re-run on
the regenerated weights and must reproduce the fixture."""
import importlib.util
import os

import pytest
import torch

from oracle import vtp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_bottleneck_heads", os.path.join(ROOT, "tools", "record_bottleneck_heads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fx():
    return _tool().load()


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def ssl_outputs_bottleneck(sd, gc, lc, masks, heads):
    """VTP.get_teacher_forward_outputs + get_student_ssl_outputs (vtp.py:410-484) with use_bottleneck=True: the teacher's and the
    student's own feature_bottleneck on the cls and patch tokens, the DINO heads on the 64-d latents"""
    idx = masks.flatten().nonzero().flatten()
    with torch.no_grad():
        t = O.trunk_forward(sd, gc, heads, use_bottleneck=True, pre="teacher_trunk.")
        cls = t["x_norm_clstoken"].chunk(2)
        cls = torch.cat((cls[1], cls[0]))
        th = O.dino_head_forward(sd, "teacher_dino_head.", torch.cat([cls, t["x_norm_patchtokens"].flatten(0, 1)[idx]]))
    n = cls.shape[0]
    sg = O.trunk_forward(sd, gc, heads, use_bottleneck=True, masks=masks)
    sl = O.trunk_forward(sd, lc, heads, use_bottleneck=True)
    teacher = {"teacher_cls_tokens_after_head": th[:n], "masked_teacher_patch_tokens_after_head": th[n:]}
    student = {"student_local_cls_tokens_after_head": O.dino_head_forward(sd, "dino_head.", sl["x_norm_clstoken"]),
               "student_global_cls_tokens_after_head": O.dino_head_forward(sd, "dino_head.", sg["x_norm_clstoken"]),
               "student_global_cls_tokens": sg["x_norm_clstoken"],
               "student_global_masked_patch_tokens_after_head":
                   O.dino_head_forward(sd, "dino_head.", sg["x_norm_patchtokens"].flatten(0, 1)[idx])}
    return teacher, student


def test_oracle_composition_matches_reference_fixture(fx):
    g, meta, sd = fx
    heads = meta["cfg"]["heads"]
    masks = g["in.masks"].bool()
    with torch.no_grad():
        t, s = ssl_outputs_bottleneck(sd, g["in.global_crops"], g["in.local_crops"], masks, heads)
    assert s["student_global_cls_tokens"].shape[-1] == meta["cfg"]["bott"] == 64
    for pre, d in (("teacher.", t), ("student.", s)):
        for k, v in d.items():
            ref = g[pre + k]
            assert v.shape == ref.shape, k
            print(f"{k}: rel {rel(v, ref):.2e}")
            assert rel(v, ref) < 1e-5, k
    sdv = dict(sd, **{"visual_proj.weight": sd["proj.weight"]})  # (legacy `proj` = the HF class's visual_proj)
    for feat in ("cls", "pooled"):
        with torch.no_grad():
            f = O.clip_image_feature(sdv, g["in.image"], heads, normalize=False, clip_feat=feat, ae_only=False)
        print(f"encode_image {feat}: rel {rel(f, g['enc.' + feat]):.2e}")
        assert rel(f, g["enc." + feat]) < 1e-5, feat
    assert rel(g["enc.cls"], g["enc.pooled"]) > 0.1  # the two features differ


def test_live_reference_reproduces_fixture(fx):
    from oracle.ref_stubs import reference_available
    if not reference_available():
        pytest.skip("reference tree not available")
    from oracle.ref_stubs import load_reference
    tool = _tool()
    g, meta, sd = fx
    model, cfg = tool.reference_model(load_reference(), meta["cfg"])
    assert [[k, list(v.shape)] for k, v in model.named_parameters()] == meta["params"]
    batch, image = tool.ssl_batch(meta["cfg"])
    assert torch.equal(batch["global_crops"], g["in.global_crops"]) and torch.equal(image, g["in.image"])
    out = tool.run_reference(model, cfg, sd, batch, image)
    for k, v in out.items():
        assert rel(v, g[k]) < 1e-6, k
