"""vision_bottleneck_ae_only=False / vision_clip_feat='pooled' (no GPU needed): the legacy VTP builds with the reference's head shapes
(vtp.py:215-261: proj, teacher_proj, dino_head, teacher_dino_head read the 64-d bottleneck latents), a legacy checkpoint round-trips
with strict=True, and the EMA pairs cover the teacher's bottleneck."""
import pytest
import torch


def _cfg(**kw):
    from oracle.ref_stubs import TINY
    from vtp_amd import VTPConfig
    return VTPConfig(**TINY, **kw)


@pytest.mark.parametrize("feat", ["cls", "pooled"])
def test_vtp_builds_with_bottlenecked_heads(feat):
    from vtp_amd import VTP
    torch.manual_seed(0)
    m = VTP(_cfg(vision_bottleneck_ae_only=False, vision_clip_feat=feat), dino_out_dim=256, dino_hidden_dim=96, dino_bottleneck_dim=32)
    Db, Dt = m.config.vision_feature_bottleneck, m.config.text_embed_dim
    assert Db != m.config.vision_embed_dim
    assert tuple(m.trunk.feature_bottleneck.weight.shape) == (Db, m.config.vision_embed_dim)
    assert tuple(m.teacher_trunk.feature_bottleneck.weight.shape) == (Db, m.config.vision_embed_dim)
    assert tuple(m.proj.weight.shape) == (Dt, Db) and tuple(m.teacher_proj.weight.shape) == (Dt, Db)
    assert tuple(m.dino_head.mlp[0].weight.shape) == (96, Db) and tuple(m.teacher_dino_head.mlp[0].weight.shape) == (96, Db)
    assert not m.teacher_trunk.feature_bottleneck.weight.requires_grad
    sd = m.legacy_state_dict()
    assert "proj.weight" in sd and "teacher_proj.weight" in sd and "teacher_trunk.feature_bottleneck.weight" in sd
    m2 = VTP(_cfg(vision_bottleneck_ae_only=False, vision_clip_feat=feat), dino_out_dim=256, dino_hidden_dim=96, dino_bottleneck_dim=32)
    m2.load_state_dict(sd, strict=True)
    assert torch.equal(m2.dino_head.mlp[0].weight, m.dino_head.mlp[0].weight)
    assert ("teacher_trunk.", "trunk.") in m.ema_pairs()


def test_default_heads_unchanged():
    from vtp_amd import VTP
    m = VTP(_cfg(), dino_out_dim=256, dino_hidden_dim=96, dino_bottleneck_dim=32)
    D = m.config.vision_embed_dim
    assert tuple(m.dino_head.mlp[0].weight.shape) == (96, D) and tuple(m.proj.weight.shape) == (m.config.text_embed_dim, D)
