"""Training-step parity at the WIDTHS of the reference's wide presets, one per tower: trunk 1152 / 18 heads / FFN ratio 3.7778 (vit_so400m:
SwiGLU hidden 2904), pixel decoder 1280 / 20 heads (vit_huge2: hidden 3416), text tower 1536 / 24 heads (vit_giant2).  Every row norm is
therefore the 8-chunk instantiation (trunk RMSNorm at 1152, decoder LayerNorm at 1280, text LayerNorm at 1536), RoPE runs over 18 and 20
heads, every GEMM has N or K tails (1152, 3456, 5808, 2904), and the trunk's last block cannot take the tail-row plan (D > 1024).  256 x 256,
depth 2 in all three towers, B = 2 images with 2 global 256^2 + 8 local 96^2 crops each: M = 4 * 257 + 16 * 37 = 1620 token rows in the
list forward; K = 8192 prototypes keep the CPU oracle at seconds.

Protocol = tests/test_parity_ssl_gpu.py, exactly as tests/test_parity_large_gpu.py applies it: E_ours <= 1.25 x E_ref against the oracle
in fp32, E_ref = the reference algorithm under bf16 autocast on the CPU and on this GPU; the same loss bars.

Also here: the fused step's one refusal above 1024 -- vision_clip_feat='pooled' (its final-norm backward takes the pooled gradient and
has no 8-chunk variant) -- is raised before any work is issued, and leaves the trainer usable."""
import pytest
import torch

from test_parity_ssl_gpu import DEV, HEAD_KEYS, LOSS_REL_FLOOR, Case, _compare_grads, _trainer, check

pytestmark = pytest.mark.gpu

W2 = dict(image_size=256,
          vision_embed_dim=1152, vision_depth=2, vision_num_heads=18, vision_mlp_ratio=3.777777778,
          decoder_embed_dim=1280, decoder_depth=2, decoder_num_heads=20,
          text_embed_dim=1536, text_depth=2, text_num_heads=24)
TRUNK_KEYS = [f"trunk.blocks.{i}.{n}" for i in (0, 1)
              for n in ("attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "mlp.w1.weight", "mlp.w2.bias", "mlp.w3.weight",
                        "norm1.weight", "norm2.weight")] + \
             ["trunk.patch_embed.proj.weight", "trunk.patch_embed.proj.bias", "trunk.cls_token", "trunk.mask_token", "trunk.norm.weight"]
_CASE = []


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def case() -> Case:
    if not _CASE:
        _CASE.append(Case(cfg_kw=W2, heads=(18, 20, 24), K=8192, res=256, seed=43))
    return _CASE[0]


def test_wide_ssl_head_outputs():
    """teacher / student dicts from a 1152-wide trunk, N = 257 + N = 37"""
    c = case()
    col = c.col
    cfg = c.model.config
    assert (cfg.vision_embed_dim, cfg.decoder_embed_dim, cfg.text_embed_dim) == (1152, 1280, 1536)
    assert c.sd["trunk.blocks.0.mlp.w1.weight"].shape == (2904, 1152) and c.sd["pixel_decoder.blocks.0.mlp.w1.weight"].shape == (3416, 1280)
    with torch.no_grad():
        c.model.eval()
        t_out, s_out = c.model.forward_ssl_learning(c.gc.to(DEV), 2, col["mask_indices_list"].to(DEV), int(col["n_masked_patches"]),
                                                    col["upperbound"], c.lc.to(DEV), c.masks.to(DEV))
        c.model.train()
    ref_t, ref_s = c.out["f32"]
    for k in ("teacher_cls_tokens_after_head", "masked_teacher_patch_tokens_after_head"):
        check(f"W2 teacher {k}", t_out[k], ref_t[k], c.out["cpu16"][0][k], c.out["gpu16"][0][k])
    for k in ("student_local_cls_tokens_after_head", "student_global_cls_tokens_after_head", "student_global_cls_tokens",
              "student_global_masked_patch_tokens_after_head"):
        check(f"W2 student {k}", s_out[k], ref_s[k], c.out["cpu16"][1][k], c.out["gpu16"][1][k])


def test_wide_ssl_only_gradients():
    """DINO + iBOT alone through the 1152-wide trunk: 8-chunk RMSNorm backward, H = 2904 SwiGLU backward and weight gradients"""
    c = case()
    tr, ssl = _trainer(c, rec_weight=0.0)
    tr.step(c.img.to(DEV), None, ssl)
    torch.cuda.synchronize()
    loss = float(tr.ssl_loss_sum)
    e, e_ref = abs(loss - c.loss["f32"]), max(abs(c.loss["cpu16"] - c.loss["f32"]), abs(c.loss["gpu16"] - c.loss["f32"]))
    print(f"PARITY W2 SSL loss: ours={loss:.6f} oracle fp32={c.loss['f32']:.6f} |err| ours={e:.2e} ref={e_ref:.2e}")
    assert e <= max(1.25 * e_ref, LOSS_REL_FLOOR * abs(c.loss["f32"]))
    _compare_grads("W2 SSL-only", dict(c.model.named_parameters()), HEAD_KEYS + TRUNK_KEYS, c.grads_ssl)


def test_wide_full_step_gradients():
    """rec + clip + ssl: one list forward, one trunk backward, the decoder at 1280 / N = 256, the text tower at 1536; the trunk's last
    block runs on all rows (no tail-row plan above 1024) and the step still matches"""
    c = case()
    tr, ssl = _trainer(c)
    assert tr.trunk.tail_rows_ok(True) is False and tr.trunk.tail_rows_ok(False) is False, "the tail-row plan stops at D = 1024"
    l1, lc = tr.step(c.img.to(DEV), c.txt.to(DEV), ssl)
    torch.cuda.synchronize()
    print(f"PARITY W2 full step losses: ours L1={float(l1):.6f} clip={float(lc):.6f} ssl={float(tr.ssl_loss_sum):.6f} | oracle fp32 "
          f"L1={c.loss_full[0]:.6f} clip={c.loss_full[1]:.6f} ssl={c.loss_full[2]:.6f}")
    assert abs(float(l1) - c.loss_full[0]) < 2e-3 * c.loss_full[0]
    assert abs(float(lc) - c.loss_full[1]) < 5e-3 * max(c.loss_full[1], 1e-3)
    assert abs(float(tr.ssl_loss_sum) - c.loss_full[2]) < 1e-3 * c.loss_full[2]
    dec = [f"pixel_decoder.blocks.{i}.{n}" for i in (0, 1) for n in ("attn.qkv.weight", "attn.proj.weight", "mlp.w3.weight", "norm2.weight")]
    txt = [f"text_transformer.resblocks.{i}.{n}" for i in (0, 1) for n in ("attn.in_proj_weight", "mlp.c_fc.weight")]
    _compare_grads("W2 FULL step", dict(c.model.named_parameters()),
                   HEAD_KEYS + TRUNK_KEYS + dec + txt + ["pixel_decoder.proj_out.weight", "trunk.feature_bottleneck.weight",
                                                        "visual_proj.weight", "logit_scale"], c.grads_full)


def test_pooled_clip_is_refused_above_1024_before_any_work():
    """vision_clip_feat='pooled' at vision_embed_dim = 1152: step(images, text, ssl) raises NotImplementedError naming vision_embed_dim
    with every parameter and gradient bit-identical to before; step(images, None, ssl) on the same trainer then runs"""
    from vtp_amd import VTP, VTPConfig, VTPTrainer
    c = case()  # (its inputs only)
    torch.manual_seed(44)
    m = VTP(VTPConfig(**{**W2, "vision_depth": 1, "decoder_depth": 1, "text_depth": 1, "vision_clip_feat": "pooled"}), dino_out_dim=8192).to(DEV)
    tr = VTPTrainer(m, lr=1e-4)
    ssl = tr.prepare_ssl(c.gc.to(DEV), c.lc.to(DEV), c.masks, upperbound=c.col["upperbound"])
    torch.cuda.synchronize()
    before = {n: (p.detach().clone(), None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
    with pytest.raises(NotImplementedError, match="vision_embed_dim"):
        tr.step(c.img.to(DEV), c.txt.to(DEV), ssl)
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        p0, g0 = before[n]
        assert torch.equal(p.detach(), p0), f"{n} changed by a refused step"
        assert (p.grad is None) == (g0 is None) and (g0 is None or torch.equal(p.grad, g0)), f"{n}.grad changed by a refused step"
    l1, lc = tr.step(c.img.to(DEV), None, ssl)
    torch.cuda.synchronize()
    assert torch.isfinite(l1).all() and torch.isfinite(tr.ssl_loss_sum).all()
    assert lc is None or torch.isfinite(torch.as_tensor(lc)).all()
    assert all(torch.isfinite(p).all() for p in m.parameters())
