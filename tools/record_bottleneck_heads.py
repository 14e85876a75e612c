"""Records tests/golden/vtp_tiny_bottleneck_heads.safetensors from the REAL reference's legacy training class (vtp/models/vtp.py `VTP`)
configured with vision_encoder.bottleneck_ae_only=False: CLIP, DINO and iBOT read the 64-d bottleneck latents (vtp.py:215-261,
275-293,418-423,457-463).  Needs the reference tree (oracle/ref_stubs.py finds it); run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/record_bottleneck_heads.py

The fixture stays small: the weights are not stored but regenerated from seeds (seeded_state below: one generator per parameter, in
the recorded key order), and only the buffers (RoPE periods) are kept.  Stored: the seeded ssl_dict (2 global 64x64 crops, 2 local
32x32 crops per image, iBOT masks), an image batch, the reference's teacher / student SSL output dicts (student_global_cls_tokens
included) and encode_image (un-normalised) for clip_feat 'cls' and 'pooled'."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vtp_tiny_bottleneck_heads.safetensors")
CFG = dict(embed_dim=128, depth=2, heads=2, K=256, hidden=128, bott=64, R=64, r=32, B=2, n_local=2, text_layers=1, text_heads=2,
           vocab=64, ctx=8, dec_depth=1, dec_heads=2)
_NORMS = ("norm.weight", "norm1.weight", "norm2.weight", "ln_1.weight", "ln_2.weight", "ln_final.weight", "last_layer.weight_g")


def seeded_state(keys):
    """keys: [(name, shape)] in the recorded order -> {name: f32 tensor}; parameter i is drawn from Generator().manual_seed(1000 + i)"""
    sd = {}
    for i, (name, shape) in enumerate(keys):
        x = torch.randn(tuple(shape), generator=torch.Generator().manual_seed(1000 + i))
        if name == "logit_scale":
            sd[name] = torch.full(tuple(shape), math.log(1 / 0.07))
        elif name.endswith(_NORMS):
            sd[name] = 1 + 0.1 * x
        else:
            sd[name] = 0.02 * x
    return sd


def load(path=OUT):
    """(tensors, meta, state_dict) of the fixture; the state_dict is rebuilt from the seeds plus the stored buffers"""
    from safetensors import safe_open
    from safetensors.torch import load_file
    g = load_file(path)
    with safe_open(path, "pt") as f:
        meta = json.loads(f.metadata()["meta"])
    sd = seeded_state(meta["params"])
    sd.update({k[4:]: v for k, v in g.items() if k.startswith("buf.")})
    return g, meta, sd


def reference_model(ns, c, seed_keys=None):
    """the reference's legacy VTP at this fixture's configuration (bottleneck_ae_only=False, train_clip + train_dinov2)"""
    from oracle.make_golden_legacy import legacy_config
    cfg = legacy_config(ns, c)
    cfg.training.train_reconstruction = False
    cfg.vtp_model.vision_encoder.bottleneck_ae_only = False
    torch.manual_seed(0)
    return ns.VTP(vtp_config=cfg), cfg


def ssl_batch(c, seed=7):
    g = torch.Generator().manual_seed(seed)
    B, hw = c["B"], (c["R"] // 16) ** 2
    global_crops = torch.randn(2 * B, 3, c["R"], c["R"], generator=g)
    local_crops = torch.randn(c["n_local"] * B, 3, c["r"], c["r"], generator=g)
    masks = torch.rand(2 * B, hw, generator=g) < 0.35
    masks[1] = False  # an un-masked image
    idx = masks.flatten().nonzero().flatten()
    image = torch.randn(B, 3, c["R"], c["R"], generator=g)
    return dict(global_crops=global_crops, n_global_crops=2, mask_indices_list=idx, n_masked_patches=int(idx.numel()),
                upperbound=int(idx.numel()) + 5, local_crops=local_crops, masks=masks), image


def run_reference(model, cfg, sd, batch, image):
    """the reference's outputs with the weights `sd` loaded: {fixture key: tensor}"""
    model.load_state_dict(sd, strict=True)
    model.train()  # forward_ssl_learning and encode_image are training-time paths (drop rates 0)
    out = {}
    with torch.no_grad():
        t_out, s_out = model(forward_type="ssl", ssl_dict=batch)
        for k, v in t_out.items():
            if torch.is_tensor(v):
                out["teacher." + k] = v.detach().float().contiguous()
        for k, v in s_out.items():
            out["student." + k] = v.detach().float().contiguous()
        for feat in ("cls", "pooled"):
            cfg.vtp_model.vision_encoder.clip_feat = feat
            out["enc." + feat] = model.encode_image(image).detach().float().contiguous()
    return out


def main():
    from safetensors.torch import save_file
    from oracle.ref_stubs import load_reference
    ns = load_reference()
    c = CFG
    model, cfg = reference_model(ns, c)
    pnames = {n for n, _ in model.named_parameters()}
    keys = [(k, list(v.shape)) for k, v in model.state_dict().items() if k in pnames]
    bufs = {k: v.detach().clone().contiguous() for k, v in model.state_dict().items() if k not in pnames}
    sd = seeded_state(keys)
    sd.update(bufs)
    batch, image = ssl_batch(c)
    out = run_reference(model, cfg, sd, batch, image)
    out.update({"in.global_crops": batch["global_crops"], "in.local_crops": batch["local_crops"],
                "in.masks": batch["masks"].to(torch.uint8), "in.image": image})
    out.update({"buf." + k: v for k, v in bufs.items()})
    meta = {"params": keys, "cfg": c}
    save_file(out, OUT, metadata={"meta": json.dumps(meta)})
    print("wrote", OUT, os.path.getsize(OUT) / 1e6, "MB;", {k: tuple(v.shape) for k, v in out.items() if not k.startswith("in.")})


if __name__ == "__main__":
    main()
