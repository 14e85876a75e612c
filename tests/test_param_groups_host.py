"""Per-parameter-group learning-rate / weight-decay scales of VTPTrainer, the host side: how param_groups resolve to table rows
(first match wins, the implicit default group, the split by no_decay, every ValueError), layerwise_lr_decay against DINOv2's rule on
the tiny golden configuration's parameter names, and the argument checks of the two grouped entry points (no GPU needed)."""
import ctypes
import math

import pytest

SHAPES = {
    "trunk.patch_embed.proj.weight": (8, 3, 16, 16), "trunk.patch_embed.proj.bias": (8,), "trunk.cls_token": (1, 1, 8),
    "trunk.blocks.0.attn.qkv.weight": (24, 8), "trunk.blocks.0.attn.qkv.bias": (24,), "trunk.blocks.1.attn.qkv.weight": (24, 8),
    "trunk.norm.weight": (8,), "pixel_decoder.proj_in.weight": (8, 4, 1, 1), "dino_head.last_layer.weight_g": (16, 1), "logit_scale": (),
}


def _no_decay(name, shape):
    return len(shape) < 2 or name.endswith("cls_token")


def test_first_match_wins_and_the_rest_is_default():
    from vtp_amd.train import group_table, resolve_param_groups
    pg = [{"name": "embed", "match": ("trunk.patch_embed.",), "lr_scale": 0.2},
          {"name": "trunk", "match": ("trunk.",), "lr_scale": 0.5, "wd_scale": 2.0},
          {"name": "wide", "match": lambda name, shape: len(shape) == 4, "lr_scale": 3.0},  # patch_embed went to "embed" already
          {"name": "frozen", "match": "dino_head.last_layer", "lr_scale": 0.0}]
    groups, rows = resolve_param_groups(pg, SHAPES)
    assert [g["name"] for g in groups] == ["embed", "trunk", "wide", "frozen", "default"]
    assert groups[0] == {"name": "embed", "lr_scale": 0.2, "wd_scale": 1.0}
    assert groups[-1] == {"name": "default", "lr_scale": 1.0, "wd_scale": 1.0}
    want = {"trunk.patch_embed.proj.weight": 0, "trunk.patch_embed.proj.bias": 0, "trunk.cls_token": 1, "trunk.blocks.0.attn.qkv.weight": 1,
            "trunk.blocks.0.attn.qkv.bias": 1, "trunk.blocks.1.attn.qkv.weight": 1, "trunk.norm.weight": 1,
            "pixel_decoder.proj_in.weight": 2, "dino_head.last_layer.weight_g": 3, "logit_scale": 4}
    assert rows == {k: 2 * v for k, v in want.items()}  # no_decay=None: every parameter on its group's decayed row
    assert group_table(groups) == [0.2, 1.0, 0.2, 0.0, 0.5, 2.0, 0.5, 0.0, 3.0, 1.0, 3.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0]


def test_no_decay_splits_every_group_into_two_rows():
    from vtp_amd.train import resolve_param_groups
    pg = [{"name": "trunk", "match": ("trunk.",), "wd_scale": 2.0}]
    groups, rows = resolve_param_groups(pg, SHAPES, _no_decay)
    assert [g["name"] for g in groups] == ["trunk", "default"]
    for name, shape in SHAPES.items():
        gi = 0 if name.startswith("trunk.") else 1
        assert rows[name] == 2 * gi + int(_no_decay(name, shape)), name
    assert rows["trunk.cls_token"] == 1 and rows["logit_scale"] == 3 and rows["trunk.blocks.0.attn.qkv.weight"] == 0


def test_everything_matched_means_no_default_group():
    from vtp_amd.train import resolve_param_groups
    groups, rows = resolve_param_groups([{"name": "all", "match": ("",)}], SHAPES)
    assert [g["name"] for g in groups] == ["all"] and set(rows.values()) == {0}


def test_value_errors():
    from vtp_amd.train import group_table, resolve_param_groups
    one = lambda **kw: [dict({"name": "g", "match": ("trunk.",)}, **kw)]  # noqa: E731
    for bad in (-0.5, float("nan"), float("inf"), float("-inf"), "fast", None, True):
        for key in ("lr_scale", "wd_scale"):
            with pytest.raises(ValueError, match=key):
                resolve_param_groups(one(**{key: bad}), SHAPES)
    with pytest.raises(ValueError, match="duplicate"):
        resolve_param_groups(one() + one(), SHAPES)
    with pytest.raises(ValueError, match="duplicate"):
        resolve_param_groups([{"name": "default", "match": ("trunk.",)}], SHAPES)  # collides with the implicit group
    with pytest.raises(ValueError, match="match no parameter"):
        resolve_param_groups(one() + [{"name": "text", "match": ("text_transformer.",)}], SHAPES)
    with pytest.raises(ValueError, match="match no parameter"):
        resolve_param_groups([{"name": "a", "match": ("trunk.",)}, {"name": "b", "match": ("trunk.blocks.",)}], SHAPES)  # shadowed
    many = {f"p{i}": (4,) for i in range(130)}
    per_param = lambda k: [{"name": f"g{i}", "match": (lambda n, s, i=i: n == f"p{i}")} for i in range(k)]  # noqa: E731
    with pytest.raises(ValueError, match="at most 128"):
        resolve_param_groups(per_param(129), many)
    with pytest.raises(ValueError, match="default"):
        resolve_param_groups(per_param(128), many)  # 128 groups + the implicit one
    groups, rows = resolve_param_groups(per_param(128), {k: many[k] for k in list(many)[:128]}, lambda n, s: True)
    assert len(groups) == 128 and max(rows.values()) == 255
    with pytest.raises(ValueError):
        resolve_param_groups([{"name": "g"}], SHAPES)
    with pytest.raises(ValueError):
        resolve_param_groups([{"name": "g", "match": ("trunk.",), "lr": 0.1}], SHAPES)
    # a scale that a scheduler broke later is caught where the table is built
    groups, _ = resolve_param_groups(one(), SHAPES)
    groups[0]["lr_scale"] = -1.0
    with pytest.raises(ValueError, match="lr_scale"):
        group_table(groups)


def test_layerwise_lr_decay_on_the_tiny_golden_names(golden_sd):
    from oracle.ref_stubs import TINY
    from vtp_amd import VTPConfig
    from vtp_amd.train import layerwise_lr_decay, resolve_param_groups
    L = VTPConfig(**TINY).vision_depth
    names = list(golden_sd)
    assert f"trunk.blocks.{L - 1}.attn.qkv.weight" in names and f"trunk.blocks.{L}.attn.qkv.weight" not in names
    decay, mult = 0.75, 0.2
    pg = layerwise_lr_decay(names, L, decay, patch_embed_lr_mult=mult)
    groups, rows = resolve_param_groups(pg, {n: tuple(golden_sd[n].shape) for n in names})
    scale = lambda n: groups[rows[n] // 2]["lr_scale"]  # noqa: E731
    assert scale("trunk.patch_embed.proj.weight") == decay ** (L + 1) * mult
    assert scale("trunk.patch_embed.proj.bias") == decay ** (L + 1) * mult
    assert scale("trunk.cls_token") == decay ** (L + 1) and scale("trunk.mask_token") == decay ** (L + 1)
    assert scale("trunk.blocks.0.attn.qkv.weight") == decay ** L and scale("trunk.blocks.0.norm1.weight") == decay ** L
    assert scale(f"trunk.blocks.{L - 1}.mlp.w3.weight") == decay ** 1
    assert scale("trunk.norm.weight") == 1.0 and scale("trunk.feature_bottleneck.weight") == 1.0
    for n in names:
        if n.startswith("trunk.blocks."):
            assert scale(n) == decay ** (L - int(n.split(".")[2])), n
        if not n.startswith("trunk."):  # non-trunk names are untouched: the default group
            assert groups[rows[n] // 2]["name"] == "default" and scale(n) == 1.0, n
    assert all(g["wd_scale"] == 1.0 for g in groups)
    assert len(pg) <= L + 3 and len({g["lr_scale"] for g in pg}) == len(pg)  # equal scales share a group
    assert all(g["name"].startswith("trunk.") for g in pg)
    # another prefix; decay 1 folds every layer into one group (and the patch embedding into its own)
    dec = layerwise_lr_decay(names, 2, 0.5, prefix="pixel_decoder.")
    g2, r2 = resolve_param_groups(dec, {n: tuple(golden_sd[n].shape) for n in names})
    assert g2[r2["pixel_decoder.blocks.1.attn.qkv.weight"] // 2]["lr_scale"] == 0.5
    assert g2[r2["trunk.norm.weight"] // 2]["name"] == "default"
    flat = layerwise_lr_decay(names, L, 1.0, patch_embed_lr_mult=0.1)
    assert sorted(g["lr_scale"] for g in flat) == [0.1, 1.0]
    # a depth-12 trunk: 14 layer ids and the patch embedding -> 15 groups
    big = ["trunk.patch_embed.proj.weight", "trunk.cls_token", "trunk.norm.weight"] + [f"trunk.blocks.{i}.w" for i in range(12)]
    pg12 = layerwise_lr_decay(big, 12, 0.9, patch_embed_lr_mult=0.5)
    assert len(pg12) == 15
    assert math.isclose(min(g["lr_scale"] for g in pg12), 0.9 ** 13 * 0.5)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("entry", ["vtp_adamw_dev_grouped", "vtp_adamw_ema_dev_grouped"])
def test_grouped_entry_points_validate_without_a_gpu(lib, entry):
    from vtp_amd import _lib
    fn = getattr(lib, entry)
    P = ctypes.c_void_p(16)
    head = (P, P, P, P, None)  # p, g, m, v, p_bf16 | teacher; every call below is rejected before any HIP call is made
    bad = [
        ((None, P, P, P, None), P, P, 2, 8, P),    # NULL parameter buffer, as the siblings
        (head, P, P, 2, 6, P),                     # n % 4 != 0
        (head, P, P, 2, 0, P),                     # n == 0
        (head, P, P, 2, 8, None),                  # NULL hyper
        (head, None, P, 2, 8, P),                  # NULL group4
        (head, P, None, 2, 8, P),                  # NULL group_tab
        (head, P, P, 0, 8, P),                     # ngroups outside 1..256
        (head, P, P, 257, 8, P),
        (head, P, P, -1, 8, P),
    ]
    for h, g4, tab, ng, n, hyper in bad:
        rc = fn(*h, g4, tab, ng, n, hyper, None)
        assert rc == -1, (entry, g4, tab, ng, n)
        assert entry.encode() in lib.vtp_last_error()
    with pytest.raises(RuntimeError, match=entry):
        _lib.check(fn(*head, P, P, 300, 8, P, None), entry)
    assert lib.vtp_abi_version() == 1
