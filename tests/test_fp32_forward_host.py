"""Host-side pieces of the fp32 inference forward: the tower selection and the heads-follow-towers rule as pure functions, and the ABI
triple (include/vtp_hip.h, vtp_amd/_lib.SIGNATURES, the exports of the cross-compiled library) for the new entry points."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vtp_gemm_nt_f32", "vtp_attn_fwd_f32", "vtp_norm_fwd_f32", "vtp_rope_qk_f32", "vtp_im2col16_rows_f32", "vtp_pixel_shuffle16_f32",
       "vtp_pool_patch_rows_f32")


def test_tower_selection():
    from vtp_amd.model import FP32_TOWERS, fp32_towers
    assert FP32_TOWERS == ("trunk", "decoder", "text")
    assert fp32_towers(("text", "trunk")) == ("trunk", "text")  # canonical order, whatever the caller's
    assert fp32_towers(["decoder"]) == ("decoder",) and fp32_towers("decoder") == ("decoder",)
    assert fp32_towers(("trunk", "trunk", "decoder", "text")) == FP32_TOWERS
    assert fp32_towers(("trunk",), has_decoder=False, has_text=False) == ("trunk",)
    with pytest.raises(ValueError, match="unknown tower"):
        fp32_towers(("trunk", "head"))
    with pytest.raises(ValueError, match="at least one"):
        fp32_towers(())
    with pytest.raises(ValueError, match="pixel decoder"):
        fp32_towers(("decoder",), has_decoder=False)
    with pytest.raises(ValueError, match="text tower"):
        fp32_towers(("text",), has_text=False)


def test_heads_follow_their_tower():
    from vtp_amd.model import FP32_HEAD_TOWER, fp32_head
    assert FP32_HEAD_TOWER["feature_bottleneck"] == FP32_HEAD_TOWER["visual_proj"] == FP32_HEAD_TOWER["pooled_patch_mean"] == "trunk"
    assert FP32_HEAD_TOWER["text_projection"] == FP32_HEAD_TOWER["text_pool"] == "text"
    assert "decoder" not in FP32_HEAD_TOWER.values()
    for head, tower in FP32_HEAD_TOWER.items():
        assert fp32_head(head, (tower,)) and not fp32_head(head, ()) and not fp32_head(head, ("decoder",))
    assert fp32_head("logits", ("trunk", "text")) and fp32_head("logits", ("trunk", "decoder", "text"))
    assert not fp32_head("logits", ("trunk",)) and not fp32_head("logits", ("text", "decoder"))


def test_default_is_bf16_and_the_switch_needs_no_device():
    from oracle.ref_stubs import TINY
    from vtp_amd import VTPConfig, VTPModel
    m = VTPModel(VTPConfig(**TINY))
    assert m.fp32_forward == ()
    with pytest.raises(ValueError, match="unknown tower"):  # validated before the engine (and the device) is touched
        m.enable_fp32_forward(("encoder",))
    assert m.disable_fp32_forward() is m and m.fp32_forward == ()


def test_abi_triple_holds_the_new_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vtp_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), f"{name} is not declared in include/vtp_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"libvtp_hip.so does not export {name}"
    assert lib.vtp_abi_version() == 1
    # argument validation runs before any HIP call: safe without a GPU
    assert lib.vtp_gemm_nt_f32(None, 8, None, 8, None, None, 8, None, None, None, None, 0, 1, 8, 8, 0, None) == -1
    assert b"null" in lib.vtp_last_error()
    import ctypes
    p = ctypes.c_void_p(16)
    assert lib.vtp_gemm_nt_f32(p, 12, p, 12, None, p, 8, None, None, None, None, 0, 4, 8, 12, 0, None) == -1
    assert b"multiples of 8" in lib.vtp_last_error()
    assert lib.vtp_gemm_nt_f32(p, 8, p, 8, None, p, 8, None, None, None, None, 0, 4, 8, 8, 2, None) == -1 and b"W2" in lib.vtp_last_error()
    assert lib.vtp_attn_fwd_f32(p, p, p, p, 1, 0, 1, 0, 192, 0, 64, 0.125, 0, None) == -1 and b"bad shape" in lib.vtp_last_error()


def test_torch_ops_are_registered():
    import vtp_amd.torch_ops as t
    assert {"gemm_nt_f32", "attn_fwd_f32"} <= set(t.OPS)
