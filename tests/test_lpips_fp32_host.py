"""Host-side checks of LPIPS.enable_fp32_forward (vtp_amd/lpips.py): the switch, its errors and the cached fp32 operands.  No GPU."""
import pytest
import torch


def _module(seed=0):
    from oracle import lpips_oracle as L
    from vtp_amd import LPIPS
    m = LPIPS(use_dropout=True)
    sd = L.make_state(seed)
    m.load_state_dict(sd, strict=True)
    return m, sd


def test_the_switch_exists_defaults_to_off_and_returns_the_module():
    from vtp_amd import LPIPS
    m = LPIPS()
    assert m.fp32_forward is False
    assert m.enable_fp32_forward() is m and m.fp32_forward is True
    assert m.disable_fp32_forward() is m and m.fp32_forward is False


def test_chunk_argument():
    from vtp_amd import LPIPS
    from vtp_amd.lpips import FP32_CHUNK
    assert LPIPS().fp32_chunk == FP32_CHUNK
    assert LPIPS(fp32_chunk=3).fp32_chunk == 3
    m = LPIPS().enable_fp32_forward(chunk=2)
    assert m.fp32_chunk == 2 and m.enable_fp32_forward().fp32_chunk == 2
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="fp32_chunk"):
            LPIPS().enable_fp32_forward(chunk=bad)
    with pytest.raises(ValueError, match="fp32_chunk"):
        LPIPS(fp32_chunk=0)


def test_workspace_bytes_are_bounded_by_the_chunk():
    from vtp_amd import LPIPS
    from vtp_amd.lpips import FP32_CHUNK
    one = LPIPS.fp32_workspace_bytes(1, 256, 256)
    assert one == 4 * 2 * 256 * 256 * (128 + 4) + 8 * (256 + 64 + 16 + 4 + 1)
    assert LPIPS.fp32_workspace_bytes(FP32_CHUNK, 256, 256) == FP32_CHUNK * one < 2 ** 30


def test_a_cpu_module_raises_on_forward():
    m, _ = _module()
    m.enable_fp32_forward()
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, x)
    m.disable_fp32_forward()
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # as before
        m(x, x)


@pytest.mark.parametrize("shape", [(1, 3, 24, 16), (1, 3, 16, 40), (1, 3, 8, 8), (1, 1, 16, 16)])
def test_a_wrongly_sized_input_raises_before_anything_runs(shape):
    m, _ = _module()
    m.enable_fp32_forward()
    x = torch.zeros(*shape)
    with pytest.raises(ValueError):
        m(x, x)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 16, 16), torch.zeros(2, 3, 16, 16))


def test_cached_operands_are_the_permuted_fp32_weights():
    from vtp_amd.lpips import FP32_CIN0, VGG_CONVS
    m, sd = _module(3)
    op = m._fp32_operands()
    for i, (sl, idx, cin, cout) in enumerate(VGG_CONVS):
        w = sd[f"net.slice{sl}.{idx}.weight"]
        got = op["w"][i]
        assert got.dtype == torch.float32 and got.is_contiguous()
        if i == 0:
            assert got.shape == (cout, 3, 3, FP32_CIN0)
            assert torch.equal(got[..., :3], w.permute(0, 2, 3, 1))
            assert FP32_CIN0 == 3 or bool((got[..., 3:] == 0).all())
        else:
            assert got.shape == (cout, 3, 3, cin) and torch.equal(got, w.permute(0, 2, 3, 1))
        assert torch.equal(op["b"][i], sd[f"net.slice{sl}.{idx}.bias"])
    for k in range(5):
        assert torch.equal(op["lin"][k], sd[f"lin{k}.model.1.weight"].flatten())
    assert op["shift"] == sd["scaling_layer.shift"].flatten().tolist()  # the fp32 buffer values, widened exactly
    assert op["scale"] == sd["scaling_layer.scale"].flatten().tolist()


def test_state_dict_keys_do_not_move_with_the_switch():
    from vtp_amd import LPIPS
    m, sd = _module()
    keys = list(m.state_dict().keys())
    assert set(keys) == set(sd.keys())
    m.enable_fp32_forward()
    assert list(m.state_dict().keys()) == keys
    nd = LPIPS(use_dropout=False).enable_fp32_forward()
    assert "lin0.model.0.weight" in nd.state_dict() and len(nd._fp32_operands()["lin"]) == 5
