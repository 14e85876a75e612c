"""Host-side checks of VTPTrainer's skip_nonfinite option (no GPU): the validation of the switch and the C ABI of the guarded
entry points (argument checks run before any HIP call)."""
import ctypes

import pytest


@pytest.mark.parametrize("max_grad_norm", [1.0, 3, float("inf")])
def test_skip_nonfinite_needs_a_max_grad_norm(max_grad_norm):
    from vtp_amd.train import _skip_nonfinite_value
    assert _skip_nonfinite_value(True, max_grad_norm) is True
    assert _skip_nonfinite_value(False, max_grad_norm) is False
    assert _skip_nonfinite_value(False, None) is False
    with pytest.raises(ValueError, match="max_grad_norm"):
        _skip_nonfinite_value(True, None)


@pytest.mark.parametrize("value", [0, 1, 1.0, "yes", None, [True]])
def test_skip_nonfinite_rejects_non_bools(value):
    from vtp_amd.train import _skip_nonfinite_value
    with pytest.raises(ValueError, match="skip_nonfinite"):
        _skip_nonfinite_value(value, 1.0)


def test_constructor_takes_the_switch_and_checks_it_first():
    import inspect
    from vtp_amd import VTPTrainer
    par = inspect.signature(VTPTrainer.__init__).parameters["skip_nonfinite"]
    assert par.default is False
    with pytest.raises(ValueError, match="max_grad_norm"):  # raised before the model is touched
        VTPTrainer(None, skip_nonfinite=True)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        VTPTrainer(None, max_grad_norm=1.0, skip_nonfinite=1)


GUARDED = ("vtp_grad_clip_finalize_guarded", "vtp_adamw_dev_guarded", "vtp_adamw_ema_dev_guarded", "vtp_ema_dev_guarded")


def test_abi_lists_the_guarded_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    lib = _lib.load()
    for name in GUARDED:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    p = ctypes.c_void_p(16)
    betas = (ctypes.c_double * 2)(0.9, 0.95)
    assert lib.vtp_grad_clip_finalize_guarded(p, 2, p, p, p, None, betas, None) == -1  # no state block
    assert lib.vtp_grad_clip_finalize_guarded(p, 2, p, p, p, p, None, None) == -1      # no betas
    assert lib.vtp_grad_clip_finalize_guarded(p, 0, p, p, p, p, betas, None) == -1     # count >= 1
    assert lib.vtp_grad_clip_finalize_guarded(p, 2, p, p, p, p, (ctypes.c_double * 2)(0.9, 1.0), None) == -1
    assert b"betas" in lib.vtp_last_error()
    assert lib.vtp_adamw_dev_guarded(p, p, p, p, None, None, None, 0, 8, p, None, None) == -1      # the skip word is mandatory
    assert lib.vtp_adamw_dev_guarded(p, p, p, p, None, None, None, 0, 6, p, p, None) == -1         # n % 4 != 0
    assert lib.vtp_adamw_dev_guarded(p, p, p, p, None, None, p, 3, 8, p, p, None) == -1            # a table without group4
    assert lib.vtp_adamw_ema_dev_guarded(p, p, p, p, None, p, p, 257, 8, p, p, None) == -1         # ngroups <= 256
    assert lib.vtp_adamw_ema_dev_guarded(p, p, p, p, None, None, None, 0, 8, p, None, None) == -1
    assert lib.vtp_ema_dev_guarded(p, p, 8, p, None, None) == -1
