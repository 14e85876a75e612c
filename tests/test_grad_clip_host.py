"""Host-side checks of VTPTrainer's gradient clipping option (no GPU): the validation of max_grad_norm and the C ABI of the clip
kernels (argument checks run before any HIP call)."""
import ctypes
import math

import pytest


@pytest.mark.parametrize("value,want", [(1.0, 1.0), (3, 3.0), (1e-6, 1e-6), (float("inf"), math.inf)])
def test_max_grad_norm_accepts_positive_numbers(value, want):
    from vtp_amd.train import _max_norm_value
    assert _max_norm_value(value) == want


@pytest.mark.parametrize("value", [0, 0.0, -1.0, float("nan"), float("-inf"), "3.0x", None, True, [1.0]])
def test_max_grad_norm_rejects_everything_else(value):
    from vtp_amd.train import _max_norm_value
    with pytest.raises(ValueError):
        _max_norm_value(value)


def test_partials_count_depends_on_the_length_only():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    lib = _lib.load()
    assert [lib.vtp_sumsq_partials_count(n) for n in (0, 4, 8192, 8196, 1 << 24, (1 << 24) + 4)] == [0, 1, 1, 2, 2048, 2049]
    p = ctypes.c_void_p(16)
    assert lib.vtp_sumsq_partials(p, 6, p, None) == -1            # n % 4 != 0
    assert lib.vtp_sumsq_partials(None, 8, p, None) == -1
    assert lib.vtp_sum_partials(p, 0, p, None) == -1              # count >= 1
    assert lib.vtp_grad_clip_finalize(p, 4, None, p, p, None) == -1  # no hyper block
