"""CPU-side checks of the Inception Score (vtp_amd/inception_score.py, csrc/inception_score.hip) and of GenEval's result keys: the
restatement of tests/is_ref.py on cases with a known answer, the host finalisation against it, the zero-row padding of the
classifier, and that the entry points and wrappers refuse bad arguments before any launch."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import is_ref as IR
from vtp_amd.inception_score import InceptionScore, inception_score_from_sums, pad_fc


def _logits(n=37, C=11, seed=0, scale=3.0):
    return (scale * torch.randn(n, C, generator=torch.Generator().manual_seed(seed))).float()


def test_uniform_logits_score_one():
    for value in (0.0, -3.5, 3e4):
        l = torch.full((12, 9), value)
        for split in (None, 5, 12):
            assert abs(IR.inception_score(l.double(), split)[0] - 1.0) <= 1e-12
            mean, std = inception_score_from_sums(*IR.sums(l.numpy(), split))
            assert abs(mean - 1.0) <= 1e-12 and std <= 1e-12


@pytest.mark.parametrize("C", [2, 10, 1000])
def test_rows_certain_of_different_classes_score_the_class_count(C):
    l = torch.zeros(C, C)
    l[torch.arange(C), torch.arange(C)] = 60.0  # margin 60: the other classes share e^-60 of the mass
    assert abs(IR.inception_score(l.double())[0] - C) <= 1e-9 * C
    mean, std = inception_score_from_sums(*IR.sums(l.numpy()))
    assert abs(mean - C) <= 1e-9 * C and std == 0.0


@pytest.mark.parametrize("split", [None, 1, 7, 36, 37, 50])
def test_from_sums_against_the_direct_formula_with_partial_splits(split):
    l = _logits()
    want_mean, want_std, scores = IR.inception_score(l.double(), split)
    n, H, S = IR.sums(l.numpy(), split)
    assert len(n) == len(scores) == (1 if split is None else -(-37 // split)) and n.sum() == 37
    if split == 7:
        assert n[-1] == 2  # the last split is partial
    mean, std = inception_score_from_sums(n, H, S)
    assert (want_mean > 1.5) == (split != 1)  # not the trivial case -- except for splits of one row, which score exactly 1
    assert abs(mean - want_mean) <= 1e-12 * want_mean
    assert abs(std - want_std) <= 1e-12 * want_mean
    # empty slots (a state that has grown past the rows) are left out
    pad = lambda a: np.concatenate([a, np.zeros((3,) + a.shape[1:])])
    assert inception_score_from_sums(pad(n), pad(H), pad(S)) == (mean, std)


def test_a_class_without_any_mass_gives_a_finite_score():
    l = _logits(20, 6, seed=3)
    l[:, 4] = -1e4  # exp(-1e4) is 0 in fp64: the column sum is exactly 0
    p, h, _ = IR.rows(l.numpy())
    n, H, S = IR.sums(l.numpy(), 8)
    assert (S[:, 4] == 0).all() and np.isfinite(H).all()
    mean, std = inception_score_from_sums(n, H, S)
    want = IR.inception_score(l.double(), 8)[0]
    assert np.isfinite(mean) and np.isfinite(std) and abs(mean - want) <= 1e-12 * want


def test_from_sums_arguments():
    with pytest.raises(ValueError):
        inception_score_from_sums([3.0, 2.0], [0.0], np.ones((2, 4)))
    with pytest.raises(RuntimeError, match="no rows"):
        inception_score_from_sums([0.0], [0.0], np.zeros((1, 4)))
    mean, std = inception_score_from_sums(3.0, -3 * np.log(4.0), np.full(4, 0.75))  # scalars and one row: one split
    assert abs(mean - 1.0) <= 1e-12 and std == 0.0


def test_rows_reference_keeps_the_entropy_of_a_certain_row():
    """one logit 80 above the rest: log Z = log1p(7 e^-80); log(1 + 7 e^-80) would be 0 and h would lose its largest term"""
    l = np.zeros((1, 8), dtype=np.float32)
    l[0, 3] = 80.0
    p, h, mag = IR.rows(l)
    eps = 7 * np.exp(np.longdouble(-80))
    assert abs(h[0] + 81 * eps) <= 1e-15 * 81 * eps and abs(p[0, 3] - (1 - eps)) <= 1e-18 and p[0, 0] > 0


def test_fc_padding_for_ten_classes():
    g = torch.Generator().manual_seed(1)
    w, b = torch.randn(10, 2048, generator=g), torch.randn(10, generator=g)
    wp, bp = pad_fc(w, b)
    assert wp.shape == (16, 2048) and bp.shape == (16,) and wp.dtype == torch.float32 and wp.is_contiguous()
    assert torch.equal(wp[:10], w) and torch.equal(bp[:10], b)
    assert float(wp[10:].abs().max()) == 0 and float(bp[10:].abs().max()) == 0
    wp, bp = pad_fc(torch.randn(1000, 64, generator=g).double(), torch.randn(1000, generator=g))
    assert wp.shape == (1000, 64) and wp.dtype == torch.float32


def test_constructor_arguments():
    w, b = torch.zeros(10, 2048), torch.zeros(10)
    for args, kw in (((w[:1], b[:1]), {}), ((w[:, :2044], b), {}), ((w, b[:9]), {}), ((w, b), dict(split_size=0)),
                     ((w, b), dict(max_rows=0))):
        with pytest.raises(ValueError):
            InceptionScore(*args, **kw)
    with pytest.raises(KeyError, match="fc.bias"):
        InceptionScore.load_fc({"fc.weight": w})


def test_entry_points_validate_before_any_hip_call():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    lib = _lib.load()
    err = lib.vtp_last_error
    p = ctypes.c_void_p(16)

    name, ok = b"vtp_is_rows", [p, 16, 4, 10, p, 10, p, None]  # logits ldl B C p ldp h stream
    for i in (0, 4, 6):
        a = list(ok)
        a[i] = None
        assert lib.vtp_is_rows(*a) == -1 and err().startswith(name) and b"null" in err(), i
    for i, v, msg in ((2, 0, b"B, C"), (3, 0, b"B, C"), (1, 9, b"leading"), (5, 9, b"leading")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_is_rows(*a) == -1 and err().startswith(name) and msg in err(), (i, v, err())

    name, ok = b"vtp_is_accum", [p, 10, p, 100, 50, 4, 10, p, 3, None]  # p ldp h row_base split_size B C state n_slots stream
    for i in (0, 2, 7):
        a = list(ok)
        a[i] = None
        assert lib.vtp_is_accum(*a) == -1 and err().startswith(name) and b"null" in err(), i
    for i, v, msg in ((5, 0, b"B, C"), (6, 0, b"B, C"), (1, 9, b"ldp"), (4, 0, b"split_size"), (3, -1, b"row_base"),
                      (3, 147, b"slot"), (8, 2, b"slot"), (8, 0, b"slot")):  # rows 147 .. 150 reach slot 3 of 3
        a = list(ok)
        a[i] = v
        assert lib.vtp_is_accum(*a) == -1 and err().startswith(name) and msg in err(), (i, v, err())
    a = list(ok)
    a[3], a[4], a[5], a[8] = 0, 1, 70000, 70000  # one row per slot: more slots than one launch takes
    assert lib.vtp_is_accum(*a) == -1 and b"65535" in err()


def test_op_wrappers_check_tensors_before_any_launch():
    from vtp_amd import ops
    f64 = torch.float64
    lg, p, h = torch.zeros(4, 16), torch.zeros(4, 10, dtype=f64), torch.zeros(4, dtype=f64)
    for bad in (dict(lg=lg.double()), dict(lg=lg.t()), dict(C=17), dict(C=0), dict(p=torch.zeros(4, 10)), dict(p=torch.zeros(4, 9, dtype=f64)),
                dict(h=torch.zeros(3, dtype=f64)), dict(p=torch.zeros(4, 16, dtype=f64)[:, :10])):
        a = dict(lg=lg, C=10, p=p, h=h)
        a.update(bad)
        with pytest.raises(ValueError, match="must"):
            ops.is_rows(a["lg"], a["C"], a["p"], a["h"])
    with pytest.raises(ValueError, match="no CPU path"):
        ops.is_rows(lg, 10, p, h)
    state = torch.zeros(3, 11, dtype=f64)
    for bad in (dict(p=p.float()), dict(h=h[:3]), dict(state=torch.zeros(3, 10, dtype=f64)), dict(state=state.float())):
        a = dict(p=p, h=h, state=state)
        a.update(bad)
        with pytest.raises(ValueError, match="must"):
            ops.is_accum(a["p"], a["h"], a["state"], 0, 50)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.is_accum(p, h, state, 0, None)


def test_gen_eval_result_keys_for_every_combination_of_inputs():
    from vtp_amd.gen_eval import result_keys
    for fc, ref, ref_s, real, pr in itertools.product((False, True), (False, True), (False, True), (0, 1, 12), (False, True)):
        if ref_s and not ref:
            continue  # the spatial statistics come with the pool statistics
        keys = result_keys(fc, ref, ref_s, real, pr)
        assert ("fid" in keys) == (ref or real >= 2)
        assert ("sfid" in keys) == (ref_s or real >= 2)  # set_reference without mu_s: no sfid unless real images were added
        assert ("is" in keys) == ("is_std" in keys) == fc
        assert ("precision" in keys) == ("recall" in keys) == (pr and real >= 1)
        assert set(keys) <= {"fid", "sfid", "is", "is_std", "precision", "recall"} and len(set(keys)) == len(keys)
    assert result_keys(True, True, True, 12) == ("fid", "sfid", "is", "is_std", "precision", "recall")
    assert result_keys(False, True, False, 0) == ("fid",)
