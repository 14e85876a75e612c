"""CPU-side checks of the FID feature (vtp_amd/fid.py against tests/fid_ref.py): the restated network's shape, the state-dict
contract, BatchNorm folding in fp64, the Frechet distance against a closed form, and the seeded weights the GPU tests rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_ref as R
from vtp_amd import fid as FD


@pytest.fixture(scope="module")
def sd64():
    return R.seeded_state_dict(0, torch.float64)


def test_restatement_has_94_convolutions_and_the_tables_keys():
    assert len(R.CONVS) == 94 and len(FD.INCEPTION_CONVS) == 94
    m = FD.InceptionFeatures()
    assert list(m.state_dict().keys()) == R.state_dict_keys()
    for (name, cin, cout, k, s, p) in FD.INCEPTION_CONVS:
        rc = R.CONVS[name]
        pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
        assert (cin, cout, k, s, p) == (rc[0], rc[1], pair(rc[2]), rc[3], pair(rc[4])), name
    assert m.state_dict()["Mixed_6c.branch7x7dbl_3.conv.weight"].shape == (160, 160, 1, 7)
    assert abs(FD.forward_gflop(299, 299) / 2 - 5.7) < 0.05  # the 5.7 G multiply-adds torchvision's network is quoted at


@pytest.mark.parametrize("variant", ["torchvision", "pytorch_fid"])
def test_output_shape_and_spatial_sizes(sd64, variant):
    sd = {k: v.float() for k, v in sd64.items()}
    g = torch.Generator().manual_seed(1)
    assert R.features(sd, torch.rand(1, 3, 75, 75, generator=g), variant).shape == (1, 2048)
    trace = []
    out = R.features(sd, torch.rand(2, 3, 91, 107, generator=g), variant, trace)
    assert out.shape == (2, 2048)
    at = dict(trace)
    names = ["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "maxpool2", "Mixed_5d",
             "Mixed_6a", "Mixed_7c"]
    if variant == "torchvision":
        assert [at[n].shape[2] for n in names[:-1]] == [45, 43, 43, 21, 21, 19, 9, 9, 4]
        assert [at[n].shape[3] for n in names[:-1]] == [53, 51, 51, 25, 25, 23, 11, 11, 5]
        assert at["Mixed_7c"].shape == (2, 2048, 1, 2)
    else:  # resized to 299 first
        assert [at[n].shape[2] for n in names] == [149, 147, 147, 73, 73, 71, 35, 35, 17, 8]
    assert [at[n].shape[1] for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6e", "Mixed_7a", "Mixed_7b")] == \
        [256, 288, 288, 768, 768, 1280, 2048]


def test_variants_differ_only_where_stated(sd64):
    """at 299 x 299 the resize is the identity; feeding (x + 1) / 2 undoes the affine: what remains is the pooling difference"""
    sd = {k: v.float() for k, v in sd64.items()}
    x = torch.rand(1, 3, 299, 299, generator=torch.Generator().manual_seed(2))
    ta, tb = [], []
    R.features(sd, x, "torchvision", ta)
    R.features(sd, (x + 1) / 2, "pytorch_fid", tb)
    a, b = dict(ta), dict(tb)
    assert torch.allclose(a["maxpool2"], b["maxpool2"], atol=1e-5)  # the stem is shared
    assert not torch.allclose(a["Mixed_5b"][:, 224:], b["Mixed_5b"][:, 224:], atol=1e-4)  # the pool branch is not
    assert torch.allclose(a["Mixed_5b"][:, :224], b["Mixed_5b"][:, :224], atol=1e-4)


@pytest.mark.parametrize("name", ["Conv2d_1a_3x3", "Mixed_5b.branch5x5_2", "Mixed_6c.branch7x7dbl_3", "Mixed_7a.branch3x3_2"])
def test_folded_conv_equals_conv_then_batchnorm_in_fp64(sd64, name):
    cin, cout, k, s, p = R.CONVS[name]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, cin, 13, 15, generator=g, dtype=torch.float64)
    w = sd64[name + ".conv.weight"]
    bn = [sd64[name + ".bn." + t] for t in ("weight", "bias", "running_mean", "running_var")]
    want = F.batch_norm(F.conv2d(x, w, None, s, p), bn[2], bn[3], bn[0], bn[1], training=False, eps=1e-3)
    wf, bf = FD.fold_conv_bn(w, *bn)
    assert wf.dtype == torch.float64 and bf.dtype == torch.float64
    got = F.conv2d(x, wf, bf, s, p)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_state_dict_contract(sd64):
    m = FD.InceptionFeatures()
    sd = {k: v.float() for k, v in sd64.items()}
    extra = dict(sd)
    extra["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    extra["AuxLogits.fc.weight"] = torch.zeros(1000, 768)
    extra["fc.weight"] = torch.zeros(1000, 2048)
    extra["fc.bias"] = torch.zeros(1000)
    extra["Conv2d_1a_3x3.bn.num_batches_tracked"] = torch.tensor(7)
    m.load_state_dict(extra)
    assert torch.equal(m.state_dict()["Mixed_7c.branch_pool.bn.running_var"], sd["Mixed_7c.branch_pool.bn.running_var"])
    for gone in ("Mixed_6a.branch3x3.conv.weight", "Conv2d_2b_3x3.bn.running_mean"):
        short = {k: v for k, v in sd.items() if k != gone}
        with pytest.raises(RuntimeError, match="Missing key"):
            m.load_state_dict(short)
    with pytest.raises(ValueError):
        FD.InceptionFeatures("tf")


def test_reset_parameters_is_the_restated_recipe(sd64):
    m = FD.InceptionFeatures().reset_parameters(0)
    for k, v in m.state_dict().items():
        assert torch.equal(v.double(), sd64[k]), k


def test_seeded_weights_keep_the_features_alive(sd64):
    """the GPU tests compare features of these weights: they must neither die nor blow up on the way through 94 layers"""
    x = torch.rand(2, 3, 91, 107, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    for variant in ("torchvision", "pytorch_fid"):
        f = R.features(sd64, x, variant)
        assert torch.isfinite(f).all() and float(f.abs().max()) > 0
        assert 1e-2 <= float(f.std()) <= 1e2, float(f.std())


def _commuting(D=48, seed=5):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    a, b = rng.uniform(0.5, 2.0, D), rng.uniform(0.5, 2.0, D)
    mu1, mu2 = rng.standard_normal(D), rng.standard_normal(D)
    return mu1, (q * a) @ q.T, mu2, (q * b) @ q.T, a, b


@pytest.mark.parametrize("method", ["eig", "scipy"])
def test_frechet_distance_against_the_closed_form(method):
    if method == "scipy":
        pytest.importorskip("scipy")
    mu1, s1, mu2, s2, a, b = _commuting()
    want = float(np.sum((mu1 - mu2) ** 2) + np.sum(a + b - 2 * np.sqrt(a * b)))
    tol = 1e-10 * (np.trace(s1) + np.trace(s2))
    assert abs(FD.frechet_distance(mu1, s1, mu2, s2, method) - want) <= tol
    assert abs(FD.frechet_distance(mu1, s1, mu1, s1, method)) <= tol
    if method == "scipy":
        assert abs(R.frechet(mu1, s1, mu2, s2) - want) <= tol


def test_frechet_distance_arguments():
    mu1, s1, mu2, s2, _, _ = _commuting(8)
    with pytest.raises(ValueError):
        FD.frechet_distance(mu1, s1, mu2, s2, "cholesky")
    with pytest.raises(ValueError):
        FD.frechet_distance(mu1[:4], s1, mu2, s2)
    assert FD.frechet_distance(mu1, s1, mu2, s2) == FD.frechet_distance(mu1, s1, mu2, s2, "auto")


def test_entry_points_validate_before_any_hip_call():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.vtp_conv2d_f32(None, p, p, p, 1, 9, 9, 16, 32, 3, 3, 1, 1, 1, 1, 0, 32, None) == -1 and b"null" in lib.vtp_last_error()
    assert lib.vtp_conv2d_f32(p, p, p, p, 1, 9, 9, 16, 32, 2, 3, 1, 0, 0, 1, 0, 32, None) == -1 and b"kh, kw" in lib.vtp_last_error()
    assert lib.vtp_conv2d_f32(p, p, p, p, 1, 9, 9, 16, 32, 3, 3, 3, 0, 0, 1, 0, 32, None) == -1 and b"stride" in lib.vtp_last_error()
    assert lib.vtp_conv2d_f32(p, p, p, p, 1, 9, 9, 16, 32, 3, 3, 1, 0, 0, 1, 8, 32, None) == -1 and b"slice" in lib.vtp_last_error()
    assert lib.vtp_conv2d_f32(p, p, p, p, 1, 2, 9, 16, 32, 3, 3, 1, 0, 0, 1, 0, 32, None) == -1 and b"smaller" in lib.vtp_last_error()
    assert lib.vtp_conv2d_f32(ctypes.c_void_p(20), p, p, p, 1, 9, 9, 16, 32, 3, 3, 1, 0, 0, 1, 0, 32, None) == -1
    assert b"aligned" in lib.vtp_last_error()
    assert lib.vtp_pool3x3_f32(p, p, 1, 9, 9, 6, 1, 0, 0, 8, None) == -1
    assert lib.vtp_pool3x3_f32(p, p, 1, 9, 9, 8, 1, 3, 0, 8, None) == -1 and b"mode" in lib.vtp_last_error()
    assert lib.vtp_pool3x3_f32(p, p, 1, 2, 9, 8, 2, 0, 0, 8, None) == -1
    assert lib.vtp_global_avgpool_f32(p, None, 1, 4, 8, None) == -1
    assert lib.vtp_resize_bilinear_nhwc(p, p, 1, 3, 0, 4, 8, 8, 1.0, 0.0, None) == -1
    assert lib.vtp_fid_accum(p, 4, p, p, 3, 8, None) == -1 and b"ldf" in lib.vtp_last_error()
    assert lib.vtp_fid_accum(p, 8, p, None, 3, 8, None) == -1


def test_op_wrappers_check_tensors_before_any_launch():
    """the kernels see pointers only: a wrong dtype, shape or layout must raise in the wrapper (checked before the device is)"""
    from vtp_amd import ops
    x, w, b = torch.zeros(1, 9, 9, 16), torch.zeros(32, 3, 3, 16), torch.zeros(32)
    y = torch.zeros(1, 7, 7, 32)
    for bad in (dict(x=x.double()), dict(w=torch.zeros(32, 3, 3, 8)), dict(b=torch.zeros(31)), dict(y=torch.zeros(1, 7, 6, 32)),
                dict(y=torch.zeros(1, 7, 7, 31)), dict(y=torch.zeros(1, 7, 7, 64)[..., :32]), dict(y=y.double()), dict(c0=1)):
        a = dict(x=x, w=w, b=b, y=y, c0=0)
        a.update(bad)
        with pytest.raises(ValueError, match="must"):
            ops.conv2d_f32(a["x"], a["w"], a["b"], a["y"], c0=a["c0"])
    with pytest.raises(ValueError, match="no CPU path"):  # everything else in order: only the device is wrong here
        ops.conv2d_f32(x, w, b, y)
    with pytest.raises(ValueError, match="y must be"):
        ops.pool3x3_f32(x, torch.zeros(1, 9, 9, 12), 1, ops.POOL_MAX)
    with pytest.raises(ValueError, match="y must be"):
        ops.pool3x3_f32(x, torch.zeros(1, 5, 4, 16), 2, ops.POOL_MAX)
    with pytest.raises(ValueError, match="y must be"):
        ops.global_avgpool_f32(x, torch.zeros(1, 8))
    with pytest.raises(ValueError, match="y must be"):
        ops.resize_bilinear_nhwc(torch.zeros(2, 3, 8, 8), torch.zeros(2, 16, 16, 4))
    f = torch.zeros(5, 8)
    with pytest.raises(ValueError, match="sum_ must be"):
        ops.fid_accum(f, torch.zeros(8), torch.zeros(8, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="outer must be"):
        ops.fid_accum(f, torch.zeros(8, dtype=torch.float64), torch.zeros(8, 7, dtype=torch.float64))
    with pytest.raises(ValueError, match="feats must be"):
        ops.fid_accum(f.t(), torch.zeros(5, dtype=torch.float64), torch.zeros(5, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.fid_accum(f, torch.zeros(8, dtype=torch.float64), torch.zeros(8, 8, dtype=torch.float64))


def test_folded_weights_are_forgotten_when_the_module_moves_or_loads():
    m = FD.InceptionFeatures().reset_parameters(0)
    for act in (lambda: m.cpu(), lambda: m.load_state_dict(m.state_dict()), lambda: m.reset_parameters(1), lambda: m.float()):
        m._prepped = ("stale",)
        act()
        assert m._prepped is None
