"""GPU checks of the FID kernels and classes (csrc/fid.hip, vtp_amd/fid.py) against fp64 references and tests/fid_ref.py.

Bounds.  gamma_n = n u / (1 - n u), u = 2^-24, is the a-priori error of n fp32 roundings in a chain.  A convolution output is a
product chain over K = kh kw Cin terms that starts at the bias: |err| <= gamma_{K+2} (|x| (*) |w| + |b|) elementwise (the bound of
tests/test_zeroshot_gpu.py).  A sum of n terms and one division: gamma_{n+1} sum|x| / divisor.  The resize works in fp64 and
rounds once (u |v|, inside the 4 u max|x| asked for).  The fp64 accumulator: gamma_{n+1} in fp64 of sum |x_i x_j|.
The network has no a-priori bound worth stating: E = max|f - f64| / max|f64| of ours must stay within twice that of the
restatement's own fp32 runs (CPU and GPU), both printed."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -7.25


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- convolution
# (Cin, Cout, (kh, kw), stride, (ph, pw), H, W): one case per geometry the network has
CONV_CASES = {
    "3-32_k3_s2": (3, 32, (3, 3), 2, (0, 0), 21, 23),
    "64-80_k1": (64, 80, (1, 1), 1, (0, 0), 9, 11),
    "48-64_k5_p2": (48, 64, (5, 5), 1, (2, 2), 9, 11),
    "160-160_1x7": (160, 160, (1, 7), 1, (0, 3), 9, 11),
    "160-192_7x1": (160, 192, (7, 1), 1, (3, 0), 9, 11),
    "288-384_k3_s2": (288, 384, (3, 3), 2, (0, 0), 9, 11),
    "384-384_1x3": (384, 384, (1, 3), 1, (0, 1), 9, 11),
    "384-384_3x1": (384, 384, (3, 1), 1, (1, 0), 9, 11),
    "448-384_k3_p1": (448, 384, (3, 3), 1, (1, 1), 9, 11),
}


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    """inputs and the fp64 reference with its bound, computed once per geometry on the CPU"""
    cin, cout, k, s, p, H, W = CONV_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(3, H, W, cin, generator=g)
    w = torch.randn(cout, k[0], k[1], cin, generator=g) * (cin * k[0] * k[1]) ** -0.5
    b = torch.randn(cout, generator=g)
    xd, wd = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    ref = F.conv2d(xd, wd, b.double(), s, p).permute(0, 2, 3, 1).contiguous()
    mag = F.conv2d(xd.abs(), wd.abs(), b.double().abs(), s, p).permute(0, 2, 3, 1).contiguous()
    return x, w, b, ref, R.gamma(k[0] * k[1] * cin + 2) * mag


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_within_the_chain_bound_slice_and_batch_independence(name, relu):
    from vtp_amd import ops
    dev = _dev()
    cin, cout, k, s, p, H, W = CONV_CASES[name]
    x, w, b, ref, bound = _conv_case(name)
    xg, wg, bg = x.to(dev), w.to(dev), b.to(dev)
    ho, wo = ops.conv_out_size(H, W, k[0], k[1], s, p[0], p[1])
    assert ref.shape == (3, ho, wo, cout)
    y = torch.full((3, ho, wo, cout + 64), SENTINEL, device=dev)
    ops.conv2d_f32(xg, wg, bg, y, stride=s, pad=p, relu=relu, c0=32)
    got = y[..., 32:32 + cout]
    want = ref.clamp_min(0) if relu else ref
    err = (got.double().cpu() - want).abs()
    print(f"{name} relu={relu}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    sent = torch.full((3, ho, wo, 32), SENTINEL, device=dev)
    assert torch.equal(_bits(y[..., :32]), _bits(sent)) and torch.equal(_bits(y[..., 32 + cout:]), _bits(sent))
    for i in range(3):  # the same image alone: the same bits
        y1 = torch.full((1, ho, wo, cout + 64), SENTINEL, device=dev)
        ops.conv2d_f32(xg[i:i + 1].contiguous(), wg, bg, y1, stride=s, pad=p, relu=relu, c0=32)
        assert torch.equal(_bits(y1[0]), _bits(y[i])), f"image {i} differs between a batch of 3 and a batch of 1"


def test_conv_repeats_bit_for_bit_and_takes_no_bias():
    from vtp_amd import ops
    dev = _dev()
    x, w, b, ref, bound = _conv_case("48-64_k5_p2")
    xg, wg = x.to(dev), w.to(dev)
    ys = []
    for _ in range(2):
        y = torch.empty(3, 9, 11, 64, device=dev)
        ops.conv2d_f32(xg, wg, None, y, stride=1, pad=(2, 2), relu=False)
        ys.append(y)
    assert torch.equal(_bits(ys[0]), _bits(ys[1]))
    assert bool(((ys[0].double().cpu() - (ref - b.double())).abs() <= bound).all())


# ---------------------------------------------------------------------------------------------------------------- pooling, resize
@pytest.mark.parametrize("stride", [1, 2])
def test_pooling(stride):
    from vtp_amd import ops
    dev = _dev()
    B, H, W, C = 2, 9, 11, 20
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(7))
    xg, xn = x.to(dev), x.permute(0, 3, 1, 2)
    xnan = x.clone()
    xnan[0, 4, 5, 3] = xnan[1, 0, 0, 7] = float("nan")
    pad = 1 if stride == 1 else 0
    ho, wo = ((H, W) if stride == 1 else ((H - 3) // 2 + 1, (W - 3) // 2 + 1))
    sent = torch.full((B, ho, wo, 4), SENTINEL, device=dev)

    def run(mode):
        y = torch.full((B, ho, wo, C + 8), SENTINEL, device=dev)
        ops.pool3x3_f32(xg, y, stride, mode, c0=4)
        assert torch.equal(_bits(y[..., :4]), _bits(sent)) and torch.equal(_bits(y[..., 4 + C:]), _bits(sent))
        return y[..., 4:4 + C].cpu().permute(0, 3, 1, 2)

    assert torch.equal(_bits(run(ops.POOL_MAX)), _bits(F.max_pool2d(xn, 3, stride, pad)))
    y = torch.empty(B, ho, wo, C, device=dev)  # a NaN tap gives NaN, as in torch
    ops.pool3x3_f32(xnan.to(dev), y, stride, ops.POOL_MAX)
    want = F.max_pool2d(xnan.permute(0, 3, 1, 2), 3, stride, pad)
    got = y.cpu().permute(0, 3, 1, 2)
    assert bool(want.isnan().any()) and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))
    for mode, include in ((ops.POOL_AVG, True), (ops.POOL_AVG_INSIDE, False)):
        ref = F.avg_pool2d(xn.double(), 3, stride, pad, count_include_pad=include)
        bound = R.gamma(9 + 1) * F.avg_pool2d(xn.double().abs(), 3, stride, pad, count_include_pad=include)
        assert bool(((run(mode).double() - ref).abs() <= bound).all()), mode


def test_global_average_pool():
    from vtp_amd import ops
    dev = _dev()
    x = torch.randn(3, 5, 7, 2048, generator=torch.Generator().manual_seed(8))
    y = torch.empty(3, 2048, device=dev)
    ops.global_avgpool_f32(x.to(dev), y)
    ref = x.double().mean((1, 2))
    bound = R.gamma(35 + 1) * x.double().abs().mean((1, 2))
    assert bool(((y.double().cpu() - ref).abs() <= bound).all())


@pytest.mark.parametrize("H,W", [(64, 64), (91, 107), (350, 310), (299, 299)])
def test_bilinear_resize_and_repack(H, W):
    from vtp_amd import ops
    dev = _dev()
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(9))
    ref = F.interpolate(x.double(), size=(299, 299), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    y = torch.empty(2, 299, 299, 3, device=dev)
    ops.resize_bilinear_nhwc(x.to(dev), y, 1.0, 0.0)
    err = float((y.double().cpu() - ref).abs().max())
    print(f"resize {H}x{W}: max err {err:.3e} = {err / U:.2f} u")
    assert err <= 4 * U * float(x.abs().max())
    ops.resize_bilinear_nhwc(x.to(dev), y, 2.0, -1.0)
    assert float((y.double().cpu() - (2 * ref - 1)).abs().max()) <= 4 * U * float(x.abs().max())
    z = torch.empty(2, H, W, 3, device=dev)  # equal sizes: the NCHW -> NHWC repack, a copy
    ops.resize_bilinear_nhwc(x.to(dev), z, 1.0, 0.0)
    assert torch.equal(_bits(z.cpu()), _bits(x.permute(0, 2, 3, 1)))


# ---------------------------------------------------------------------------------------------------------------- the network
@functools.lru_cache(maxsize=None)
def _weights():
    sd64 = R.seeded_state_dict(0, torch.float64)
    return sd64, {k: v.float() for k, v in sd64.items()}


def _rel(f, f64):
    return float((f.double().cpu() - f64).abs().max() / f64.abs().max())


@functools.lru_cache(maxsize=None)
def _net_case(variant, B, H, W):
    """(ours, fp64 restatement, E_ref) for one input; E_ref = the larger error of the restatement's fp32 runs on CPU and GPU"""
    from vtp_amd import InceptionFeatures
    dev = _dev()
    sd64, sd32 = _weights()
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(B * H + W))
    f64 = R.features(sd64, x.double(), variant)
    e_cpu = _rel(R.features(sd32, x, variant), f64)
    e_gpu = _rel(R.features({k: v.to(dev) for k, v in sd32.items()}, x.to(dev), variant), f64)
    inc = InceptionFeatures(variant).reset_parameters(0).to(dev)
    ours = inc(x.to(dev))
    return ours, f64, max(e_cpu, e_gpu), (e_cpu, e_gpu), inc, x


@pytest.mark.parametrize("B,H,W", [(3, 91, 107), (2, 299, 299)])
@pytest.mark.parametrize("variant", ["torchvision", "pytorch_fid"])
def test_network_error_within_twice_the_restatements_own(variant, B, H, W):
    ours, f64, e_ref, (e_cpu, e_gpu), inc, x = _net_case(variant, B, H, W)
    assert ours.shape == (B, 2048) and ours.dtype == torch.float32 and bool(torch.isfinite(ours).all())
    e_ours = _rel(ours, f64)
    print(f"fid network {variant} B={B} {H}x{W}: E_ours {e_ours:.3e}  E_ref {e_ref:.3e} (cpu {e_cpu:.3e}, gpu {e_gpu:.3e})  "
          f"ratio {e_ours / e_ref:.3f}")
    assert e_ours <= 2 * e_ref
    one = inc(x[1:2].to(ours.device))  # an image's features do not depend on its batch, and repeat
    assert torch.equal(_bits(one[0]), _bits(ours[1]))


def test_moved_and_reloaded_module_folds_its_new_weights():
    """.cpu() / .cuda() hand out fresh buffers whose version counters restart: the weights folded before must not be reused"""
    from vtp_amd import InceptionFeatures
    dev = _dev()
    x = torch.rand(1, 3, 80, 91, generator=torch.Generator().manual_seed(5)).to(dev)
    inc = InceptionFeatures().reset_parameters(0).to(dev)
    f0 = inc(x)
    inc.cpu()
    inc.load_state_dict(R.seeded_state_dict(1))
    inc.to(dev)
    f1 = inc(x)
    fresh = InceptionFeatures().reset_parameters(1).to(dev)(x)
    assert torch.equal(_bits(f1), _bits(fresh)) and not torch.equal(_bits(f1), _bits(f0))


def test_network_refuses_the_cpu_and_small_inputs():
    from vtp_amd import InceptionFeatures
    dev = _dev()
    inc = InceptionFeatures().reset_parameters(0)
    with pytest.raises(ValueError, match="no CPU path"):
        inc.to(dev)(torch.rand(1, 3, 91, 91))
    with pytest.raises(ValueError, match="at least"):
        inc(torch.rand(1, 3, 74, 91, device=dev))


# ---------------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("D,n", [(2048, 5), (70, 37)])
def test_accumulator_bound_and_split_invariance(D, n):
    from vtp_amd import ops
    dev = _dev()
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(D + n)) + 0.5
    xg = x.to(dev)

    def run(splits):
        s = torch.zeros(D, device=dev, dtype=torch.float64)
        o = torch.zeros(D, D, device=dev, dtype=torch.float64)
        at = 0
        for m in splits:
            ops.fid_accum(xg[at:at + m], s, o)
            at += m
        assert at == n
        return s, o

    s, o = run([n])
    xd = x.double()

    def exact(terms):
        """sum over the leading axis of fp64 terms by a two-sum chain: the rounded total plus the collected rounding errors, which
        is the exact sum to about u^2 -- the terms themselves (an f32 value, or the product of two) are exact in fp64"""
        tot, low = torch.zeros_like(terms[0]), torch.zeros_like(terms[0])
        for p in terms:
            t = tot + p
            bp = t - tot
            low += (tot - (t - bp)) + (p - bp)
            tot = t
        return tot + low

    g = R.gamma64(n + 1)
    assert bool(((s.cpu() - exact(xd)).abs() <= g * xd.abs().sum(0)).all())
    prods = xd[:, :, None] * xd[:, None, :]  # [n, D, D]: 24-bit x 24-bit significands, exact
    assert bool(((o.cpu() - exact(prods)).abs() <= g * prods.abs().sum(0)).all())
    splits = ([20, 17], [1] * 37) if n == 37 else ([3, 2], [1] * 5)
    for sp in splits:
        s2, o2 = run(sp)
        assert torch.equal(s2.view(torch.int64), s.view(torch.int64)) and torch.equal(o2.view(torch.int64), o.view(torch.int64))


def _two_gaussians(D=128, n=2048):
    rng = np.random.default_rng(11)
    a = (rng.standard_normal((n, D)) @ (rng.standard_normal((D, D)) / np.sqrt(D)) + rng.standard_normal(D)).astype(np.float32)
    b = (1.3 * rng.standard_normal((n, D)) @ (rng.standard_normal((D, D)) / np.sqrt(D)) + 0.5 + rng.standard_normal(D)).astype(np.float32)
    return a, b


def test_frechet_stats_against_numpy_and_the_distance():
    from vtp_amd import FrechetStats, frechet_distance
    dev = _dev()
    a, b = _two_gaussians()
    st = [FrechetStats(128, dev), FrechetStats(128, dev)]
    for s, act in zip(st, (a, b)):
        t = torch.from_numpy(act).to(dev)
        for lo in range(0, 2048, 500):  # uneven batches
            s.update(t[lo:lo + 500])
        assert s.n == 2048
    got, want = [], []
    for s, act in zip(st, (a, b)):
        mu, sigma = s.mean_cov()
        mu_n, sigma_n = R.statistics(act)
        assert mu.dtype == np.float64 and sigma.shape == (128, 128)
        assert np.abs(mu - mu_n).max() <= 1e-12 * np.abs(mu_n).max()
        assert np.abs(sigma - sigma_n).max() <= 1e-12 * np.abs(sigma_n).max()
        got += [mu, sigma]
        want += [mu_n, sigma_n]
    for method in ("eig", "auto"):
        d, d_n = frechet_distance(*got, method=method), frechet_distance(*want, method=method)
        assert d_n > 1 and abs(d - d_n) <= 1e-9 * d_n
    sd = st[0].state_dict()
    other = FrechetStats(128, dev)
    other.load_state_dict(sd)
    assert np.array_equal(other.mean_cov()[1], st[0].mean_cov()[1])
    st[0].reset()
    assert st[0].n == 0 and float(st[0].outer.abs().max()) == 0
    with pytest.raises(RuntimeError):
        st[0].mean_cov()


def _byte_images(seed, n=2, S=64):
    """smooth random byte images [n, S, S, 3]"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, 8, 8, generator=g)
    img = F.interpolate(low, size=(S, S), mode="bicubic", align_corners=False) + 0.05 * torch.randn(n, 3, S, S, generator=g)
    return (img.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _pil_resized(u8):
    from PIL import Image
    out = [np.asarray(Image.fromarray(a).resize((299, 299), Image.BILINEAR)) for a in u8.numpy()]
    return torch.from_numpy(np.stack(out)).permute(0, 3, 1, 2).double() / 255


def test_fid_update_against_the_fp64_pipeline():
    """two batches of two byte images a side.  The fp64 pipeline: Pillow's resize, ToTensor, the restatement in fp64, np.cov.  mu and
    sigma of ours are held to twice the error the restatement's own fp32 features (CPU and GPU) leave in the same statistics"""
    from vtp_amd import FID, InceptionFeatures
    dev = _dev()
    sd64, sd32 = _weights()
    sd32g = {k: v.to(dev) for k, v in sd32.items()}
    fid = FID(InceptionFeatures("torchvision").reset_parameters(0).to(dev))
    sides = {"ref": [_byte_images(21), _byte_images(22)], "rec": [_byte_images(23), _byte_images(24)]}
    for r, c in zip(sides["ref"], sides["rec"]):
        fid.update(r.to(dev), c.to(dev))
    assert fid.ref.n == 4 and fid.rec.n == 4
    for side, st in (("ref", fid.ref), ("rec", fid.rec)):
        x = _pil_resized(torch.cat(sides[side]))
        mu64, s64 = R.statistics(R.features(sd64, x).numpy())
        e_mu, e_s = 0.0, 0.0
        for f32 in (R.features(sd32, x.float()), R.features(sd32g, x.float().to(dev)).cpu()):
            mu32, s32 = R.statistics(f32.numpy())
            e_mu = max(e_mu, np.abs(mu32 - mu64).max() / np.abs(mu64).max())
            e_s = max(e_s, np.abs(s32 - s64).max() / np.abs(s64).max())
        mu, sigma = st.mean_cov()
        o_mu, o_s = np.abs(mu - mu64).max() / np.abs(mu64).max(), np.abs(sigma - s64).max() / np.abs(s64).max()
        print(f"FID.update {side}: mu E_ours {o_mu:.3e} E_ref {e_mu:.3e}; sigma E_ours {o_s:.3e} E_ref {e_s:.3e}")
        assert o_mu <= 2 * e_mu and o_s <= 2 * e_s
    d = fid.result("eig")
    assert np.isfinite(d) and np.isfinite(fid.result())
    fid.reset()
    assert fid.ref.n == 0 and fid.rec.n == 0


def test_fid_update_pytorch_fid_variant_and_features_entry():
    from vtp_amd import FID, InceptionFeatures
    dev = _dev()
    fid = FID(InceptionFeatures("pytorch_fid").reset_parameters(0).to(dev))
    for s in (31, 32):
        fid.update(_byte_images(s).to(dev), _byte_images(s + 10).to(dev))
    assert fid.ref.n == 4 and fid.rec.n == 4 and np.isfinite(fid.result("eig"))
    f = fid.features(_byte_images(31).to(dev))
    other = FID(fid.inception)
    other.update_features(f, f)
    other.update_features(fid.features(_byte_images(32).to(dev)), fid.features(_byte_images(32).to(dev)))
    assert np.array_equal(other.ref.mean_cov()[1], fid.ref.mean_cov()[1])  # the same rows in the same order: the same bits
    with pytest.raises(ValueError):
        fid.update(torch.zeros(2, 3, 64, 64, device=dev), torch.zeros(2, 3, 64, 64, device=dev))


# ---------------------------------------------------------------------------------------------------------------- ReconEval
def test_recon_eval_feeds_the_fid_and_is_unchanged_without_one():
    from vtp_amd import FID, InceptionFeatures, ReconEval
    dev = _dev()
    g = torch.Generator().manual_seed(41)
    inc = InceptionFeatures("pytorch_fid").reset_parameters(0).to(dev)
    fid, alone = FID(inc), FID(inc)
    ev, plain = ReconEval(None, fid=fid), ReconEval(None)
    for _ in range(2):
        x = torch.randn(2, 3, 64, 64, generator=g).to(dev)
        y = (x + 0.2 * torch.randn(2, 3, 64, 64, generator=g).to(dev))
        out = ev.update_pair(x, y)
        assert out.ref_u8 is None and out.rec_u8 is None  # want_u8 was not set
        ref = plain.update_pair(x, y, want_u8=True)
        alone.update(ref.ref_u8, ref.rec_u8)
    res, base = ev.results(), plain.results()
    assert set(base) == {"psnr", "ssim", "lpips", "num_samples", "ssim_per_image", "lpips_per_image", "identical_images"}
    assert set(res) == set(base) | {"fid"}
    assert res["fid"] == alone.result() and np.isfinite(res["fid"])
    assert all(res[k] == base[k] for k in base)
    ev.reset()
    assert fid.ref.n == 0
