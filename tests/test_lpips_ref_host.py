"""The references of tests/lpips_ref.py against independent torch code, and the proof that the bars of tests/test_lpips_kernels_gpu.py
discriminate: a deliberately wrong variant of each reference misses the GPU test's bar at the GPU test's own inputs.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def _shuffle(tok, n, H, W):
    """tokens [n*hw, 768] -> image [n, 3, H, W] by F.pixel_shuffle"""
    return F.pixel_shuffle(tok.view(n, H // 16, W // 16, 768).permute(0, 3, 1, 2), 16)


def _unshuffle(img):
    n, _, H, W = img.shape
    return F.pixel_unshuffle(img, 16).permute(0, 2, 3, 1).reshape(n * (H // 16) * (W // 16), 768)


def _unfold_torch(scaled):
    """[n, 3, H, W] -> [n, H, W, 27] in (ky, kx, c) order by F.unfold (whose own order is (c, ky, kx))"""
    n, _, H, W = scaled.shape
    cols = F.unfold(F.pad(scaled, (1, 1, 1, 1)), 3).view(n, 3, 3, 3, H, W)  # [n, c, ky, kx, H, W]
    return cols.permute(0, 4, 5, 2, 3, 1).reshape(n, H, W, 27)


def _swap_taps(a):
    """[..., 32] with the 27 live columns re-ordered as if ky and kx had been exchanged"""
    live = a[..., :27].reshape(*a.shape[:-1], 3, 3, 3).transpose(-3, -2).reshape(*a.shape[:-1], 27)
    return torch.cat([live, a[..., 27:]], -1)


# ------------------------------------------------------------------------------------------------------------ unfold / fold
@pytest.mark.parametrize("n,H,W", R.UNFOLD_CASES)
@pytest.mark.parametrize("shift,scale", [(R.SHIFT, R.SCALE), (R.SHIFT_WIDE, R.SCALE_WIDE)])
def test_unfold3_ref_is_f_unfold_reordered(n, H, W, shift, scale):
    img, tok = R.unfold_case(n, H, W)
    sh = torch.tensor(shift, dtype=F32).view(1, 3, 1, 1)
    inv = (torch.ones(3, dtype=F32) / torch.tensor(scale, dtype=F32)).view(1, 3, 1, 1)
    scaled = ((img - sh) * inv).to(BF).float()
    ref = R.unfold3_ref(img, H, W, shift, scale)
    assert ref.dtype == BF and ref.shape == (n, H + 2, W + 2, 32)
    assert torch.equal(ref[:, 1:-1, 1:-1, :27].float(), _unfold_torch(scaled))
    assert not bool(ref[..., 27:].any())
    assert not bool(ref[:, 0].any() or ref[:, -1].any() or ref[:, :, 0].any() or ref[:, :, -1].any())
    # the token source: the same tokens through PixelShuffle(16), then the image source (bf16 -> f32 is exact)
    assert torch.equal(R.unfold3_ref(tok, H, W, shift, scale), R.unfold3_ref(_shuffle(tok.float(), n, H, W), H, W, shift, scale))
    assert torch.equal(R.tokens_to_image(R.image_to_tokens(img), n, H, W), img)


@pytest.mark.parametrize("n,H,W", R.UNFOLD_CASES)
def test_fold3_ref_is_the_gradient_of_the_unfold(n, H, W):
    dA, dt0 = R.fold_case(n, H, W)
    junk = dA.clone()  # border rows are not part of the sum, whatever they hold
    junk[:, 0], junk[:, -1], junk[:, :, 0], junk[:, :, -1] = 3.0, -5.0, 7.0, 11.0
    ref, sumabs = R.fold3_ref(junk, dt0, H, W, R.SCALE_WIDE)
    img = torch.randn(n, 3, H, W, dtype=F64, requires_grad=True)
    sc = torch.tensor(R.SCALE_WIDE, dtype=F32).to(F64).view(1, 3, 1, 1)
    (_unfold_torch(img / sc) * dA[:, 1:-1, 1:-1, :27].to(F64)).sum().backward()
    want = dt0.to(F64) + _unshuffle(img.grad)
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((sumabs >= ref.abs() - 1e-12).all()) and bool((sumabs >= dt0.to(F64).abs()).all())
    assert torch.equal(R.fold3_ref(dA, dt0, H, W, R.SCALE_WIDE)[0], ref)


@pytest.mark.parametrize("n,H,W", R.UNFOLD_CASES)
def test_transposed_taps_miss_the_bars(n, H, W):
    """ky <-> kx in the unfold changes bits; in the fold it misses the bar of the fold test"""
    img, _ = R.unfold_case(n, H, W)
    ref = R.unfold3_ref(img, H, W, R.SHIFT, R.SCALE)
    assert not torch.equal(_swap_taps(ref), ref)
    dA, dt0 = R.fold_case(n, H, W)
    good, sumabs = R.fold3_ref(dA, dt0, H, W, R.SCALE)
    bad, _ = R.fold3_ref(_swap_taps(dA), dt0, H, W, R.SCALE)
    miss = (bad - good).abs() > R.fold_bar(good, sumabs)
    assert float(miss.double().mean()) > 0.1   # not an odd element: the 3 * H * W written columns, of 768 per 256 pixels


# ------------------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("NB,H,W,C", R.POOL_CASES)
def test_maxpool2_refs_are_autograd_of_max_pool2d(NB, H, W, C):
    Y, dP, tap = R.pool_case(NB, H, W, C)
    assert torch.equal(R.maxpool2_fwd_ref(Y), F.max_pool2d(Y, 2, 2))
    yr = Y.clone().requires_grad_(True)
    F.max_pool2d(yr, 2, 2).backward(dP)
    assert torch.equal(R.maxpool2_bwd_ref(Y, dP, None), yr.grad * (Y > 0))
    assert torch.equal(R.maxpool2_bwd_ref(Y, dP, tap), (yr.grad + tap).to(BF).float() * (Y > 0))
    got = R.maxpool2_bwd_ref(Y, dP, None)
    assert torch.equal(got[0, 0:8, 0, 0], dP[0, 0:8, 0, 0])                       # the four-way tie: the first pixel
    assert not bool(got[0, 0:8, 0:2, 0:2].flatten(1)[:, 1:].any())
    assert not bool(R.maxpool2_bwd_ref(Y, dP, tap)[0, 8:16, 0:2, 0:2].any())      # the all-zero window: masked, tap included
    assert torch.equal(got[0, 16:24, 0, 1], dP[0, 16:24, 0, 0]) and not bool(got[0, 16:24, 1, 0].any())


def _route_to_last(Y, dP, tap):
    """the wrong variant: the last maximum of the window (the right reference on the point-mirrored maps)"""
    fl = lambda t: None if t is None else t.flip(2, 3)
    return R.maxpool2_bwd_ref(fl(Y), fl(dP), fl(tap)).flip(2, 3)


@pytest.mark.parametrize("NB,H,W,C", R.POOL_CASES)
def test_routing_to_the_last_maximum_changes_bits(NB, H, W, C):
    Y, dP, tap = R.pool_case(NB, H, W, C)
    for t in (None, tap):
        assert not torch.equal(_route_to_last(Y, dP, t), R.maxpool2_bwd_ref(Y, dP, t))
    Y2 = Y.clone()  # without a tie the two agree: the variant is wrong only in what it is meant to be wrong in
    Y2[0, 0:24, 0:2, 0:2] = torch.tensor([[1.0, 2.0], [4.0, 3.0]])
    assert torch.equal(_route_to_last(Y2, dP, tap)[0, :24, 0:2, 0:2], R.maxpool2_bwd_ref(Y2, dP, tap)[0, :24, 0:2, 0:2])


# ------------------------------------------------------------------------------------------------------------ the head
def test_tap_ref_summed_over_the_five_taps_is_the_oracle(monkeypatch):
    from oracle import lpips_oracle as L
    sd = {k: v.to(F64) for k, v in L.make_state(3).items()}
    n, H, W = 2, 16, 32
    g = torch.Generator().manual_seed(0)
    feats = [[F.relu(torch.randn(n, c, H >> k, W >> k, generator=g, dtype=F64)).requires_grad_(i == 0) for k, c in enumerate(L.CHNS)]
             for i in range(2)]
    monkeypatch.setattr(L, "vgg_features", lambda sd_, x: feats[int(x.flatten()[0])])  # the oracle's head on given features
    shape = (n, 3, H, W)
    val = L.lpips(sd, torch.zeros(shape, dtype=F64) + sd["scaling_layer.shift"], torch.ones(shape, dtype=F64) * sd["scaling_layer.scale"]
                  + sd["scaling_layer.shift"])
    val.sum().backward()
    tot = torch.zeros(n, dtype=F64)
    for k in range(5):
        f0, f1 = feats[0][k], feats[1][k]
        h, w = f0.shape[2:]
        v, df0 = R.tap_ref(f0.detach(), f1, sd[f"lin{k}.model.1.weight"].flatten(), 1.0 / (h * w), h, w)
        want = f0.grad * (f0.detach() > 0)
        assert float((df0 - want).abs().max()) <= 1e-9 * float(want.abs().max())
        tot += v
    assert float((tot - val.detach().flatten()).abs().max()) <= 1e-9 * float(val.detach().abs().max())


@pytest.mark.parametrize("C,n,H,W", R.TAP_CASES)
def test_tap_ref_special_pixels(C, n, H, W):
    f0, f1, w = R.tap_case(C, n, H, W)
    val, df0 = R.tap_ref(f0, f1, w, 1.0, H, W)
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(df0).all())
    assert not bool(df0[0, :, 0, 0].any())            # |f0| = 0
    same = R.tap_identical(n, H, W)
    if same is not None:
        assert float(val[same]) == 0.0 and not bool(df0[same].any())     # f0 == f1
    assert bool((val[:n if same is None else same] > 0).all())
    e = R.tap_pixel_error_f32(f0, f1, w)
    assert 0 < e < 2e-6, e                            # fp32 torch alone, per pixel: the unit of the bar on val


@pytest.mark.parametrize("C,n,H,W", R.TAP_CASES)
def test_a_head_without_the_relu_mask_misses_the_bar(C, n, H, W):
    f0, f1, w = R.tap_case(C, n, H, W)
    for gs in R.GSCALES:
        _, good = R.tap_ref(f0, f1, w, gs, H, W)
        _, bad = R.tap_ref(f0, f1, w, gs, H, W, relu_mask=False)
        miss = (bad - good).abs() > R.tap_df_bar(good)
        assert float(miss.double().mean()) > 0.05, float(miss.double().mean())  # about half the elements are zero; a live f1 there shows


@pytest.mark.parametrize("C,n,H,W", R.TAP_CASES)
def test_a_head_that_skips_the_last_column_misses_the_bars(C, n, H, W):
    f0, f1, w = R.tap_case(C, n, H, W)
    val, df0 = R.tap_ref(f0, f1, w, 1.0, H, W)
    v_bad, d_bad = R.tap_ref(f0[..., :W - 1], f1[..., :W - 1], w, 1.0, H, W)
    d_bad = F.pad(d_bad, (0, 1))
    same = R.tap_identical(n, H, W)
    live = slice(0, n if same is None else same)      # the image with f0 == f1 has nothing to lose
    bar = R.VAL_FACTOR * R.tap_pixel_error_f32(f0, f1, w) * val
    assert bool(((v_bad - val).abs()[live] > bar[live]).all()), (v_bad, val, bar)
    assert bool(((d_bad - df0).abs() > R.tap_df_bar(df0))[live, :, :, W - 1].any())


# ------------------------------------------------------------------------------------------------------------ convolutions
def test_conv_refs_agree_with_each_other():
    g = torch.Generator().manual_seed(0)
    x = R.bf_round(torch.randn(2, 64, 4, 6, generator=g))
    w = R.bf_round(torch.randn(128, 64, 3, 3, generator=g) * 0.05)
    b = torch.randn(128, generator=g)
    # the forward on the unfolded rows is the taps = 1 form
    cols = F.unfold(x.to(F64), 3, padding=1).view(2, 64 * 9, 4, 6)
    assert torch.allclose(R.rows_ref(cols, w.reshape(128, 64 * 9), b), R.conv3x3_fwd_ref(x, w, b), rtol=1e-12, atol=1e-12)
    # the input gradient is the gradient
    xr = x.to(F64).requires_grad_(True)
    dy = R.bf_round(torch.randn(2, 128, 4, 6, generator=g))
    (F.conv2d(xr, w.to(F64), padding=1) * dy.to(F64)).sum().backward()
    assert torch.allclose(R.conv3x3_dgrad_ref(dy, w), xr.grad, rtol=1e-12, atol=1e-12)
    m = torch.randn(2, 64, 4, 6, generator=g)
    assert torch.equal(R.conv3x3_dgrad_ref(dy, w, m), R.conv3x3_dgrad_ref(dy, w) * (m > 0))
    # and equals the forward kernel's form on the flipped, transposed weights (what LPIPS._prep hands the kernel)
    wd = w.flip(2, 3).permute(1, 0, 2, 3)
    assert torch.allclose(F.conv2d(dy.to(F64), wd.to(F64), padding=1), xr.grad, rtol=1e-12, atol=1e-12)
