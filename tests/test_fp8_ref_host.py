"""tests/fp8_ref.py proved without a GPU: the e4m3 codec against torch's CPU float8_e4m3fn on every code, every tie and its
neighbours; every GEMM case of tests/test_fp8_kernels_gpu.py shown to be independent of the order of summation (so its comparison
can be an equality of bits); every wrong variant of a kernel shown to break that equality at every listed shape; the SwiGLU bar shown
to hold for the stated rounding points and to reject a wrong quad order and a wrong hidden-column map."""
import numpy as np
import pytest
import torch

import fp8_ref as R

F8 = torch.float8_e4m3fn


def torch_encode(x32, clamp=True):
    t = torch.from_numpy(np.ascontiguousarray(x32, np.float32))
    if clamp:
        t = t.clamp(-448, 448)
    return t.to(F8).view(torch.uint8).numpy()


def test_decode_table_is_torch_e4m3fn_on_all_256_codes():
    ours = R.DECODE
    theirs = torch.arange(256, dtype=torch.uint8).view(F8).to(torch.float64).numpy()
    assert np.array_equal(np.isnan(ours), np.isnan(theirs)) and [int(c) for c in np.flatnonzero(np.isnan(ours))] == list(R.NAN_CODES)
    assert np.array_equal(ours[~np.isnan(ours)], theirs[~np.isnan(theirs)])
    assert np.array_equal(np.signbit(ours), np.signbit(theirs))          # code 0x80 is -0
    assert not np.isinf(ours).any() and np.nanmax(ours) == 448 and ours[1] == 2.0 ** -9 and ours[8] == 2.0 ** -6
    assert np.array_equal(ours[:8], np.arange(8) * 2.0 ** -9)            # subnormals: multiples of 2^-9


def test_encoder_round_trips_every_code():
    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.canon(R.encode(R.DECODE)), R.canon(codes))


def test_encoder_matches_torch_on_the_code_point_table():
    t = R.code_point_table()
    assert len(t) % 8 == 0 and np.isnan(t).sum() == 2 and np.isinf(t).sum() == 2
    assert np.array_equal(R.canon(R.encode(t)), R.canon(torch_encode(t)))
    tb = torch.from_numpy(t).to(torch.bfloat16).float().numpy()           # the same table as a bf16 input sees it
    assert np.array_equal(R.canon(R.encode(tb)), R.canon(torch_encode(tb)))
    mid = R.midpoints()
    lo, hi = R.encode(R.f32_bits_ulp(mid, -1)), R.encode(R.f32_bits_ulp(mid, 1))
    tie = R.encode(mid)
    assert (np.abs(hi.astype(int) - lo.astype(int)) == 1).all()            # a midpoint separates two neighbouring codes ...
    assert ((tie == lo) | (tie == hi)).all() and ((tie & 1) == 0).all()      # ... and itself goes to the even one


def test_encoder_hand_values():
    enc = lambda v: int(R.encode(np.array([v], np.float32))[0])
    dec = lambda v: R.DECODE[enc(v)]
    assert dec(17.0) == 16 and dec(19.0) == 20 and dec(2.0 ** -10) == 0 and dec(3 * 2.0 ** -10) == 2.0 ** -8
    assert dec(464.0) == 448 and dec(465.0) == 448 and dec(1e30) == 448 and dec(-np.inf) == -448 and enc(np.inf) == 0x7E
    assert enc(0.0) == 0 and enc(-0.0) == 0x80 and enc(1e-40) == 0 and enc(-1e-40) == 0x80 and enc(np.nan) == 0x7F
    # what this torch build does on the CPU, which the comparisons above lean on: ties to even, and NaN past 464 without the clamp
    assert [int(c) for c in torch_encode(np.array([17.0, 19.0, 2.0 ** -10, 464.0], np.float32), clamp=False)] == [enc(16.0), enc(20.0), 0, 0x7E]
    assert int(torch_encode(np.array([465.0], np.float32), clamp=False)[0]) & 0x7F == 0x7F


def test_encoder_matches_torch_on_a_million_random_floats():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(1_000_000) * np.exp2(rng.integers(-14, 10, 1_000_000))).astype(np.float32)
    assert np.array_equal(R.encode(x), torch_encode(x))


@pytest.mark.parametrize("scale", R.QUANT_SCALES)
def test_quantize_ref_is_the_float32_product_then_torch_cast(scale):
    x = R.quant_input(scale)
    ref = R.quantize_ref(x, scale)
    t = (torch.from_numpy(x) * torch.tensor(scale, dtype=torch.float32)).clamp(-448, 448).to(F8).view(torch.uint8).numpy()
    assert np.array_equal(R.canon(ref), R.canon(t))
    if scale != 1.7:  # the power-of-two scales put x * scale back on the table: every tie is hit again
        with np.errstate(invalid="ignore", over="ignore"):
            back = x * np.float32(scale)
        tab = R.code_point_table()
        keep = np.isfinite(tab) & ((np.abs(tab) >= 2.0 ** -120) | (tab == 0)) & (np.abs(tab) < 1e37)  # (but for the ends of the f32 range)
        assert np.array_equal(back[keep], tab[keep])
    assert np.array_equal(np.flatnonzero(np.isnan(x)), np.flatnonzero((ref & 0x7F) == 0x7F))  # NaN in, NaN code out -- nowhere else
    d = R.dequantize_ref(np.arange(256, dtype=np.uint8), 1.0)
    assert np.isnan(d[list(R.NAN_CODES)]).all() and np.array_equal(d[:0x7F].astype(np.float64), R.DECODE[:0x7F])


# ------------------------------------------------------------------------------------------------------------ exact-sum GEMMs
def test_exact_values_are_the_49_multiples_of_an_eighth():
    v = R.EXACT_VALUES
    assert len(v) == 49 and v.min() == -4 and v.max() == 4 and 0.0 in v
    assert np.array_equal(v * 8, np.rint(v * 8)) and np.array_equal(R.DECODE[R.encode(v)], v)


@pytest.fixture(scope="module", params=R.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def gemm_case(request):
    M, N, K, lda, ldb, ldc = request.param
    return R.exact_case(M, N, K, lda, ldb)


def test_gemm_case_is_independent_of_the_order_of_summation(gemm_case):
    c = gemm_case
    a, b, K = c["a"], c["b"], c["K"]
    assert K <= 16384 and K % 16 == 0
    assert np.array_equal(R.DECODE[c["a8"][:, :K]], a) and np.array_equal(R.DECODE[c["b8"][:, :K]], b)
    assert (c["a8"][:, K:] == 0x7F).all() and (c["b8"][:, K:] == 0x7F).all()                  # the padding is NaN codes
    assert np.array_equal(c["bias"] * 64, np.rint(c["bias"] * 64)) and np.abs(c["bias"]).max() <= 8
    assert np.array_equal(c["resid"] * 64, np.rint(c["resid"] * 64)) and np.abs(c["resid"]).max() <= 64
    acc = a @ b.T
    assert acc[-1, -1] == 16.0 * K == np.abs(acc).max()                                       # the all-4 row meets the all-4 column
    assert 16.0 * K * 64 <= 2 ** 24                                                           # every partial sum: 24 bits of 2^-6
    # float32 matmuls in two K orders give the bits of the float64 result
    perm = np.random.default_rng(1).permutation(K)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    for order in (np.arange(K), perm, np.arange(K)[::-1]):
        got = np.ascontiguousarray(a32[:, order]) @ np.ascontiguousarray(b32[:, order]).T
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), acc)
    # acc * alpha + bias (+ resid): representable in float32, whichever way it is associated, fused or not
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    step1 = acc * R.ALPHA
    assert np.array_equal(f32(step1), step1)
    for bias, resid in ((c["bias"], c["resid"]), (c["bias"], None), (None, None)):
        full = R.gemm_ref(a, b, R.ALPHA, bias, resid)
        assert np.array_equal(f32(full), full)
        if bias is not None:
            assert np.array_equal(f32(step1 + bias), step1 + bias)
            if resid is not None:
                assert np.array_equal(f32(step1 + resid), step1 + resid) and np.array_equal(f32(bias + resid), bias + resid)
    # the bf16 epilogue rounds an exact value once; ties occur
    want = R.expected(c, "bf16", True, False)
    assert want.dtype == torch.bfloat16 and torch.isfinite(want.float()).all()


def test_bf16_epilogue_cases_hold_round_to_even_ties():
    c = R.exact_case(*R.GEMM_SHAPES[4][:5])
    x = R.gemm_ref(c["a"], c["b"], R.ALPHA, c["bias"])
    b = R.bf16_round(x)
    m, _ = np.frexp(x)
    ties = np.abs(m * 256 - np.rint(m * 256)) == 0.5
    assert ties.sum() > 100
    assert np.array_equal(R.as_bf16(x).to(torch.float64).numpy(), b)      # the own bf16 rounding is torch's


def test_every_wrong_gemm_variant_breaks_bit_equality(gemm_case):
    c = gemm_case
    good = R.as_f32(R.gemm_ref(c["a"], c["b"], R.ALPHA, c["bias"], c["resid"]))
    assert torch.equal(R.bits(good), R.bits(R.expected(c, "f32", True, True)))
    variants = R.wrong_variants(c)
    need = {"last 16-byte K piece dropped", "alpha applied after the bias", "table decoded with bias 8 (fnuz)"}
    if c["M"] >= 2:
        need.add("last row taken from its neighbour")
    if c["N"] >= 8:
        need.add("last 4-column group taken from its neighbour")
    assert set(variants) == need
    for name, v in variants.items():
        differ = int((R.bits(R.as_f32(v)) != R.bits(good)).sum())
        assert differ > 0, (name, c["M"], c["N"], c["K"])
        if "row" not in name and "column" not in name:
            assert int((R.bits(R.as_bf16(v)) != R.bits(R.as_bf16(good.double().numpy()))).sum()) > 0, name


# ------------------------------------------------------------------------------------------------------------ code-pair table
@pytest.mark.parametrize("kind", ["identity", "37i"])
def test_code_pair_table_is_a_single_exact_product_per_element(kind):
    a8, b8 = R.pair_case(kind)
    want = R.pair_expected()
    p = R.pair_perm(kind)
    assert sorted(p) == list(range(256))                                    # every code sits in its own k position
    assert not np.isin(a8, R.NAN_CODES).any() and not np.isin(b8, R.NAN_CODES).any()
    assert ((a8 != 0).sum(1) <= 1).all() and (b8 == b8[:, :1]).all()
    a, b = R.DECODE[a8], R.DECODE[b8]
    for lhs, rhs, w in ((a, b, want), (b, a, want.T)):                       # and with the operand slots swapped
        got = lhs.astype(np.float32) @ rhs.astype(np.float32).T
        assert np.array_equal(got, w.numpy())                                # values (the sign of a zero: pair_expected's note)
    nz = want[want != 0].abs()
    assert float(nz.min()) == 2.0 ** -18 and float(nz.max()) == 448.0 * 448.0 == 200704.0
    m, _ = np.frexp(want.numpy().astype(np.float64))
    assert np.array_equal(m * 256, np.rint(m * 256))                         # at most 8 significant bits
    assert (R.bits(want)[want == 0] == 0).all()                              # +0
    fin = [c for c in range(256) if c not in R.NAN_CODES]
    assert np.array_equal(want.numpy()[np.ix_(fin, fin)].astype(np.float64), np.outer(R.DECODE[fin], R.DECODE[fin]) + 0.0)
    a8n, _ = R.pair_case(kind, nan_row=5)
    assert (a8n != a8).sum() == 1 and a8n[5, (p[5] + 101) % 256] == 0x7F


# ------------------------------------------------------------------------------------------------------------ SwiGLU epilogue
@pytest.mark.parametrize("shape", R.SWIGLU_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_swiglu_reference_and_bar(shape):
    c = R.swiglu_case(*shape)
    M, N = c["M"], c["N"]
    assert N % 16 == 0 and np.array_equal(c["bias"] * 64, np.rint(c["bias"] * 64))
    x = R.gemm_ref(c["a"], c["b"], R.ALPHA, c["bias"])
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)        # x1, x2 exact in float32: their bf16 rounding is exact bits
    x1 = x.reshape(M, N // 16, 2, 8)[:, :, 0, :]
    assert np.abs(x1).max() <= R.SWIGLU_X1_MAX and np.abs(x1).max() > 6
    xb, hid64, hid_rp = R.swiglu_ref(c)
    assert np.array_equal(R.as_bf16(x).to(torch.float64).numpy(), xb)
    bar = R.swiglu_bar(hid64)
    r = R.ratio(hid_rp, hid64, bar)
    assert r <= (2.0 ** -7 + 2.0 ** -16) / (2.0 ** -7 + 2.0 ** -14)          # the stated rounding points: two roundings, inside the bar
    # wrong variants at these inputs
    assert R.ratio(R.swiglu_ref(c, swap=True)[2], hid64, bar) > 100          # the w1 / w2 quads swapped
    assert R.ratio(R.swiglu_ref(c, group_shift=1)[2], hid64, bar) > 100      # the hidden-column map off by one 8-column group
    # silu left unrounded is ONE rounding less: it cannot leave a bar of two roundings around the float64 value (<= 2^-8 |ref|), and the
    # device's expf keeps a bit-exact comparison with hid_rp out of reach.  What the reference does show: it is a different bf16 array.
    one = R.swiglu_ref(c, round_silu=False)[2]
    assert R.ratio(one, hid64, bar) <= 0.5
    assert (one != hid_rp).mean() > 0.02


def test_rope_case_rows():
    assert R.rope_rows() == 1470 and 2 * R.ROPE_D % 128 == 0 and R.ROPE_D == 64 * R.ROPE_HEADS
