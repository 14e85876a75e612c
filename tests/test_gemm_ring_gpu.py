"""The ring GEMM kernel (vtp_amd/csrc/gemm.hip gemm_nt_kernel, NT) taken configuration by configuration: every tile configuration the
dispatch can name (0, 3, 4, 5, 7, 21) is FORCED and run through every epilogue of vtp_amd/csrc/gemm_common.h at shapes derived from
its own tile -- one partial tile with one partial k-tile, one row / four columns over a tile, tails everywhere, exact multiples, and
persistent launches (more tiles than resident workgroups) with 1, 2, 3 and 4 k-tiles per tile, i.e. below, at and above the depth of
the LDS ring whose staging cursor runs ahead across tile boundaries -- and with every value of the store-route flag.

Reference: the same operation in fp64 on the bf16-rounded inputs, on the device; where the kernel rounds an intermediate to bf16
(pre-activations, dh, the RoPE products) the reference rounds the same intermediate.  Tolerances are those of
test_kernels_gpu.check: 1e-3 max|ref| + 2^-7 |ref| for bf16 outputs, scale 1e-5 for fp32 outputs, 2e-5 for split-K sums.  Outputs
computed FROM a bf16-rounded intermediate carry the scale the suite already gives them, because the kernel's fp32 and the reference's
fp64 accumulation now and then round that intermediate to neighbouring bf16 values and the whole ulp (2^-7 relative) travels on:
4e-3 for the SwiGLU hidden, GELU and rotated (RoPE: two such intermediates, each weighted by |cos|, |sin| <= 1) outputs, 6e-3 for the
SwiGLU backward (test_swiglu_gelu_bwd_adamw_ema_assemble: dh -> bf16(dh x2) -> bf16(. silu'), two roundings downstream of the ulp).

Guard bands: every output is allocated with ldc = N + 16 and 8 rows below the last one, prefilled (NaN where the launch overwrites,
finite values where it accumulates -- a NaN guard read and written back would keep its bits), and every element the launch must not
touch is compared BIT FOR BIT with its value before the launch; rows a row map does not name are such elements."""
import math

import pytest
import torch

from test_kernels_gpu import DEV, bf, check, interleave, ops  # noqa: F401  (same helpers / tolerance)

pytestmark = pytest.mark.gpu

# cfg id -> ((BM, BN) of the bf16 epilogue, (BM, BN) of every other epilogue, STAGES): the `launch_gemm` switch of csrc/gemm.hip
# (cfg 4 is 256 x 128 for EPI_BF16 -- which also carries the fused RoPE and SwiGLU backward -- and 256 x 256 otherwise; 21 = 5 with
# the software-pipelined k-tile body)
RING = {
    0: ((128, 128), (128, 128), 2),
    3: ((256, 128), (256, 128), 3),
    4: ((256, 128), (256, 256), 2),
    5: ((128, 128), (128, 128), 2),
    7: ((128, 64), (128, 64), 3),
    21: ((128, 128), (128, 128), 2),
}
CFGS = sorted(RING)
LDS_PER_CU = 160 * 1024  # CDNA4
GUARD_ROWS, GUARD_COLS = 8, 16
FINITE_GUARD = -1234.5   # guard value of accumulated outputs
HW = 36                  # row maps: groups of 36 rows behind one skipped row (a [B, 1 + 36, D] token stream)
SPLIT_K = 328            # three slices of 128: the last one holds 72 = one k-tile and 8 elements


@pytest.fixture(autouse=True)
def _restore_tuning():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vtp_amd import _lib
    lib = _lib.load()
    yield
    lib.vtp_set_gemm_tuning(-1, 3)  # process-global


def _force(cfg, flags=3):
    from vtp_amd import _lib
    _lib.check(_lib.load().vtp_set_gemm_tuning(cfg, flags), "vtp_set_gemm_tuning")


def _tile(cfg, bf16_epi):
    return RING[cfg][0 if bf16_epi else 1]


def _shape(cfg, case, bf16_epi):
    BM, BN = _tile(cfg, bf16_epi)
    if case == 1:  # one partial tile, one partial k-tile; N % 8 == 0, N % 16 != 0
        return BM - 27, BN - 24, 40
    if case == 2:  # one row and four columns over (N % 8 != 0: bf16 stores directly); the second k-tile holds 8 elements
        return BM + 1, BN + 4, 72
    if case == 3:  # several tiles, tails everywhere
        return 3 * BM - 1, 2 * BN + 8, 216
    return 2 * BM, 2 * BN, 128


def _persistent_shape(cfg, bf16_epi):
    """smallest M = BM r + 5, N = BN c + 8 (fewest tile rows + tile columns, then fewest tiles, then fewest rows) whose tile count
    exceeds -- and is no multiple of -- an upper bound on the resident workgroups: CUs x floor(LDS per CU / LDS of launch_cfg)"""
    BM, BN = _tile(cfg, bf16_epi)
    stages = RING[cfg][2]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bound = cus * (LDS_PER_CU // (stages * (BM + BN) * 128))
    best = None
    for tm in range(2, 200):
        for tn in range(2, 200):
            t = tm * tn
            if t > bound and t % bound != 0:
                key = (tm + tn, t, tm)
                if best is None or key < best[0]:
                    best = (key, tm, tn)
    _, tm, tn = best
    return BM * (tm - 1) + 5, BN * (tn - 1) + 8, bound


def _assert_persistent(cfg, bf16_epi, M, N, bound):
    BM, BN = _tile(cfg, bf16_epi)
    ntiles = -(-M // BM) * -(-N // BN)
    assert ntiles > bound and ntiles % bound != 0, f"cfg {cfg}: {ntiles} tiles of {BM}x{BN} against {bound} resident workgroups"


def _up(n, q):
    return -(-n // q) * q


# ------------------------------------------------------------------------------------------------------------ inputs / guard bands
def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _act(g, M, K):
    """bf16 activations with a per-row ramp (a transposed or shifted tile shows)"""
    return bf(torch.randn(M, K, device=DEV, generator=g) + torch.linspace(-1, 1, M, device=DEV)[:, None])


def _wgt(g, N, K):
    return bf(torch.randn(N, K, device=DEV, generator=g) * K ** -0.5)  # outputs O(1)


def _guarded(rows, cols, dtype, inside=float("nan"), guard=float("nan")):
    """[rows + 8, cols + 16] buffer: `guard` everywhere, `inside` (scalar or tensor) in [0, rows) x [0, cols)"""
    buf = torch.full((rows + GUARD_ROWS, cols + GUARD_COLS), guard, dtype=dtype, device=DEV)
    buf[:rows, :cols] = inside
    return buf


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _assert_untouched(buf, before, rows, cols, name):
    """every element outside rows x [0, cols) keeps its bits (rows: a count = the first rows, or the tensor of written row indices)"""
    sel = torch.zeros(buf.shape[0], dtype=torch.bool, device=DEV)
    if isinstance(rows, int):
        sel[:rows] = True
    else:
        sel[rows] = True
    written = sel[:, None] & (torch.arange(buf.shape[1], device=DEV) < cols)[None, :]
    changed = (_bits(buf) != _bits(before)) & ~written
    n = int(changed.sum())
    assert n == 0, f"{name}: {n} elements outside the output were written, first at {changed.nonzero()[0].tolist()} of {list(buf.shape)}"


def _row_map(M):
    m = torch.arange(M, device=DEV)
    return m + (m // HW + 1)  # remap_row(m, HW, 1)


def _bf64(x):
    return bf(x).double()


# ------------------------------------------------------------------------------------------------------------ the epilogues
def _bias_bf16(M, N, K, seed, tag, alpha=1.0):
    o = ops()
    g = _gen(seed)
    a, b = _act(g, M, K), _wgt(g, N, K)
    bias = torch.randn(N, device=DEV, generator=g)
    c = _guarded(M, N, torch.bfloat16)
    before = c.clone()
    o.gemm_nt(a, b, c, M=M, N=N, K=K, bias=bias, epi=o.EPI_BF16, alpha=alpha)
    _assert_untouched(c, before, M, N, tag)
    check(c[:M, :N], alpha * (a.double() @ b.double().T) + bias.double(), tag)


def _bias_bf16_alpha(M, N, K, seed, tag):
    _bias_bf16(M, N, K, seed, tag, alpha=0.37)


def _f32_resid(M, N, K, seed, tag):
    """out = resid + gamma (acc + bias), resid aliased to C"""
    o = ops()
    g = _gen(seed)
    a, b = _act(g, M, K), _wgt(g, N, K)
    bias = torch.randn(N, device=DEV, generator=g)
    gamma = torch.rand(N, device=DEV, generator=g) + 0.5
    x = _guarded(M, N, torch.float32, torch.randn(M, N, device=DEV, generator=g), FINITE_GUARD)
    before = x.clone()
    o.gemm_nt(a, b, x, M=M, N=N, K=K, bias=bias, gamma=gamma, resid=x, epi=o.EPI_F32)
    _assert_untouched(x, before, M, N, tag)
    ref = before[:M, :N].double() + (a.double() @ b.double().T + bias.double()) * gamma.double()
    check(x[:M, :N], ref, tag, bf16_out=False, scale=1e-5)


def _f32_c_remap(M, N, K, seed, tag):
    """only the patch rows of a token stream are written (in place: resid = C); the skipped rows are guard rows"""
    o = ops()
    g = _gen(seed)
    a, b = _act(g, M, K), _wgt(g, N, K)
    bias = torch.randn(N, device=DEV, generator=g)
    rows = _row_map(M)
    R = int(rows[-1]) + 1
    x = _guarded(R, N, torch.float32, torch.randn(R, N, device=DEV, generator=g), FINITE_GUARD)
    before = x.clone()
    o.gemm_nt(a, b, x, M=M, N=N, K=K, bias=bias, resid=x, epi=o.EPI_F32, c_remap=(HW, 1))
    _assert_untouched(x, before, rows, N, tag)
    ref = before[rows, :N].double() + a.double() @ b.double().T + bias.double()
    check(x[rows, :N], ref, tag, bf16_out=False, scale=1e-5)


def _f32_a_remap(M, N, K, seed, tag):
    """only the patch rows of A are read: the rows the map skips hold NaN"""
    o = ops()
    g = _gen(seed)
    b = _wgt(g, N, K)
    rows = _row_map(M)
    full = torch.full((int(rows[-1]) + 1, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    full[rows] = _act(g, M, K)
    c = _guarded(M, N, torch.float32)
    before = c.clone()
    o.gemm_nt(full, b, c, M=M, N=N, K=K, epi=o.EPI_F32, a_remap=(HW, 1))
    _assert_untouched(c, before, M, N, tag)
    check(c[:M, :N], full[rows].double() @ b.double().T, tag, bf16_out=False, scale=1e-5)


def _f32_strided(M, N, K, seed, tag):
    """lda, ldb > K with NaN behind the K columns: a k-tail chunk that is read instead of zero-filled poisons the row"""
    o = ops()
    g = _gen(seed)
    abuf = torch.full((M, K + 24), float("nan"), dtype=torch.bfloat16, device=DEV)
    bbuf = torch.full((N, K + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    abuf[:, :K] = _act(g, M, K)
    bbuf[:, :K] = _wgt(g, N, K)
    c = _guarded(M, N, torch.float32)
    before = c.clone()
    o.gemm_nt(abuf, bbuf, c, M=M, N=N, K=K, lda=K + 24, ldb=K + 8, epi=o.EPI_F32)
    _assert_untouched(c, before, M, N, tag)
    check(c[:M, :N], abuf[:, :K].double() @ bbuf[:, :K].double().T, tag, bf16_out=False, scale=1e-5)


def _swiglu(M, N, K, seed, tag):
    o = ops()
    N = _up(N, 16)
    H = N // 2
    g = _gen(seed)
    x = _act(g, M, K)
    w1, w2 = _wgt(g, H, K), _wgt(g, H, K)
    b1 = torch.randn(H, device=DEV, generator=g) * 0.1
    b2 = torch.randn(H, device=DEV, generator=g) * 0.1
    w12, b12 = interleave(w1, w2).contiguous(), interleave(b1, b2).contiguous()
    hid = _guarded(M, H, torch.bfloat16)
    x12 = _guarded(M, N, torch.bfloat16)
    hid0, x120 = hid.clone(), x12.clone()
    o.gemm_nt(x, w12, hid, M=M, N=N, K=K, c2=x12, bias=b12, epi=o.EPI_SWIGLU)
    _assert_untouched(hid, hid0, M, H, tag + " hidden")
    _assert_untouched(x12, x120, M, N, tag + " x12")
    x1 = _bf64(x.double() @ w1.double().T + b1.double())
    x2 = _bf64(x.double() @ w2.double().T + b2.double())
    check(hid[:M, :H], _bf64(x1 * torch.sigmoid(x1)) * x2, tag + " hidden", scale=4e-3)  # one bf16 ulp of x1 / x2 propagates
    check(x12[:M, :N], interleave(x1.T.contiguous(), x2.T.contiguous()).T, tag + " x12")


def _gelu(M, N, K, seed, tag, quick=False):
    o = ops()
    g = _gen(seed)
    a, b = _act(g, M, K), _wgt(g, N, K)
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    out = _guarded(M, N, torch.bfloat16)
    pre = _guarded(M, N, torch.bfloat16)
    out0, pre0 = out.clone(), pre.clone()
    o.gemm_nt(a, b, out, M=M, N=N, K=K, c2=pre, bias=bias, epi=o.EPI_QUICK_GELU if quick else o.EPI_GELU)
    _assert_untouched(out, out0, M, N, tag + " out")
    _assert_untouched(pre, pre0, M, N, tag + " pre")
    p = _bf64(a.double() @ b.double().T + bias.double())
    check(pre[:M, :N], p, tag + " pre")
    act = p * torch.sigmoid(1.702 * p) if quick else 0.5 * p * (1 + torch.erf(p * math.sqrt(0.5)))
    check(out[:M, :N], act, tag + " out", scale=4e-3)


def _quick_gelu(M, N, K, seed, tag):
    _gelu(M, N, K, seed, tag, quick=True)


def _atomic(M, N, K, seed, tag):
    o = ops()
    K = SPLIT_K
    g = _gen(seed)
    a, b = _act(g, M, K), _wgt(g, N, K)
    c = _guarded(M, N, torch.float32, 1.0, FINITE_GUARD)
    before = c.clone()
    assert o.gemm_splits(K, 3) == 3
    o.gemm_nt(a, b, c, M=M, N=N, K=K, epi=o.EPI_F32_ATOMIC, splits=3)
    _assert_untouched(c, before, M, N, tag)
    check(c[:M, :N], 1.0 + a.double() @ b.double().T, tag, bf16_out=False, scale=2e-5)


def _slab(M, N, K, seed, tag):
    o = ops()
    K = SPLIT_K
    g = _gen(seed)
    a, b = _act(g, M, K), _wgt(g, N, K)
    S = o.gemm_splits(K, 3)
    assert S == 3
    R, ld = M + GUARD_ROWS, N + GUARD_COLS
    slab = torch.stack([_guarded(M, N, torch.float32) for _ in range(S)])
    before = slab.clone()
    o.gemm_nt(a, b, slab, M=M, N=N, K=K, ldc=ld, ldc2=R * ld // 4, epi=o.EPI_F32_SLAB, splits=S)
    for s in range(S):
        _assert_untouched(slab[s], before[s], M, N, f"{tag} slab {s}")
    dst = torch.ones(R, ld, device=DEV)
    o.reduce_slabs(slab, R * ld, S, dst, R * ld, accumulate=True)
    check(dst[:M, :N], 1.0 + a.double() @ b.double().T, tag, bf16_out=False, scale=2e-5)


def _qkv_rope(M, N, K, seed, tag):
    """apply_rope in the bf16 epilogue: N = 3 D with D a multiple of 128, rows with rope_pos = -1 (cls) mixed in"""
    o = ops()
    N = _up(N, 384)
    D, P = N // 3, 50
    g = _gen(seed)
    a, w = _act(g, M, K), _wgt(g, N, K)
    bias = torch.randn(N, device=DEV, generator=g)
    ang = torch.rand(P, 32, device=DEV, generator=g) * 6.2831853
    cos, sin = bf(torch.cos(ang).repeat(1, 2)).contiguous(), bf(torch.sin(ang).repeat(1, 2)).contiguous()
    pos = torch.randint(0, P, (M,), device=DEV, generator=g).to(torch.int32)
    pos[::5] = -1
    c = _guarded(M, N, torch.bfloat16)
    before = c.clone()
    o.gemm_qkv_rope(a, w, bias, c, M, N, K, pos, sin, cos, 2 * D)
    _assert_untouched(c, before, M, N, tag)
    pre = _bf64(a.double() @ w.double().T + bias.double())
    x = pre[:, :2 * D].reshape(M, -1, 64)                      # q and k heads
    rot = torch.cat([-x[..., 32:], x[..., :32]], dim=-1)        # rot_half
    pp = pos.long().clamp(min=0)
    t1 = _bf64(x * cos[pp].double()[:, None, :])
    t2 = _bf64(rot * sin[pp].double()[:, None, :])
    ref = pre.clone()
    ref[:, :2 * D] = torch.where((pos >= 0)[:, None, None], t1 + t2, x).reshape(M, 2 * D)
    rotated = (pos >= 0)[:, None] & (torch.arange(N, device=DEV) < 2 * D)[None, :]
    out = c[:M, :N]
    check(out[rotated], ref[rotated], tag + " rotated", scale=4e-3)
    check(out[~rotated], ref[~rotated], tag + " unrotated (v, cls rows)")


def _dgrad_swiglu(M, N, K, seed, tag):
    """w3 dgrad with the SwiGLU backward in its epilogue: dx12 [M, 2H] from dh = dy W3 (never stored) and the saved x12"""
    o = ops()
    H = _up(N, 8)
    g = _gen(seed)
    dy, wT = _act(g, M, K), _wgt(g, H, K)
    x12 = bf(torch.randn(M, 2 * H, device=DEV, generator=g))
    c = _guarded(M, 2 * H, torch.bfloat16)
    before = c.clone()
    o.gemm_dgrad_swiglu(dy, wT, x12, c, M, H, K)
    _assert_untouched(c, before, M, 2 * H, tag)
    dh = _bf64(dy.double() @ wT.double().T)
    xg = x12.double().view(M, H // 8, 2, 8)                     # 16-column groups: 8 of x1 | 8 of x2
    x1, x2 = xg[:, :, 0].reshape(M, H), xg[:, :, 1].reshape(M, H)
    sg = torch.sigmoid(x1)
    d1 = _bf64(dh * x2) * (sg * (1 + x1 * (1 - sg)))            # swiglu_bwd8: gs = bf16(dh x2), times silu'(x1)
    d2 = dh * _bf64(x1 * sg)                                    # dh times bf16(silu(x1))
    ref = torch.stack([d1.view(M, H // 8, 8), d2.view(M, H // 8, 8)], dim=2).reshape(M, 2 * H)
    check(c[:M, :2 * H], ref, tag, scale=6e-3)


# (runner, takes the bf16-epilogue tile of cfg 4)
EPILOGUES = {
    "bias_bf16": (_bias_bf16, True),
    "bias_bf16_alpha": (_bias_bf16_alpha, True),
    "f32_resid_gamma_inplace": (_f32_resid, False),
    "f32_c_remap": (_f32_c_remap, False),
    "f32_a_remap": (_f32_a_remap, False),
    "f32_strided_lda": (_f32_strided, False),
    "swiglu": (_swiglu, False),
    "gelu": (_gelu, False),
    "quick_gelu": (_quick_gelu, False),
    "atomic_splitk": (_atomic, False),
    "slab_splitk": (_slab, False),
    "qkv_rope": (_qkv_rope, True),
    "dgrad_swiglu": (_dgrad_swiglu, True),
}
# the three routes that reuse a ring slot as store staging while the next tile's DMA is in flight
STAGED = ["bias_bf16", "f32_resid_gamma_inplace", "swiglu"]


def _seed(cfg, case, epi):
    return cfg * 10000 + case * 100 + sorted(EPILOGUES).index(epi)


# ------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("case", [1, 2, 3, 4])
@pytest.mark.parametrize("cfg", CFGS)
def test_ring_config_epilogue_shape(cfg, case, epi):
    run, bf16_epi = EPILOGUES[epi]
    M, N, K = _shape(cfg, case, bf16_epi)
    _force(cfg)
    run(M, N, K, _seed(cfg, case, epi), f"ring cfg {cfg} case {case} {epi} {M}x{N}x{K}")


@pytest.mark.parametrize("epi", STAGED)
@pytest.mark.parametrize("K", [40, 72, 136, 200])  # 1, 2, 3, 4 k-tiles per tile: below, at and above the ring depth
@pytest.mark.parametrize("cfg", CFGS)
def test_ring_persistent_short_k(cfg, K, epi):
    """more tiles than resident workgroups, unequal tile counts per workgroup: the staging cursor crosses tile boundaries (with 3 stages
    and 1 or 2 k-tiles per tile the prologue stages k-tiles of two or three tiles) while the epilogue reuses a ring slot"""
    run, bf16_epi = EPILOGUES[epi]
    M, N, bound = _persistent_shape(cfg, bf16_epi)
    if epi == "swiglu":
        N = _up(N, 16)
    _assert_persistent(cfg, bf16_epi, M, N, bound)
    _force(cfg)
    run(M, N, K, _seed(cfg, 5, epi) + K, f"ring cfg {cfg} persistent {epi} {M}x{N}x{K}")


@pytest.mark.parametrize("epi", STAGED)
@pytest.mark.parametrize("case", [2, 3])
@pytest.mark.parametrize("flags", [0, 1, 2])  # bit 0: XCD tile order | bit 1: LDS-staged stores (3 = the default of every other test)
@pytest.mark.parametrize("cfg", CFGS)
def test_ring_store_route_flags(cfg, flags, case, epi):
    run, bf16_epi = EPILOGUES[epi]
    M, N, K = _shape(cfg, case, bf16_epi)
    _force(cfg, flags)
    run(M, N, K, _seed(cfg, case, epi), f"ring cfg {cfg} flags {flags} case {case} {epi} {M}x{N}x{K}")


@pytest.mark.parametrize("want,epi,M,N,K", [(7, "f32_resid_gamma_inplace", 200, 136, 520), (7, "bias_bf16", 200, 136, 520),
                                            (5, "gelu", 200, 136, 520), (0, "bias_bf16", 100, 136, 520)])
def test_unforced_dispatch_lands_on_ring_config(want, epi, M, N, K):
    """the dispatch table sends these shapes to the ring kernel: pinned, so the case cannot drift to another kernel unnoticed"""
    from vtp_amd import _lib
    o = ops()
    code = {"f32_resid_gamma_inplace": o.EPI_F32, "bias_bf16": o.EPI_BF16, "gelu": o.EPI_GELU}[epi]
    got = _lib.load().vtp_gemm_nt_config(M, N, K, code)
    assert got & 255 == want and got >> 8 == 0, (M, N, K, epi, got)
    EPILOGUES[epi][0](M, N, K, want * 10 + code, f"ring unforced -> cfg {want} {epi} {M}x{N}x{K}")
