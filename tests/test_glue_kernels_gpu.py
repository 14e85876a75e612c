"""The data-movement and glue kernels one by one against tests/glue_ref.py, past the caps of their grid-stride loops.

csrc/elementwise.hip: vtp_im2col16, vtp_im2col16_rows, vtp_im2col16_rows_f32, vtp_col2im16, vtp_pixel_shuffle16, vtp_pixel_shuffle16_f32,
vtp_pixel_unshuffle16, vtp_l1_loss_fwd_bwd, vtp_assemble_tokens, vtp_token_rows_bwd, vtp_mask_rows_bwd, vtp_strided_rowsum,
vtp_transpose_bf16, vtp_colsum_bf16, vtp_colsum_bf16_rows, vtp_cast_f32_bf16, vtp_cast_transpose_f32_bf16, vtp_reduce_slabs,
vtp_prep_weights, vtp_prep_weights_range, vtp_rope_qk (forward and inverse), vtp_rope_qk_f32.
csrc/clip.hip: vtp_embed_tokens, vtp_embed_tokens_bwd, vtp_gather_rows, vtp_scatter_rows, vtp_text_row_plan, vtp_embed_tokens_packed,
vtp_embed_tokens_bwd_packed, vtp_gather_rows_packed, vtp_scatter_rows_packed.

Permutations, casts and the deterministic fp32 sums are compared bit for bit (a NaN need only stay a NaN).  The atomically accumulated
sums run twice: on small integers, where any order of fp32 additions is exact and the float64 sum must be met exactly, and on a
normal draw against the bar derived in glue_ref.py.  Buffers a kernel must fully write are prefilled with NaN; accumulators with a
non-zero value; rows, columns and tails it must not touch hold finite values and are compared bit for bit, and every output has a
guard behind it.  tests/test_glue_ref_host.py shows without a GPU that each comparison rejects wrong variants at these inputs.

Every test prints `glue_kernels: <kernel> <case>: ...` (profiles/glue_kernels.log)."""
import pytest
import torch

import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vtp_amd import _lib
    _lib.load()  # loud failure if the HIP library is missing


def ops():
    from vtp_amd import ops as o
    return o


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def exact(kernel, case, got, ref, what=""):
    ok = R.same_bits(got, ref)
    print(f"glue_kernels: {kernel} {case}: {what or 'output'} bit for bit: {'yes' if ok else 'NO'}")
    assert ok, (kernel, case, what)


def exact_sum(kernel, case, got, ref64, what):
    """the integer case: the fp32 result equals the float64 sum"""
    ok = bool((got.double().cpu() == ref64).all())
    print(f"glue_kernels: {kernel} {case}: {what} equals the float64 sum: {'yes' if ok else 'NO'}")
    assert ok, (kernel, case, what)


def barred(kernel, case, got, ref64, bar, what):
    r = R.ratio(got, ref64, bar)
    print(f"glue_kernels: {kernel} {case}: {what} worst error / bar = {r:.4f}")
    assert r <= 1.0, (kernel, case, what, r)


def check_sum(kernel, case, got, ref64, sumabs, n_adds, integer, what, *inputs):
    """got = PREFILL + sum, behind it a guard that still holds PREFILL"""
    n = ref64.numel()
    assert bool((got.view(-1)[n:] == R.PREFILL).all()), (kernel, case, what, "guard")
    got = got.view(-1)[:n].view(ref64.shape)
    if integer:
        R.assert_exact_case(sumabs, R.PREFILL, *inputs)
        exact_sum(kernel, case, got, R.PREFILL + ref64, what)
    else:
        barred(kernel, case, got, R.PREFILL + ref64, R.atomic_bar(n_adds, sumabs), what)


def accumulator(n):
    return torch.full((n + R.GUARD,), R.PREFILL, dtype=F32, device=DEV)


# ------------------------------------------------------------------------------------------------------------ patches and pixels
@pytest.mark.parametrize("B,H,W", R.PATCH_SHAPES)
def test_im2col(B, H, W):
    o = ops()
    img, _ = R.patch_case(B, H, W)
    img_d = dev(img)
    for pre in R.PATCH_PREFIXES:
        ref32 = R.im2col_ref(img, B, H, W, pre, F32)
        rows = dev(R.rows_prefill(B, H, W, pre, BF))
        o.im2col16_rows(img_d, rows, B, H, W, pre)
        exact("im2col16_rows", (B, H, W, pre), rows, ref32.to(BF))
        rows32 = dev(R.rows_prefill(B, H, W, pre, F32))
        o.im2col16_rows_f32(img_d, rows32, B, H, W, pre)
        exact("im2col16_rows_f32", (B, H, W, pre), rows32, ref32)
        if pre == 0:
            plain = dev(R.rows_prefill(B, H, W, 0, BF))
            o.im2col16(img_d, plain, B, H, W)
            exact("im2col16", (B, H, W), plain, ref32.to(BF))
            back = dev(R.image_prefill(B, H, W))                      # the fold of the f32 rows is the image again
            o.col2im16(rows32, back, B, H, W)
            exact("col2im16", (B, H, W), back, R.fold_ref(ref32[:ref32.shape[0] - R.GUARD], B, H, W))
            exact("col2im16", (B, H, W), back[:img.numel()], img.reshape(-1), "inverse of im2col16_rows_f32")


@pytest.mark.parametrize("B,H,W", R.PATCH_SHAPES)
def test_pixel_shuffle_unshuffle(B, H, W):
    o = ops()
    h, w = H // 16, W // 16
    T = B * h * w
    img, t = R.patch_case(B, H, W)
    t_d = dev(t)
    out = dev(R.image_prefill(B, H, W))
    o.pixel_shuffle16(t_d, out, B, h, w)
    ref = R.fold_ref(t, B, H, W)
    exact("pixel_shuffle16", (B, h, w), out, ref)
    t32 = R.im2col_ref(img, B, H, W, 0, F32)[:T]                      # fp32 tokens that are not bf16 values: they shuffle into img
    out32 = dev(R.image_prefill(B, H, W))
    o.pixel_shuffle16_f32(dev(t32), out32, B, h, w)
    exact("pixel_shuffle16_f32", (B, h, w), out32[:img.numel()], img.reshape(-1))
    assert bool((out32[img.numel():] == R.SENTINEL).all())
    dt = dev(R.guarded((T, 768), BF))
    o.pixel_unshuffle16(out, dt, B, h, w)                             # on bf16-exact data: the inverse of the shuffle
    exact("pixel_unshuffle16", (B, h, w), dt[:T], t, "inverse of pixel_shuffle16")
    assert bool((dt[T:] == R.SENTINEL).all())
    dt2 = dev(R.guarded((T, 768), BF))
    o.pixel_unshuffle16(dev(img), dt2, B, h, w)                       # on fp32 data: the rounding
    exact("pixel_unshuffle16", (B, h, w), dt2, R.im2col_ref(img, B, H, W, 0, BF), "fp32 image")


@pytest.mark.parametrize("integer", (True, False), ids=("integer", "normal"))
@pytest.mark.parametrize("B,h,w", R.L1_SHAPES)
def test_l1_loss_fwd_bwd(B, h, w, integer):
    o = ops()
    t, target, gscale = R.l1_case(B, h, w, integer)
    dt_ref, loss_ref, n_adds = R.l1_ref(t, target, B, h, w, gscale)
    dt = dev(R.guarded((B * h * w, 768), BF))
    loss = accumulator(1)
    o.l1_loss_fwd_bwd(dev(t), dev(target), dt, loss, B, h, w, gscale)
    case = (B, h, w, "integer" if integer else "normal")
    exact("l1_loss_fwd_bwd", case, dt, dt_ref, "dt")
    assert int((dt_ref[:B * h * w] == 0).sum()) > 0                   # the ties are there
    check_sum("l1_loss_fwd_bwd", case, loss, loss_ref.view(1), loss_ref.view(1), n_adds, integer, "loss_sum", t, target)


# ------------------------------------------------------------------------------------------------------------ token glue
@pytest.mark.parametrize("with_masks", (True, False), ids=("masks", "no_masks"))
@pytest.mark.parametrize("B,N,D", R.ASSEMBLE_SHAPES)
def test_assemble_tokens(B, N, D, with_masks):
    o = ops()
    x, cls, mt, masks = R.assemble_case(B, N, D, with_masks)
    x_d = dev(x)
    o.assemble_tokens(x_d, dev(cls), dev(mt) if with_masks else None, dev(masks), B, N, D)
    exact("assemble_tokens", (B, N, D, "masks" if with_masks else "no masks"), x_d, R.assemble_ref(x, cls, mt, masks, B, N, D))


@pytest.mark.parametrize("integer", (True, False), ids=("integer", "normal"))
@pytest.mark.parametrize("B,N,D", R.TOKEN_ROWS_SHAPES)
def test_token_rows_bwd(B, N, D, integer):
    o = ops()
    dx, dxb, masks = R.token_rows_case(B, N, D, integer)
    dx_d, masks_d = dev(dx), dev(masks)
    rpb, nblocks = R.token_rows_plan(B * N)
    for mode, use_masks, with_cls in (("token_rows_bwd", True, True), ("token_rows_bwd", False, True), ("mask_rows_bwd", True, False)):
        ref_dxb, s_mask, a_mask, s_cls, a_cls, n_adds = R.token_rows_ref(dx, dxb, masks if use_masks else None, B, N, D, with_cls)
        dxb_d, d_mask, d_cls = dev(dxb), accumulator(D), accumulator(D)
        if mode == "mask_rows_bwd":
            o.mask_rows_bwd(dx_d, dxb_d, masks_d, d_mask, B, N, D)
        else:
            o.token_rows_bwd(dx_d, dxb_d, masks_d if use_masks else None, d_mask if use_masks else None, d_cls, B, N, D)
        case = (B, N, D, f"rpb {rpb} x {nblocks}", "masks" if use_masks else "no masks", "integer" if integer else "normal")
        exact(mode, case, dxb_d, ref_dxb, "dx_bf16")
        check_sum(mode, case, d_mask, s_mask, a_mask, n_adds, integer, "d_mask_token", dx)
        check_sum(mode, case, d_cls, s_cls, a_cls, n_adds, integer, "d_cls_token", dx)


@pytest.mark.parametrize("D", R.STRIDED_D)
def test_strided_rowsum(D):
    o = ops()
    for B in R.STRIDED_B:
        x, stride = R.strided_case(B, D)
        out = accumulator(D)
        o.strided_rowsum(dev(x), stride, out, B, D)
        ref = torch.full((D + R.GUARD,), R.PREFILL)
        ref[:D] = R.strided_rowsum_ref(x, stride, R.PREFILL, B, D)
        exact("strided_rowsum", (B, D), out, ref)


# ------------------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("C", R.TRANSPOSE_C)
@pytest.mark.parametrize("R_", R.TRANSPOSE_R)
def test_transpose_bf16(R_, C):
    o = ops()
    ld_out = R.transpose_ld_out(R_)
    x, rin = R.matrix_case(R_, C, False, False)
    out = dev(R.guarded((C, ld_out), BF))
    o.transpose_bf16(dev(x), C + 8, out, ld_out, R_, C)
    exact("transpose_bf16", (R_, C, "plain"), out, R.transpose_ref(x, rin, R_, C))
    H = R.swiglu_h(C)
    for integer in (True, False):                                     # column sums, the SwiGLU remap and the input-row remap in one call
        x, rin = R.matrix_case(R_, C, integer, True)
        out, cs = dev(R.guarded((C, ld_out), BF)), accumulator(2 * H)
        o.transpose_bf16(dev(x), C + 8, out, ld_out, R_, C, colsum=cs, swiglu_h=H, in_remap=R.IN_REMAP)
        case = (R_, C, "colsum + swiglu + in_remap", "integer" if integer else "normal")
        exact("transpose_bf16", case, out, R.transpose_ref(x, rin, R_, C))
        s, a = R.colsum_ref(x, rin, C, True)
        check_sum("transpose_bf16", case, cs, s, a, R.transpose_colsum_adds(R_), integer, "colsum", x[rin, :C])


@pytest.mark.parametrize("remap", (False, True), ids=("plain", "remaps"))
@pytest.mark.parametrize("R_", R.COLSUM_R)
def test_colsum_bf16(R_, remap):
    o = ops()
    C = R.COLSUM_C
    H = R.swiglu_h(C) if remap else 0
    for integer in (True, False):
        x, rin = R.matrix_case(R_, C, integer, remap, key=59)
        cs = accumulator(2 * H if remap else C)
        o.colsum_bf16(dev(x), C + 8, cs, R_, C, swiglu_h=H, in_remap=R.IN_REMAP if remap else (0, 0))
        s, a = R.colsum_ref(x, rin, C, remap)
        check_sum("colsum_bf16", (R_, C, "remaps" if remap else "plain", "integer" if integer else "normal"), cs, s, a,
                  R.colsum_adds(R_), integer, "colsum", x[rin, :C])


@pytest.mark.parametrize("count", (0, 1, R.COLSUM_ROWS_RMAX, R.COLSUM_ROWS_RMAX + 5))
def test_colsum_bf16_rows(count):
    o = ops()
    C, RMAX = R.COLSUM_C, R.COLSUM_ROWS_RMAX
    for integer in (True, False):
        x, rin = R.matrix_case(RMAX, C, integer, False, key=61)
        x = torch.cat((x, torch.full((8, C + 8), R.NAN, dtype=BF)))   # rows behind R_max: a count beyond it must not reach them
        cs = accumulator(C)
        o.colsum_bf16_rows(dev(x), C + 8, cs, torch.tensor([count], dtype=I32, device=DEV), RMAX, C)
        s, a = R.colsum_ref(x, rin, C, False, n_rows=min(count, RMAX))
        check_sum("colsum_bf16_rows", (count, RMAX, C, "integer" if integer else "normal"), cs, s, a, R.colsum_adds(RMAX), integer,
                  "colsum", x[:RMAX, :C])


@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_f32_bf16(n):
    o = ops()
    x = R.cast_case(n)
    out = dev(R.guarded((n,), BF))
    o.cast_f32_bf16(dev(x), out, n)
    exact("cast_f32_bf16", (n,), out, R.cast_ref(x))


def test_cast_f32_bf16_special_values():
    o = ops()
    for s, x in enumerate(R.cast_special_cases()):
        out = dev(R.guarded((7,), BF))
        o.cast_f32_bf16(dev(x), out, 7)
        ref = R.cast_ref(x)
        ok = R.same_bits(out, ref)
        if not ok:
            print("glue_kernels: cast_f32_bf16 special values: input bits", [hex(v & 0xFFFFFFFF) for v in R.bits(x).tolist()], "got",
                  [hex(v & 0xFFFF) for v in R.bits(out.cpu()).tolist()], "want", [hex(v & 0xFFFF) for v in R.bits(ref).tolist()])
        assert ok, s
    print(f"glue_kernels: cast_f32_bf16 special values: {len(R.SPECIALS)} rotations of n = 7 (body and tail) bit for bit: yes")


@pytest.mark.parametrize("R_,C", R.CAST_T_SHAPES)
def test_cast_transpose_f32_bf16(R_, C):
    o = ops()
    x = R.cast_t_case(R_, C)
    out = dev(R.guarded((C * R_,), BF))
    o.cast_transpose_f32_bf16(dev(x), out, R_, C)
    exact("cast_transpose_f32_bf16", (R_, C), out, R.cast_t_ref(x))


@pytest.mark.parametrize("n,S,acc", R.SLAB_CASES)
def test_reduce_slabs(n, S, acc):
    o = ops()
    slabs, stride, dst = R.slab_case(n, S)
    dst_d = dev(dst)
    o.reduce_slabs(dev(slabs), stride, S, dst_d, n, accumulate=bool(acc))
    exact("reduce_slabs", (n, S, "accumulate" if acc else "overwrite"), dst_d, R.reduce_slabs_ref(slabs, stride, S, dst, n, acc))


class _Prep:
    """the buffers of glue_ref.PREP_TABLE on the device, each view at its descriptor's offset into its own allocation"""

    def __init__(self):
        self.src, self.out, rows = [], [], []
        starts = R.prep_tile_starts()
        for d, (mode, Rr, C, key, o1, o2, od, ot) in enumerate(R.PREP_TABLE):
            s1, s2 = R.prep_source(key)
            a1 = self._at(s1, o1)
            a2 = self._at(s2, o2) if s2 is not None else None
            dt = F32 if mode == 2 else BF
            dst = None if od is None else torch.empty(od + Rr * C + R.GUARD, dtype=dt, device=DEV)
            dstT = None if ot is None else torch.empty(ot + Rr * C + R.GUARD, dtype=dt, device=DEV)
            self.src.append((a1, a2))
            self.out.append((dst, dstT))
            rows.append([a1.data_ptr(), a2.data_ptr() if a2 is not None else 0,
                         0 if dst is None else dst[od:].data_ptr(), 0 if dstT is None else dstT[ot:].data_ptr(), Rr, C, mode, starts[d]])
        self.desc = torch.tensor(rows, dtype=torch.int64, device=DEV)
        self.starts = starts

    @staticmethod
    def _at(t, off):
        buf = torch.zeros(off + t.numel(), dtype=F32, device=DEV)
        buf[off:] = t.reshape(-1).to(DEV)
        return buf[off:]

    def fill(self, value):
        for pair in self.out:
            for t in pair:
                if t is not None:
                    t.fill_(value)

    @staticmethod
    def expected(d):
        """the two whole allocations of descriptor d after a launch that covers it: the data, around it the sentinel"""
        mode, Rr, C, key, o1, o2, od, ot = R.PREP_TABLE[d]
        out = []
        for off, ref in zip((od, ot), R.prep_ref(d)):
            if off is None:
                out.append(None)
                continue
            t = torch.full((off + Rr * C + R.GUARD,), R.SENTINEL, dtype=ref.dtype)
            t[off:off + Rr * C] = ref.reshape(-1)
            out.append(t)
        return out


def test_prep_weights_and_range():
    o = ops()
    P = _Prep()
    n = len(R.PREP_TABLE)
    P.fill(R.NAN)
    for d in range(n):                                                # NaN where the data goes, the sentinel in front of and behind it
        mode, Rr, C, key, o1, o2, od, ot = R.PREP_TABLE[d]
        for t, off in zip(P.out[d], (od, ot)):
            if t is not None:
                t[:off] = R.SENTINEL
                t[off + Rr * C:] = R.SENTINEL
    o.prep_weights(P.desc, n, P.starts[n])
    full = []
    for d in range(n):
        mode, Rr, C, key, o1, o2, od, ot = R.PREP_TABLE[d]
        want = P.expected(d)
        for t, w, name in zip(P.out[d], want, ("dst", "dstT")):
            if t is not None:
                exact("prep_weights", (d, f"mode {mode}", Rr, C, key, f"offsets {o1} {o2} {od} {ot}"), t, w, name)
        full.append([None if t is None else t.clone() for t in P.out[d]])
    for a, b in ((0, 2), (0, 3), (4, 5), (6, 7)):                     # the same values through the 16-byte and the scalar path
        for which, (ta, tb) in enumerate(zip(full[a], full[b])):
            if ta is not None and tb is not None:
                na = R.PREP_TABLE[a][1] * R.PREP_TABLE[a][2]
                oa, ob = R.PREP_TABLE[a][6 + which], R.PREP_TABLE[b][6 + which]
                exact("prep_weights", (a, b), ta[oa:oa + na], tb[ob:ob + na], f"both paths, {('dst', 'dstT')[which]}")
    for d0, d1 in R.PREP_RUNS:
        P.fill(R.SENTINEL)
        o.prep_weights_range(P.desc[d0:], d1 - d0, P.starts[d0], P.starts[d1] - P.starts[d0])
        ok = True
        for d in range(n):
            for t, f in zip(P.out[d], full[d]):
                if t is None:
                    continue
                ok = ok and (R.same_bits(t, f) if d0 <= d < d1 else bool((t == R.SENTINEL).all()))
        print(f"glue_kernels: prep_weights_range run [{d0}, {d1}) tiles [{P.starts[d0]}, {P.starts[d1]}): its outputs as the full launch, "
              f"every other destination untouched: {'yes' if ok else 'NO'}")
        assert ok, (d0, d1)


# ------------------------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("B,N,heads,prefix,h,w", R.ROPE_CASES)
def test_rope_past_the_cap(B, N, heads, prefix, h, w):
    o = ops()
    x32, sin, cos = R.rope_case(B, N, heads, prefix, h, w)
    sin_d, cos_d = dev(sin), dev(cos)
    D3 = 3 * heads * 64

    def run(x, **kw):
        buf = dev(R.guarded((B * N, D3), x.dtype))
        buf[:B * N] = dev(x)
        if x.dtype == F32:
            o.rope_qk_f32(buf, sin_d, cos_d, B, N, heads, prefix)
        else:
            o.rope_qk(buf, sin_d, cos_d, B, N, heads, prefix, **kw)
        assert bool((buf[B * N:] == R.SENTINEL).all())
        return buf[:B * N]

    xb = x32.to(BF)
    case = (B, N, heads, f"prefix {prefix}")
    exact("rope_qk", case, run(xb), R.rope_ref(xb, sin, cos, B, N, heads, prefix), "forward")
    exact("rope_qk", case, run(xb, inverse=True), R.rope_ref(xb, sin, cos, B, N, heads, prefix, inverse=True), "inverse")
    exact("rope_qk_f32", case, run(x32), R.rope_ref(x32, sin, cos, B, N, heads, prefix))


# ------------------------------------------------------------------------------------------------------------ text glue
@pytest.mark.parametrize("D", R.TEXT_D)
@pytest.mark.parametrize("T", R.TEXT_T)
def test_text_glue_padded_and_packed(T, D):
    o = ops()
    V = R.TEXT_V
    for full in (True, False):
        for integer in (True, False):
            ids, lens, table, pos, dy, dx = R.text_case(T, D, full, integer)
            B = len(lens)
            case = (T, D, "longest T" if full else "longest T - 3", "integer" if integer else "normal")
            eot_ref, cu_ref = R.text_plan_ref(ids)
            rows_live = int(cu_ref[B])
            ids_d, table_d, pos_d, dy_d = dev(ids), dev(table), dev(pos), dev(dy)
            # the plan
            eot_p, cu = torch.full((B + 1,), -7, dtype=I32, device=DEV), torch.full((B + 2,), -7, dtype=I32, device=DEV)
            n_rows = torch.full((2,), -7, dtype=I32, device=DEV)
            o.text_row_plan(ids_d, eot_p, cu, n_rows, B, T)
            ok = (torch.equal(eot_p.cpu()[:B], eot_ref) and torch.equal(cu.cpu()[:B + 1], cu_ref) and int(n_rows[0]) == rows_live
                  and int(eot_p[B]) == -7 and int(cu[B + 1]) == -7 and int(n_rows[1]) == -7)
            print(f"glue_kernels: text_row_plan {case}: eot, cu and the row count: {'yes' if ok else 'NO'}")
            assert ok
            # forward: embed, gather
            x_ref = R.embed_ref(ids, table, pos)
            x = dev(R.guarded((B * T, D), F32))
            eot = torch.full((B + 1,), -7, dtype=I32, device=DEV)
            o.embed_tokens(ids_d, table_d, pos_d, x, eot, B, T, D)
            exact("embed_tokens", case, x[:B * T], x_ref)
            assert bool((x[B * T:] == R.SENTINEL).all()) and torch.equal(eot.cpu()[:B], eot_ref) and int(eot[B]) == -7
            xp = dev(R.guarded((rows_live, D), F32))
            o.embed_tokens_packed(ids_d, table_d, pos_d, xp, cu, B, T, D)
            exact("embed_tokens_packed", case, xp, R.packed(x_ref, cu_ref, T), "the live rows of the padded result, the rest untouched")
            pooled_ref = x_ref.view(B, T, D)[torch.arange(B), eot_ref.long()]
            pooled = dev(R.guarded((B, D), F32))
            o.gather_rows(x, eot, pooled, B, T, D)
            exact("gather_rows", case, pooled[:B], pooled_ref)
            pooled_p = dev(R.guarded((B, D), F32))
            o.gather_rows_packed(xp, cu, pooled_p, B, D)
            exact("gather_rows_packed", case, pooled_p, pooled)
            # backward: scatter (with and without the bf16 copy), embed_bwd
            s32, s16 = R.scatter_ref(dy, eot_ref, B, T, D), R.scatter_ref(dy, eot_ref, B, T, D, BF)
            for with_bf in (True, False):
                g32, g16 = dev(R.guarded((B * T, D), F32)), dev(R.guarded((B * T, D), BF))
                o.scatter_rows(dy_d, eot, g32, g16 if with_bf else None, B, T, D)
                r32, r16 = R.guarded((B * T, D), F32), R.guarded((B * T, D), BF)
                r32[:B * T] = s32
                if with_bf:
                    r16[:B * T] = s16
                exact("scatter_rows", case, g32, r32, "dx" + ("" if with_bf else ", no bf16 copy"))
                exact("scatter_rows", case, g16, r16, "dx_bf16")
                p32, p16 = dev(R.guarded((rows_live, D), F32)), dev(R.guarded((rows_live, D), BF))
                o.scatter_rows_packed(dy_d, cu, p32, p16 if with_bf else None, B, T, D)
                exact("scatter_rows_packed", case, p32, R.packed(s32, cu_ref, T), "dx" + ("" if with_bf else ", no bf16 copy"))
                exact("scatter_rows_packed", case, p16, R.packed(s16, cu_ref, T) if with_bf else R.guarded((rows_live, D), BF), "dx_bf16")
            for name, use_lens in (("embed_tokens_bwd", None), ("embed_tokens_bwd_packed", lens)):
                s_t, a_t, n_t, s_p, a_p, n_p = R.embed_bwd_ref(ids, dx, use_lens)
                d_table, d_pos = accumulator(V * D), accumulator(T * D)
                if use_lens is None:
                    o.embed_tokens_bwd(ids_d, dev(dx), d_table, d_pos, B, T, D)
                else:
                    o.embed_tokens_bwd_packed(ids_d, dev(R.packed(dx, cu_ref, T, R.NAN)), d_table, d_pos, cu, B, T, D)
                    assert not bool(s_p[max(lens):].any())            # rows of d_pos beyond the longest caption: the prefill, exactly
                    assert bool((d_pos[:T * D].view(T, D)[max(lens):] == R.PREFILL).all())
                check_sum(name, case, d_table, s_t, a_t, n_t, integer, "d_table", dx)
                check_sum(name, case, d_pos, s_p, a_p, n_p, integer, "d_pos", dx)


# ------------------------------------------------------------------------------------------------------------ what the C ABI refuses
def test_c_abi_refusals():
    """the argument combinations next to the cases above that the entry points reject (before any launch) rather than run"""
    o = ops()
    f, b = torch.zeros(64, device=DEV), torch.zeros(64, dtype=BF, device=DEV)
    u8, i32, i64 = torch.zeros(64, dtype=torch.uint8, device=DEV), torch.zeros(8, dtype=I32, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    refused = (
        ("im2col16: H not a multiple of 16", "multiples of 16", lambda: o.im2col16(f, b, 1, 24, 16)),
        ("im2col16_rows: negative prefix", "prefix >= 0", lambda: o.im2col16_rows(f, b, 1, 16, 16, -1)),
        ("col2im16: W not a multiple of 16", "multiples of 16", lambda: o.col2im16(f, f, 1, 16, 8)),
        ("assemble_tokens: D not a multiple of 4", "bad shape", lambda: o.assemble_tokens(f, f, None, None, 2, 3, 6)),
        ("assemble_tokens: N = 1", "bad shape", lambda: o.assemble_tokens(f, f, None, None, 2, 1, 4)),
        ("assemble_tokens: masks without mask_token", "without mask_token", lambda: o.assemble_tokens(f, f, None, u8, 2, 3, 4)),
        ("token_rows_bwd: D > 2048", "D <= 2048", lambda: o.token_rows_bwd(f, b, u8, f, f, 1, 2, 2052)),
        ("mask_rows_bwd: D > 2048", "D <= 2048", lambda: o.mask_rows_bwd(f, b, u8, f, 1, 2, 2052)),
        ("mask_rows_bwd: no masks", "bad argument", lambda: o.mask_rows_bwd(f, b, None, f, 1, 2, 4)),
        ("strided_rowsum: B = 0", "bad argument", lambda: o.strided_rowsum(f, 8, f, 0, 4)),
        ("transpose_bf16: C not a multiple of 8", "multiples of 8", lambda: o.transpose_bf16(b, 16, b, 8, 4, 12)),
        ("transpose_bf16: ld_out < R", "ld_out >= R", lambda: o.transpose_bf16(b, 8, b, 8, 9, 8)),
        ("transpose_bf16: ld_in < C", "multiples of 8", lambda: o.transpose_bf16(b, 8, b, 8, 4, 16)),
        ("colsum_bf16: C not a multiple of 8", "bad argument", lambda: o.colsum_bf16(b, 16, f, 4, 12)),
        ("colsum_bf16_rows: no device row count", "bad argument", lambda: o.colsum_bf16_rows(b, 8, f, None, 4, 8)),
        ("cast_f32_bf16: n = 0", "bad argument", lambda: o.cast_f32_bf16(f, b, 0)),
        ("cast_transpose_f32_bf16: C = 0", "bad argument", lambda: o.cast_transpose_f32_bf16(f, b, 4, 0)),
        ("reduce_slabs: n not a multiple of 4", "bad argument", lambda: o.reduce_slabs(f, 8, 1, f, 6)),
        ("reduce_slabs: stride not a multiple of 4", "bad argument", lambda: o.reduce_slabs(f, 10, 2, f, 8)),
        ("prep_weights: no tiles", "bad argument", lambda: o.prep_weights(i64, 1, 0)),
        ("prep_weights_range: negative tile_base", "bad argument", lambda: o.prep_weights_range(i64, 1, -1, 1)),
        ("rope_qk: prefix > N", "prefix", lambda: o.rope_qk(b, b, b, 1, 4, 1, 9)),
        ("rope_qk_f32: prefix > N", "prefix", lambda: o.rope_qk_f32(f, b, b, 1, 4, 1, 9)),
        ("embed_tokens: D not a multiple of 4", "bad argument", lambda: o.embed_tokens(i64, f, f, f, i32, 1, 2, 6)),
        ("embed_tokens_packed: D not a multiple of 4", "bad argument", lambda: o.embed_tokens_packed(i64, f, f, f, i32, 1, 2, 6)),
        ("scatter_rows_packed: B > 65535", "bad argument", lambda: o.scatter_rows_packed(f, i32, f, None, 65536, 2, 4)),
    )
    for what, match, call in refused:
        with pytest.raises(RuntimeError, match=match):
            call()
        print(f"glue_kernels: refused: {what}")
