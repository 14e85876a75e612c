"""tests/glue_ref.py without a GPU: every reference against the stock torch op (F.unfold, F.fold, F.pixel_shuffle, F.pixel_unshuffle,
Tensor.T, index_add_, F.embedding, oracle apply_rope), and, at the very inputs tests/test_glue_kernels_gpu.py uses, each comparison of
that test applied to a wrong variant of the reference: it must reject it."""
import pytest
import torch
import torch.nn.functional as F

import glue_ref as R
from oracle import vtp_oracle as O

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def rejected_bits(wrong, ref):
    return not R.same_bits(wrong, ref)


def rejected_sum(wrong64, ref64, sumabs, n_adds, integer):
    """the GPU test's check_sum applied to the best a kernel computing `wrong64` could return: its fp32 rounding"""
    got = (R.PREFILL + wrong64).to(F32)
    if integer:
        return not bool((got.double() == R.PREFILL + ref64).all())
    return R.ratio(got, R.PREFILL + ref64, R.atomic_bar(n_adds, sumabs)) > 1.0


def test_comparators():
    a = torch.tensor([1.0, R.NAN, -0.0, 7.0])
    assert R.same_bits(a, a.clone())
    assert R.same_bits(a, torch.tensor([1.0, -R.NAN, -0.0, 7.0]))            # a NaN need only stay a NaN
    assert not R.same_bits(a, torch.tensor([1.0, R.NAN, 0.0, 7.0]))          # -0 is not +0
    assert not R.same_bits(a, torch.tensor([1.0, 2.0, -0.0, 7.0])) and not R.same_bits(a.to(BF), a)
    assert R.ratio(torch.tensor([1.0]), torch.tensor([1.0]), 0.0) == 0.0 and R.ratio(torch.tensor([R.NAN]), torch.tensor([1.0]), 1.0) > 1
    assert R.last_pass_start(21930 * 48, R.CAP) == 4096 * 256 and R.passes(21930 * 48, R.CAP) == 2
    assert R.last_pass_start(100, R.CAP) == 0 and R.passes(100, R.CAP) == 1
    assert R.last_pass_start(2 * 4096 * 256, R.CAP) == 4096 * 256


# ------------------------------------------------------------------------------------------------------------ the caps are passed
def test_cases_pass_the_grid_caps():
    for B, H, W in R.PATCH_SHAPES[:1]:
        items = B * (H // 16) * (W // 16) * 48
        assert R.passes(items, R.CAP) == 2 and R.last_pass_start(items, R.CAP) // 48 // ((H // 16) * (W // 16)) == B - 1 and H != W
    B, h, w = R.L1_SHAPES[0]
    assert R.passes(B * h * w * 48, R.L1_CAP) == 2
    B, N, D = R.ASSEMBLE_SHAPES[0]
    assert R.passes(B * N * D // 4, R.CAP) == 2
    assert R.passes(R.CAST_N[-1] // 4 + 1, R.CAP) == 2 and R.CAST_N[-1] & 3 == 3
    assert R.passes(R.SLAB_CASES[-1][0] // 4, R.SLAB_CAP) == 2
    B, N, heads = R.ROPE_CASES[0][:3]
    assert R.passes(B * N * 2 * heads * 4, R.CAP) == 2
    assert [R.token_rows_plan(b * n)[0] for b, n, _ in R.TOKEN_ROWS_SHAPES] == [16, 16, 17, 256]
    assert R.TOKEN_ROWS_SHAPES[0][0] * R.TOKEN_ROWS_SHAPES[0][1] < 16


# ------------------------------------------------------------------------------------------------------------ patches and pixels
@pytest.mark.parametrize("B,H,W", R.PATCH_SHAPES)
def test_patch_references_match_the_stock_ops(B, H, W):
    h, w = H // 16, W // 16
    T = B * h * w
    img, t = R.patch_case(B, H, W)
    unfold = F.unfold(img, 16, stride=16).transpose(1, 2).reshape(T, 768)
    assert R.same_bits(R.im2col_ref(img, B, H, W, 0, F32)[:T], unfold)
    for pre in R.PATCH_PREFIXES:
        rows = R.im2col_ref(img, B, H, W, pre, BF)
        v = rows[:B * (h * w + pre)].view(B, h * w + pre, 768)
        assert R.same_bits(v[:, pre:].reshape(T, 768), unfold.to(BF))
        assert bool((v[:, :pre] == R.SENTINEL).all()) and bool((rows[B * (h * w + pre):] == R.SENTINEL).all())
    fold = F.fold(unfold.view(B, h * w, 768).transpose(1, 2), (H, W), 16, stride=16)
    assert R.same_bits(R.fold_ref(unfold, B, H, W)[:img.numel()], fold.reshape(-1)) and R.same_bits(fold, img)
    shuffled = F.pixel_shuffle(t.float().view(B, h, w, 768).permute(0, 3, 1, 2), 16)
    assert R.same_bits(R.fold_ref(t, B, H, W)[:img.numel()], shuffled.reshape(-1))
    un = F.pixel_unshuffle(img, 16).permute(0, 2, 3, 1).reshape(T, 768)
    assert R.same_bits(R.im2col_ref(img, B, H, W, 0, BF)[:T], un.to(BF))


@pytest.mark.parametrize("B,H,W", R.PATCH_SHAPES)
def test_patch_comparisons_reject_wrong_variants(B, H, W):
    img, t = R.patch_case(B, H, W)
    T = B * (H // 16) * (W // 16)
    variants = ["drop_last_pass"] + (["swap_hw"] if H != W else [])
    for pre in R.PATCH_PREFIXES:
        ref = R.im2col_ref(img, B, H, W, pre, F32)
        for wrong in variants + (["prefix_const"] if pre and B > 1 else []):
            bad = R.im2col_ref(img, B, H, W, pre, F32, wrong)
            assert rejected_bits(bad, ref) and rejected_bits(bad.to(BF), ref.to(BF)), (pre, wrong)
    t32 = R.im2col_ref(img, B, H, W, 0, F32)[:T]
    for wrong in variants:
        assert rejected_bits(R.fold_ref(t32, B, H, W, wrong), R.fold_ref(t32, B, H, W)), wrong          # col2im16, pixel_shuffle16_f32
        assert rejected_bits(R.fold_ref(t, B, H, W, wrong), R.fold_ref(t, B, H, W)), wrong              # pixel_shuffle16
        assert rejected_bits(R.im2col_ref(img, B, H, W, 0, BF, wrong), R.im2col_ref(img, B, H, W, 0, BF)), wrong   # pixel_unshuffle16


@pytest.mark.parametrize("integer", (True, False))
@pytest.mark.parametrize("B,h,w", R.L1_SHAPES)
def test_l1_reference_and_wrong_variants(B, h, w, integer):
    t, target, gscale = R.l1_case(B, h, w, integer)
    dt, loss, n_adds = R.l1_ref(t, target, B, h, w, gscale)
    T = B * h * w
    tr = t.float().clone().requires_grad_(True)
    diff = F.pixel_shuffle(tr.view(B, h, w, 768).permute(0, 3, 1, 2), 16) - target
    (diff.abs().sum() * gscale).backward()
    assert R.same_bits(dt[:T], tr.grad.to(BF))                        # autograd's sign(0) = 0 as well
    assert abs(float(loss) - float(diff.detach().double().abs().sum())) <= 1e-12 * float(loss)
    ties = int((dt[:T] == 0).sum())
    assert 0.08 * T * 768 < ties                                      # the exact ties are in the data
    if integer:
        R.assert_exact_case(loss, R.PREFILL, t, target)
    variants = ["drop_last_pass"] + (["swap_hw"] if h != w else [])
    for wrong in variants:
        bad_dt, bad_loss, _ = R.l1_ref(t, target, B, h, w, gscale, wrong)
        assert rejected_bits(bad_dt, dt), wrong
        if wrong == "drop_last_pass":
            assert rejected_sum(bad_loss.view(1), loss.view(1), loss.view(1), n_adds, integer)
    one = loss - (t.float() - target.reshape(-1)[R.patch_src(B, h * 16, w * 16)]).abs().double().max()   # one element dropped
    if integer:
        assert rejected_sum(one.view(1), loss.view(1), loss.view(1), n_adds, True)


# ------------------------------------------------------------------------------------------------------------ token glue
@pytest.mark.parametrize("with_masks", (True, False))
@pytest.mark.parametrize("B,N,D", R.ASSEMBLE_SHAPES)
def test_assemble_reference_and_wrong_variants(B, N, D, with_masks):
    x, cls, mt, masks = R.assemble_case(B, N, D, with_masks)
    ref = R.assemble_ref(x, cls, mt, masks, B, N, D)
    v, xv = ref[:B * N].view(B, N, D), x[:B * N].view(B, N, D)
    m = torch.zeros(B, N, dtype=torch.bool)
    if with_masks:
        m[:, 1:] = masks.bool()
    want = torch.where(m[..., None], mt.expand(B, N, D), xv)
    want = torch.cat((cls.expand(B, 1, D), want[:, 1:]), 1)
    assert R.same_bits(v, want) and R.same_bits(ref[B * N:], x[B * N:])
    cls_in_last_pass = (B - 1) * N * (D // 4) >= R.last_pass_start(B * N * (D // 4), R.CAP)
    assert rejected_bits(R.assemble_ref(x, cls, mt, masks, B, N, D, "drop_last_pass"), ref) == (with_masks or cls_in_last_pass)
    assert cls_in_last_pass == ((B, N, D) != R.ASSEMBLE_SHAPES[0])
    if with_masks:
        assert rejected_bits(R.assemble_ref(x, cls, mt, None, B, N, D), ref)


@pytest.mark.parametrize("integer", (True, False))
@pytest.mark.parametrize("B,N,D", R.TOKEN_ROWS_SHAPES)
def test_token_rows_reference_and_wrong_variants(B, N, D, integer):
    dx, dxb, masks = R.token_rows_case(B, N, D, integer)
    assert bool(masks[0].all()) and not bool(masks[1].any()) and not bool((dxb == 0).any())
    out, s_m, a_m, s_c, a_c, n_adds = R.token_rows_ref(dx, dxb, masks, B, N, D, True)
    v = dx.view(B, N, D).double()
    sel = torch.cat((torch.zeros(B, 1), masks.double()), 1)
    assert torch.allclose(s_m, torch.einsum("bn,bnd->d", sel, v), rtol=0, atol=1e-9 * float(a_m.max() + 1))
    assert torch.allclose(s_c, v[:, 0].sum(0), rtol=0, atol=1e-9 * float(a_c.max() + 1))
    zero = (out[:B * N].view(B, N, D) == 0).all(-1)
    assert torch.equal(zero, sel.bool() | (torch.arange(N) == 0)) and R.same_bits(out[B * N:], dxb[B * N:])
    assert R.same_bits(out[:B * N][~zero.view(-1)], dxb[:B * N][~zero.view(-1)])
    out2, *_ = R.token_rows_ref(dx, dxb, masks, B, N, D, False)       # mask_rows_bwd leaves the cls rows alone
    assert R.same_bits(out2[:B * N].view(B, N, D)[:, 0], dxb[:B * N].view(B, N, D)[:, 0]) and rejected_bits(out2, out)
    if integer:
        R.assert_exact_case(torch.maximum(a_m, a_c), R.PREFILL, dx)
    _, b_m, _, b_c, _, _ = R.token_rows_ref(dx, dxb, masks, B, N, D, True, "drop_row")
    if integer:                                                       # one row of a column sum dropped: no tolerance could see it
        assert rejected_sum(b_m, s_m, a_m, n_adds, True) and rejected_sum(b_c, s_c, a_c, n_adds, True)


@pytest.mark.parametrize("D", R.STRIDED_D)
def test_strided_rowsum_reference(D):
    for B in R.STRIDED_B:
        x, stride = R.strided_case(B, D)
        ref = R.strided_rowsum_ref(x, stride, R.PREFILL, B, D)
        rows = x.view(B, stride)[:, :D].double()
        assert ref.dtype == F32 and R.ratio(ref, R.PREFILL + rows.sum(0), R.atomic_bar(R.cdiv(B, 4) + 3, rows.abs().sum(0))) <= 1.0
        if B > 1:
            assert rejected_bits(R.strided_rowsum_ref(x, stride, R.PREFILL, B - 1, D), ref)
        assert rejected_bits(R.strided_rowsum_ref(x, stride, 0.0, B, D), ref)             # `=` for `+=`


# ------------------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("C", R.TRANSPOSE_C)
@pytest.mark.parametrize("R_", R.TRANSPOSE_R)
def test_transpose_reference_and_wrong_variants(R_, C):
    for remap in (False, True):
        x, rin = R.matrix_case(R_, C, False, remap)
        ref = R.transpose_ref(x, rin, R_, C)
        live = x[~torch.isnan(x[:, 0])][:, :C]                        # the rows the remap reads are the rows that are not NaN
        assert live.shape == (R_, C) and R.same_bits(ref[:C, :R_], live.T)
        assert not bool(ref[:C, R_:].any()) and ref.shape[1] >= R_ + 16 and bool((ref[C:] == R.SENTINEL).all())
        assert rejected_bits(R.transpose_ref(x, rin, R_, C, "skip_tile"), ref)
    H = R.swiglu_h(C)
    assert sorted(R.swiglu_dst(C, H).tolist()) == sorted(set(R.swiglu_dst(C, H).tolist())) and int(R.swiglu_dst(C, H).max()) < 2 * H
    for integer in (True, False):
        x, rin = R.matrix_case(R_, C, integer, True)
        s, a = R.colsum_ref(x, rin, C, True)
        live = x[rin, :C].double()
        want = torch.zeros(2 * H, dtype=F64).index_add_(0, R.swiglu_dst(C, H), live.sum(0))
        assert torch.equal(s, want)
        n_adds = R.transpose_colsum_adds(R_)
        if integer:
            R.assert_exact_case(a, R.PREFILL, x[rin, :C])
            assert rejected_sum(R.colsum_ref(x, rin, C, True, "drop_row")[0], s, a, n_adds, True) or not bool(live[-1].any())
        assert rejected_sum(R.colsum_ref(x, rin, C, True, "no_swiglu")[0], s, a, n_adds, integer) or C <= 8    # at C = 8 the remap is the identity


@pytest.mark.parametrize("remap", (False, True))
@pytest.mark.parametrize("R_", R.COLSUM_R)
def test_colsum_reference_and_wrong_variants(R_, remap):
    C = R.COLSUM_C
    for integer in (True, False):
        x, rin = R.matrix_case(R_, C, integer, remap, key=59)
        s, a = R.colsum_ref(x, rin, C, remap)
        live = x[~torch.isnan(x[:, 0])][:, :C].double()
        dst = R.swiglu_dst(C, R.swiglu_h(C)) if remap else torch.arange(C)
        assert torch.equal(s, torch.zeros(s.numel(), dtype=F64).index_add_(0, dst, live.sum(0)))
        if integer:
            R.assert_exact_case(a, R.PREFILL, x[rin, :C])
            bad = R.colsum_ref(x, rin, C, remap, "drop_row")[0]
            assert rejected_sum(bad, s, a, R.colsum_adds(R_), True) or not bool(live[-1].any())
        if remap:
            assert rejected_sum(R.colsum_ref(x, rin, C, True, "no_swiglu")[0], s, a, R.colsum_adds(R_), integer)


def test_colsum_rows_counts():
    C, RMAX = R.COLSUM_C, R.COLSUM_ROWS_RMAX
    x, rin = R.matrix_case(RMAX, C, True, False, key=61)
    s_all, a_all = R.colsum_ref(x, rin, C, False, n_rows=RMAX)
    assert torch.equal(s_all, x[:, :C].double().sum(0))
    assert not bool(R.colsum_ref(x, rin, C, False, n_rows=0)[0].any())
    s1, a1 = R.colsum_ref(x, rin, C, False, n_rows=1)
    assert torch.equal(s1, x[0, :C].double()) and rejected_sum(s_all, s1, a1, R.colsum_adds(RMAX), True)


def test_cast_reference_and_wrong_variants():
    sp = R.SPECIALS
    b = sp.to(BF)
    assert R.bits(b[:5]).tolist()[:4] == [0, -32768, 0x7F80, -128] and bool(torch.isnan(b[4]))
    assert [v & 0xFFFF for v in R.bits(b[12:16]).tolist()] == [0x3F80, 0x3F82, 0xBF80, 0xBF82]      # ties to even, both directions
    assert [v & 0xFFFF for v in R.bits(b[16:18]).tolist()] == [0x3F81, 0x3F80]
    assert [v & 0xFFFF for v in R.bits(b[18:22]).tolist()] == [0x7F80, 0xFF80, 0x7F80, 0x7F7F]      # the largest finite fp32 rounds to inf
    assert [v & 0xFFFF for v in R.bits(b[5:12]).tolist()] == [0, 0x8000, 0x0040, 0x0080, 0, 0x0002, 0x0080]   # subnormals are kept
    for n in R.CAST_N:
        x = R.cast_case(n)
        ref = R.cast_ref(x)
        assert R.same_bits(ref[:n], x.to(BF)) and bool((ref[n:] == R.SENTINEL).all())
        if n & 3:
            assert rejected_bits(R.cast_ref(x, "no_tail"), ref)
        if n >= 4:
            assert rejected_bits(R.cast_ref(x, "drop_last_pass"), ref)
    seen_body, seen_tail = set(), set()
    for x in R.cast_special_cases():
        seen_body |= set(R.bits(x[:4]).tolist())
        seen_tail |= set(R.bits(x[4:]).tolist())
        assert rejected_bits(R.cast_ref(x, "no_tail"), R.cast_ref(x))
    assert seen_body == seen_tail == set(R.bits(sp).tolist())
    for R_, C in R.CAST_T_SHAPES:
        x = R.cast_t_case(R_, C)
        ref = R.cast_t_ref(x)
        assert R.same_bits(ref[:R_ * C].view(C, R_), x.T.to(BF)) and rejected_bits(R.cast_t_ref(x, "skip_tile"), ref)


@pytest.mark.parametrize("n,S,acc", R.SLAB_CASES)
def test_reduce_slabs_reference_and_wrong_variants(n, S, acc):
    slabs, stride, dst = R.slab_case(n, S)
    assert stride > n
    ref = R.reduce_slabs_ref(slabs, stride, S, dst, n, acc)
    terms = torch.stack([slabs[s * stride:s * stride + n] for s in range(S)] + ([dst[:n]] if acc else [])).double()
    assert R.ratio(ref[:n], terms.sum(0), S * R.U * terms.abs().sum(0)) <= 1.0 and R.same_bits(ref[n:], dst[n:])
    assert rejected_bits(R.reduce_slabs_ref(slabs, stride, S, dst, n, acc, "ignore_accumulate"), ref)
    assert rejected_bits(R.reduce_slabs_ref(slabs, stride, S, dst, n, acc, "drop_last_pass"), ref)
    if S > 1:
        assert rejected_bits(R.reduce_slabs_ref(slabs, n, S, dst, n, acc), ref)           # the stride taken for n


def test_prep_weights_table_and_references():
    modes = {(m, "16B" if (o1 or 0) == 0 and (o2 or 0) == 0 and (od or 0) == 0 and (ot or 0) == 0 and (m == 2 or (r % 4 == 0 and c % 4 == 0)) else "scalar")
             for m, r, c, _, o1, o2, od, ot in R.PREP_TABLE}
    assert {(0, "16B"), (0, "scalar"), (1, "16B"), (1, "scalar"), (2, "16B"), (2, "scalar")} <= modes and len(R.PREP_TABLE) >= 5
    outs = {(od is not None, ot is not None) for *_, od, ot in R.PREP_TABLE}
    assert outs == {(True, True), (True, False), (False, True)}
    starts = R.prep_tile_starts()
    assert all(starts[d1] > starts[d0] for d0, d1 in R.PREP_RUNS) and {d for a, b in R.PREP_RUNS for d in range(a, b)} == set(range(len(R.PREP_TABLE)))
    for d, (mode, R_, C, key, *_) in enumerate(R.PREP_TABLE):
        src, src2 = R.prep_source(key)
        dst, dstT = R.prep_ref(d)
        if mode == 0:
            assert R.same_bits(dst, src.to(BF)) and R.same_bits(dstT, src.to(BF).T.contiguous())
        else:
            H = R_ // 2
            shape = (H // 8, 8) + tuple(src.shape[1:])
            inter = torch.stack((src.view(shape), src2.view(shape)), 1).reshape((R_,) + tuple(src.shape[1:]))    # [8 of w1 | 8 of w2 | ...]
            if mode == 1:
                assert R.same_bits(dst, inter.to(BF)) and R.same_bits(dstT, inter.to(BF).T.contiguous())
            else:
                assert R.same_bits(dst, inter) and dstT is None
        if mode != 2:
            bad, badT = R.prep_ref(d, "skip_tile")
            assert rejected_bits(bad, dst) and rejected_bits(badT, dstT)
    w = R.prep_source("w")[0]
    assert set(R.bits(R.SPECIALS).tolist()) <= set(R.bits(w).view(-1).tolist())


# ------------------------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("B,N,heads,prefix,h,w", R.ROPE_CASES)
def test_rope_reference_and_wrong_variants(B, N, heads, prefix, h, w):
    x32, sin, cos = R.rope_case(B, N, heads, prefix, h, w)
    xb = x32.to(BF)
    D = heads * 64
    ref = R.rope_ref(xb, sin, cos, B, N, heads, prefix)
    q, k, v = xb.view(B, N, 3, heads, 64).unbind(2)
    qr, kr = O.apply_rope(q.transpose(1, 2), k.transpose(1, 2), sin, cos)
    want = torch.stack([qr.transpose(1, 2), kr.transpose(1, 2), v], dim=2).reshape(B * N, 3 * D)
    assert R.same_bits(ref, want)
    q32, k32, v32 = x32.view(B, N, 3, heads, 64).unbind(2)
    qr, kr = O.apply_rope(q32.transpose(1, 2), k32.transpose(1, 2), sin, cos)
    want32 = torch.stack([qr.transpose(1, 2), kr.transpose(1, 2), v32], dim=2).reshape(B * N, 3 * D)
    ref32 = R.rope_ref(x32, sin, cos, B, N, heads, prefix)
    assert R.same_bits(ref32, want32) and R.same_bits(ref32[:, 2 * D:], x32[:, 2 * D:])
    inv = R.rope_ref(xb, sin, cos, B, N, heads, prefix, inverse=True)
    assert R.same_bits(inv[:, 2 * D:], xb[:, 2 * D:]) and rejected_bits(inv, ref)
    g = torch.Generator().manual_seed(5)                              # the inverse is the transpose: <R x, y> = <x, R^T y> up to bf16 rounding
    y = torch.randn(B * N, 3 * D, generator=g).to(BF)
    ry = R.rope_ref(y, sin, cos, B, N, heads, prefix, inverse=True)
    lhs, rhs = (ref.double()[:, :2 * D] * y.double()[:, :2 * D]).sum(), (xb.double()[:, :2 * D] * ry.double()[:, :2 * D]).sum()
    assert abs(float(lhs - rhs)) < 2e-2 * (xb.double()[:, :2 * D] * y.double()[:, :2 * D]).abs().sum().sqrt()
    for f in (False, True):
        assert rejected_bits(R.rope_ref(xb, sin, cos, B, N, heads, prefix, inverse=f, wrong="drop_last_pass"),
                             R.rope_ref(xb, sin, cos, B, N, heads, prefix, inverse=f))
    assert rejected_bits(R.rope_ref(x32, sin, cos, B, N, heads, prefix, wrong="drop_last_pass"), ref32)
    if prefix:
        pre_rows = ref.view(B, N, 3 * D)[:, :prefix]
        assert R.same_bits(pre_rows, xb.view(B, N, 3 * D)[:, :prefix])


# ------------------------------------------------------------------------------------------------------------ text glue
@pytest.mark.parametrize("D", R.TEXT_D)
@pytest.mark.parametrize("T", R.TEXT_T)
def test_text_references_and_wrong_variants(T, D):
    for full in (True, False):
        for integer in (True, False):
            ids, lens, table, pos, dy, dx = R.text_case(T, D, full, integer)
            B = len(lens)
            assert min(lens) == 1 and max(lens) == (T if full else T - 3) and len(set(lens)) > 3
            eot, cu = R.text_plan_ref(ids)
            assert (eot + 1).tolist() == lens and cu.tolist() == [sum(lens[:b]) for b in range(B + 1)]
            x = R.embed_ref(ids, table, pos)
            assert R.same_bits(x.view(B, T, D), F.embedding(ids, table) + pos)
            rows = R.live_rows(cu, T)
            assert rows.tolist() == [b * T + t for b in range(B) for t in range(lens[b])]
            xp = R.packed(x, cu, T)
            assert R.same_bits(xp[:len(rows)], x[rows]) and bool((xp[len(rows):] == R.SENTINEL).all()) and xp.shape[0] == int(cu[B]) + R.GUARD
            s32 = R.scatter_ref(dy, eot, B, T, D)
            want = torch.zeros(B, T, D)
            want[torch.arange(B), eot.long()] = dy
            assert R.same_bits(s32.view(B, T, D), want) and R.same_bits(R.scatter_ref(dy, eot, B, T, D, BF), want.view(B * T, D).to(BF))
            assert rejected_bits(R.packed(s32, cu, T, wrong="past_end"), R.packed(s32, cu, T))       # one row past cu[B]
            for use_lens in (None, lens):
                s_t, a_t, n_t, s_p, a_p, n_p = R.embed_bwd_ref(ids, dx, use_lens)
                live = torch.ones(B, T) if use_lens is None else (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float()
                g = dx.view(B, T, D).double() * live[..., None].double()
                assert torch.equal(s_t, torch.zeros(R.TEXT_V, D, dtype=F64).index_add_(0, ids.reshape(-1), g.view(B * T, D)))
                tr = table.double().clone().requires_grad_(True)
                (F.embedding(ids, tr) * g).sum().backward()
                assert torch.allclose(s_t, tr.grad, rtol=0, atol=1e-9 * float(a_t.max() + 1)) and torch.equal(s_p, g.sum(0))
                assert int((n_t[:R.TEXT_V - 1] >= 2).sum()) > 3 and int(n_t.sum()) == int(live.sum())          # tokens repeat: the atomics collide
                if use_lens is not None:
                    assert not bool(s_p[max(lens):].any()) and not bool(a_p[max(lens):].any())
                if integer:
                    R.assert_exact_case(torch.cat((a_t.view(-1), a_p.view(-1))), R.PREFILL, dx)
                    one = g.clone()
                    one[B - 2, 0] = 0                                                       # one row of dx dropped
                    bad_t = torch.zeros(R.TEXT_V, D, dtype=F64).index_add_(0, ids.reshape(-1), one.view(B * T, D))
                    if bool(g[B - 2, 0].any()):
                        assert rejected_sum(bad_t, s_t, a_t, n_t, True) and rejected_sum(one.sum(0), s_p, a_p, n_p, True)
