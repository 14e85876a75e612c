"""Thin torch-tensor front end over the C ABI (include/vtp_hip.h).  Tensors only provide device memory and the
current HIP stream; every op below is a hand-written gfx950 kernel in libvtp_hip.so."""
from __future__ import annotations

import torch

from . import _lib
# the host side of the grouped weight gradients lives in vtp_amd/wgrad.py; its public names stay reachable here
from .wgrad import (W4_TN_MIN_SLICE, WgradGroup, gemm_cus, wgrad_group_fits, wgrad_group_items, wgrad_group_kernel,  # noqa: F401
                    wgrad_group_mixed_ok, wgrad_group_splits, wgrad_group_uniform_items, wgrad_k_cuts, wgrad_mixed_splits)

EPI_BF16, EPI_F32, EPI_SWIGLU, EPI_GELU, EPI_F32_ATOMIC, EPI_F32_SLAB = 0, 1, 2, 3, 4, 5
EPI_QUICK_GELU = 8  # the GELU epilogue with x * sigmoid(1.702 x)
NORM_RMS, NORM_LN = 0, 1


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _lib_():
    return _lib.load()


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


def gemm_nt(a, b, c, *, M=None, N=None, K=None, lda=None, ldb=None, ldc=None, c2=None, ldc2=0, bias=None, gamma=None,
            resid=None, epi=EPI_BF16, a_remap=(0, 0), c_remap=(0, 0), splits=1, alpha=1.0, m_rows=None):
    """c[M,N] = epi(alpha * a[M,K] @ b[N,K]^T).  a, b bf16 (K-contiguous rows).  m_rows (int32 [1] on the device): only the rows
    [0, min(M, m_rows[0])) are computed -- the rest of a is not read, the rest of c not written (ring kernel, static launch geometry)."""
    M = a.shape[0] if M is None else M
    K = a.shape[1] if K is None else K
    N = b.shape[0] if N is None else N
    lda = a.stride(0) if lda is None else lda
    ldb = b.stride(0) if ldb is None else ldb
    ldc = c.stride(0) if ldc is None else ldc
    if c2 is not None and not ldc2:
        ldc2 = c2.stride(0)
    if m_rows is not None:
        if a_remap != (0, 0) or c_remap != (0, 0) or splits != 1:
            raise ValueError("gemm_nt: a row limit takes no row remaps and one K slice")
        _lib.check(_lib_().vtp_gemm_nt_limit(_p(a), lda, _p(b), ldb, _p(c), ldc, _p(c2), ldc2, _p(bias), _p(gamma), _p(resid), M, N, K,
                                             epi, alpha, _p(m_rows), _s()), "vtp_gemm_nt_limit")
        return
    rc = _lib_().vtp_gemm_nt(_p(a), lda, _p(b), ldb, _p(c), ldc, _p(c2), ldc2, _p(bias), _p(gamma), _p(resid), M, N, K,
                             epi, a_remap[0], a_remap[1], c_remap[0], c_remap[1], splits, alpha, _s())
    _lib.check(rc, "vtp_gemm_nt")


def gemm_qkv_rope(a, w, bias, c, M, N, K, rope_pos, rope_sin, rope_cos, rope_cols):
    """c bf16 [M, N] = a @ w^T + bias with apply_rope fused (rows with rope_pos >= 0, columns < rope_cols)."""
    _lib.check(_lib_().vtp_gemm_qkv_rope(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(c), c.stride(0), M, N, K,
                                         _p(rope_pos), _p(rope_sin), _p(rope_cos), rope_cols, _s()), "vtp_gemm_qkv_rope")


def norm_fwd(x, w, b, y, stats, M, D, eps, kind, m_rows=None):
    """m_rows (here and below): int32 [1] on the device -- the kernel works on the rows [0, min(M, m_rows[0])) only"""
    if m_rows is not None:
        _lib.check(_lib_().vtp_norm_fwd_limit(_p(x), _p(w), _p(b), _p(y), _p(stats), M, D, eps, kind, _p(m_rows), _s()), "vtp_norm_fwd_limit")
        return
    _lib.check(_lib_().vtp_norm_fwd(_p(x), _p(w), _p(b), _p(y), _p(stats), M, D, eps, kind, _s()), "vtp_norm_fwd")


def norm_bwd(dy, x, w, stats, dres, dx, dxb, dw, db, M, D, kind, dx_colsum=None, m_rows=None):
    if m_rows is not None:
        _lib.check(_lib_().vtp_norm_bwd_limit(_p(dy), _p(x), _p(w), _p(stats), _p(dres), _p(dx), _p(dxb), _p(dw), _p(db), _p(dx_colsum),
                                              M, D, kind, _p(m_rows), _s()), "vtp_norm_bwd_limit")
        return
    _lib.check(_lib_().vtp_norm_bwd(_p(dy), _p(x), _p(w), _p(stats), _p(dres), _p(dx), _p(dxb), _p(dw), _p(db), _p(dx_colsum),
                                    M, D, kind, _s()), "vtp_norm_bwd")


def norm_bwd_pvec(dy, x, w, stats, dres, dx, dxb, dw, db, M, D, kind, pvec, row0, B, N, dx_colsum=None):
    """norm_bwd with pvec f32 [B, D] added to dy of the patch rows row0 + b*N + t (t >= 1) of one list item, in f32"""
    _lib.check(_lib_().vtp_norm_bwd_pvec(_p(dy), _p(x), _p(w), _p(stats), _p(dres), _p(dx), _p(dxb), _p(dw), _p(db), _p(dx_colsum),
                                         _p(pvec), row0, B, N, M, D, kind, _s()), "vtp_norm_bwd_pvec")


def norm_bwd_rows(dy, x, w, stats, dres, dres_rows, dx, dxb, dw, db, M, D, kind, dx_colsum=None):
    """norm_bwd whose residual gradient is the COMPACT buffer dres f32 [Mc, D]: row r adds dres[dres_rows[r]] (int32 [M], -1: nothing)"""
    _lib.check(_lib_().vtp_norm_bwd_rows(_p(dy), _p(x), _p(w), _p(stats), _p(dres), _p(dres_rows), dres.shape[0], _p(dx), _p(dxb), _p(dw),
                                         _p(db), _p(dx_colsum), M, D, kind, _s()), "vtp_norm_bwd_rows")


def pool_patch_rows(x, out, B, N, D, scale=None):
    """out f32 [B, D] = scale * sum of the patch rows 1..N-1 of every image of the bf16 token rows x [B*N, D]; default scale 1/(N-1): the
    mean pooling of vision_clip_feat = 'pooled'"""
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() >= B * N * D and out.dtype == torch.float32
    assert out.is_contiguous() and out.numel() >= B * D
    s = 1.0 / (N - 1) if scale is None else float(scale)
    _lib.check(_lib_().vtp_pool_patch_rows(_p(x), _p(out), B, N, D, s, _s()), "vtp_pool_patch_rows")


def rope_qk(qkv, sin, cos, B, N, heads, prefix, inverse=False):
    _lib.check(_lib_().vtp_rope_qk(_p(qkv), _p(sin), _p(cos), B, N, heads, prefix, int(inverse), _s()), "vtp_rope_qk")


def attn_fwd(q, k, v, o, lse, B, N, heads, sb, sn, sbo, sno, scale, causal=False):
    _lib.check(_lib_().vtp_attn_fwd(_p(q), _p(k), _p(v), _p(o), _p(lse), B, N, heads, sb, sn, sbo, sno, scale, int(causal),
                                    _s()), "vtp_attn_fwd")


def attn_bwd(q, k, v, o, d_o, lse, delta, dq, dk, dv, B, N, heads, sb, sn, sbo, sno, scale, causal=False, rope=None,
             rope_prefix=0):
    """rope = (sin, cos): dq / dk come back as gradients w.r.t. the un-rotated q, k (inverse RoPE fused / appended)."""
    rs, rc = (rope[0], rope[1]) if rope is not None else (None, None)
    _lib.check(_lib_().vtp_attn_bwd(_p(q), _p(k), _p(v), _p(o), _p(d_o), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), _p(rs),
                                    _p(rc), rope_prefix, B, N, heads, sb, sn, sbo, sno, scale, int(causal), _s()), "vtp_attn_bwd")


def attn_fwd_varlen(q, k, v, o, lse, cu, B, Nmax, heads, sn, sno, scale):
    """causal attention over packed captions: batch b = rows [cu[b], cu[b + 1]) of the packed buffers (cu int32 [B + 1] on the device);
    lse keeps the padded [B, heads, Nmax] layout"""
    _lib.check(_lib_().vtp_attn_fwd_varlen(_p(q), _p(k), _p(v), _p(o), _p(lse), _p(cu), B, Nmax, heads, sn, sno, scale, _s()),
               "vtp_attn_fwd_varlen")


def attn_bwd_varlen(q, k, v, o, d_o, lse, delta, dq, dk, dv, cu, B, Nmax, heads, sn, sno, scale):
    _lib.check(_lib_().vtp_attn_bwd_varlen(_p(q), _p(k), _p(v), _p(o), _p(d_o), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), _p(cu), B, Nmax,
                                           heads, sn, sno, scale, _s()), "vtp_attn_bwd_varlen")


def im2col16(img, patches, B, H, W):
    _lib.check(_lib_().vtp_im2col16(_p(img), _p(patches), B, H, W, _s()), "vtp_im2col16")


def im2col16_rows(img, rows, B, H, W, prefix=1):
    """patch p of image b -> row b * (hw + prefix) + prefix + p of rows bf16 [B * (hw + prefix), 768] (prefix rows untouched)"""
    _lib.check(_lib_().vtp_im2col16_rows(_p(img), _p(rows), B, H, W, prefix, _s()), "vtp_im2col16_rows")


def col2im16(dpatches, dimg, B, H, W):
    """d_img f32 [B,3,H,W] <- d_patches f32 [B*hw, 768] (inverse of im2col16: the PatchEmbed input gradient)"""
    _lib.check(_lib_().vtp_col2im16(_p(dpatches), _p(dimg), B, H, W, _s()), "vtp_col2im16")


def assemble_tokens(x, cls, mask_token, masks, B, N, D):
    _lib.check(_lib_().vtp_assemble_tokens(_p(x), _p(cls), _p(mask_token), _p(masks), B, N, D, _s()), "vtp_assemble_tokens")


def transpose_bf16(inp, ld_in, out, ld_out, R, C, colsum=None, swiglu_h=0, in_remap=(0, 0)):
    _lib.check(_lib_().vtp_transpose_bf16(_p(inp), ld_in, _p(out), ld_out, _p(colsum), swiglu_h, in_remap[0], in_remap[1],
                                          R, C, _s()), "vtp_transpose_bf16")


def strided_rowsum(inp, stride, out, B, D):
    _lib.check(_lib_().vtp_strided_rowsum(_p(inp), stride, _p(out), B, D, _s()), "vtp_strided_rowsum")


def token_rows_bwd(dx, dxb, masks, d_mask_token, d_cls_token, B, N, D):
    """backward of assemble_tokens: masked rows -> d_mask_token (masks may be None), row 0 of every image -> d_cls_token; both kinds of
    row zeroed in the bf16 copy"""
    _lib.check(_lib_().vtp_token_rows_bwd(_p(dx), _p(dxb), _p(masks), None if masks is None else _p(d_mask_token), _p(d_cls_token), B, N, D,
                                          _s()), "vtp_token_rows_bwd")


def mask_rows_bwd(dx, dxb, masks, d_mask_token, B, N, D):
    _lib.check(_lib_().vtp_mask_rows_bwd(_p(dx), _p(dxb), _p(masks), _p(d_mask_token), B, N, D, _s()), "vtp_mask_rows_bwd")


def cast_f32_bf16(inp, out, n):
    _lib.check(_lib_().vtp_cast_f32_bf16(_p(inp), _p(out), n, _s()), "vtp_cast_f32_bf16")


def cast_transpose_f32_bf16(inp, out, R, C):
    _lib.check(_lib_().vtp_cast_transpose_f32_bf16(_p(inp), _p(out), R, C, _s()), "vtp_cast_transpose_f32_bf16")


def prep_weights(descs, n, total_tiles):
    _lib.check(_lib_().vtp_prep_weights(_p(descs), n, total_tiles, _s()), "vtp_prep_weights")


def prep_weights_range(descs_run, n, tile_base, n_tiles):
    """descs_run: the descriptor table sliced at the run's first record (a view: rows [d0:d1] of the int64 [*, 8] table)"""
    _lib.check(_lib_().vtp_prep_weights_range(_p(descs_run), n, tile_base, n_tiles, _s()), "vtp_prep_weights_range")


def swiglu_bwd(dh, x12, dx12, M, H, db12=None):
    _lib.check(_lib_().vtp_swiglu_bwd(_p(dh), _p(x12), _p(dx12), _p(db12), M, H, _s()), "vtp_swiglu_bwd")


def gelu_bwd(dy, pre, dx, n, quick: bool = False, m_rows=None, H: int = 0):
    """m_rows: the operands are [n / H, H] and only their first min(n / H, m_rows[0]) rows are processed"""
    if m_rows is not None:
        _lib.check(_lib_().vtp_gelu_bwd_limit(_p(dy), _p(pre), _p(dx), n // H, H, int(quick), _p(m_rows), _s()), "vtp_gelu_bwd_limit")
    elif quick:
        _lib.check(_lib_().vtp_quick_gelu_bwd(_p(dy), _p(pre), _p(dx), n, _s()), "vtp_quick_gelu_bwd")
    else:
        _lib.check(_lib_().vtp_gelu_bwd(_p(dy), _p(pre), _p(dx), n, _s()), "vtp_gelu_bwd")


def pixel_shuffle16(t, img, B, h, w):
    _lib.check(_lib_().vtp_pixel_shuffle16(_p(t), _p(img), B, h, w, _s()), "vtp_pixel_shuffle16")


def pixel_unshuffle16(d_img, dt, B, h, w):
    _lib.check(_lib_().vtp_pixel_unshuffle16(_p(d_img), _p(dt), B, h, w, _s()), "vtp_pixel_unshuffle16")


def l1_loss_fwd_bwd(t, target, dt, loss_sum, B, h, w, gscale):
    _lib.check(_lib_().vtp_l1_loss_fwd_bwd(_p(t), _p(target), _p(dt), _p(loss_sum), B, h, w, gscale, _s()),
               "vtp_l1_loss_fwd_bwd")


def adamw(p, g, m, v, p_bf16, n, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    _lib.check(_lib_().vtp_adamw(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), n, lr, beta1, beta2, eps, wd, step, grad_scale,
                                 _s()), "vtp_adamw")


def adamw_dev(p, g, m, v, p_bf16, n, hyper, nodecay4=None):
    """nodecay4: uint8 [n / 4], non-zero = the four elements are exempt from weight decay"""
    if nodecay4 is None:
        _lib.check(_lib_().vtp_adamw_dev(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), n, _p(hyper), _s()), "vtp_adamw_dev")
    else:
        _lib.check(_lib_().vtp_adamw_dev_masked(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(nodecay4), n, _p(hyper), _s()),
                   "vtp_adamw_dev_masked")


def gemm_tn(a, b, c, *, M, N, K, lda, ldb, ldc, ldc2=0, resid=None, epi=EPI_F32, a_remap=(0, 0), b_remap=(0, 0),
            c_remap=(0, 0), splits=1, a_colsum=None):
    """c[M,N] f32 = a[K,M]^T @ b[K,N]  (a, b bf16 row-major, K = token rows).  a_colsum (f32 [M], accumulated): column sums
    of a over the tokens (the bias gradient of the same linear layer)."""
    rc = _lib_().vtp_gemm_tn(_p(a), lda, _p(b), ldb, _p(c), ldc, ldc2, _p(resid), M, N, K, epi, a_remap[0], a_remap[1],
                             b_remap[0], b_remap[1], c_remap[0], c_remap[1], splits, _p(a_colsum), _s())
    _lib.check(rc, "vtp_gemm_tn")


def colsum_bf16(inp, ld, out, R, C, swiglu_h=0, in_remap=(0, 0)):
    _lib.check(_lib_().vtp_colsum_bf16(_p(inp), ld, _p(out), swiglu_h, in_remap[0], in_remap[1], R, C, _s()), "vtp_colsum_bf16")


def colsum_bf16_rows(inp, ld, out, n_rows_dev, R_max, C):
    _lib.check(_lib_().vtp_colsum_bf16_rows(_p(inp), ld, _p(out), _p(n_rows_dev), R_max, C, _s()), "vtp_colsum_bf16_rows")


def gather_image_rows(src, idx, dst, dst_bf16, n_img, N, D, scale=1.0):
    _lib.check(_lib_().vtp_gather_image_rows(_p(src), _p(idx), _p(dst), _p(dst_bf16), n_img, N, D, scale, _s()), "vtp_gather_image_rows")


def scatter_image_rows(src, idx, dst, n_img, N, D, alpha=1.0, accumulate=True):
    _lib.check(_lib_().vtp_scatter_image_rows(_p(src), _p(idx), _p(dst), n_img, N, D, alpha, int(accumulate), _s()),
               "vtp_scatter_image_rows")


def gather_tail_rows(o, x, idx, o_c, x_c, T, L, M, D):
    """compact rows of the last block's tail: o_c bf16 / x_c f32 [L + T, D] = rows [0, L) of o / x [M, D] followed by rows L + idx[t]
    (idx int32 [T] on the device, -1: an all-zero row); either pair may be None"""
    _lib.check(_lib_().vtp_gather_tail_rows(_p(o), _p(x), _p(idx), _p(o_c), _p(x_c), T, L, M, D, _s()), "vtp_gather_tail_rows")


def tail_row_map(idx, row_map, T, L, M):
    """row_map int32 [M]: full row -> compact row of gather_tail_rows (-1: no compact row reads it), built on the device"""
    _lib.check(_lib_().vtp_tail_row_map(_p(idx), _p(row_map), T, L, M, _s()), "vtp_tail_row_map")


def expand_rows_bf16(src, row_map, dst, M, Mc, D):
    """dst bf16 [M, D]: row r = src[row_map[r]] (src [Mc, D]) or zero where row_map[r] < 0 -- one pass, no fill + scatter"""
    _lib.check(_lib_().vtp_expand_rows_bf16(_p(src), _p(row_map), _p(dst), M, Mc, D, _s()), "vtp_expand_rows_bf16")


def layerscale_wgrad(G, W, bias, colsum, gamma, dW, db, dgamma, N, K):
    _lib.check(_lib_().vtp_layerscale_wgrad(_p(G), _p(W), _p(bias), _p(colsum), _p(gamma), _p(dW), _p(db), _p(dgamma), N, K, _s()),
               "vtp_layerscale_wgrad")


def scaled_transpose(W, gamma, dstT, N, K):
    _lib.check(_lib_().vtp_scaled_transpose(_p(W), _p(gamma), _p(dstT), N, K, _s()), "vtp_scaled_transpose")


def gemm_splits(K, splits):
    return _lib_().vtp_gemm_splits(K, splits)


def gemm_tn_splits(M, N, K):
    return _lib_().vtp_gemm_tn_splits(M, N, K)


def reduce_slabs(slabs, stride, S, dst, n, accumulate=True):
    _lib.check(_lib_().vtp_reduce_slabs(_p(slabs), stride, S, _p(dst), n, int(accumulate), _s()), "vtp_reduce_slabs")


def ema(t, s, n, momentum):
    _lib.check(_lib_().vtp_ema(_p(t), _p(s), n, momentum, _s()), "vtp_ema")


def embed_tokens(ids, table, pos, x, eot, B, T, D):
    _lib.check(_lib_().vtp_embed_tokens(_p(ids), _p(table), _p(pos), _p(x), _p(eot), B, T, D, _s()), "vtp_embed_tokens")


def embed_tokens_bwd(ids, dx, d_table, d_pos, B, T, D):
    _lib.check(_lib_().vtp_embed_tokens_bwd(_p(ids), _p(dx), _p(d_table), _p(d_pos), B, T, D, _s()), "vtp_embed_tokens_bwd")


def gather_rows(x, idx, out, B, T, D):
    _lib.check(_lib_().vtp_gather_rows(_p(x), _p(idx), _p(out), B, T, D, _s()), "vtp_gather_rows")


def scatter_rows(dy, idx, dx, dxb, B, T, D):
    _lib.check(_lib_().vtp_scatter_rows(_p(dy), _p(idx), _p(dx), _p(dxb), B, T, D, _s()), "vtp_scatter_rows")


def text_row_plan(ids, eot, cu, rows, B, T):
    """the packed-caption plan, on the device: eot int32 [B] (first arg-max of every caption), cu int32 [B + 1] (exclusive prefix sum of
    eot + 1), rows int32 [1] (= cu[B], the live row count)"""
    _lib.check(_lib_().vtp_text_row_plan(_p(ids), _p(eot), _p(cu), _p(rows), B, T, _s()), "vtp_text_row_plan")


def embed_tokens_packed(ids, table, pos, x, cu, B, T, D):
    _lib.check(_lib_().vtp_embed_tokens_packed(_p(ids), _p(table), _p(pos), _p(x), _p(cu), B, T, D, _s()), "vtp_embed_tokens_packed")


def embed_tokens_bwd_packed(ids, dx, d_table, d_pos, cu, B, T, D):
    _lib.check(_lib_().vtp_embed_tokens_bwd_packed(_p(ids), _p(dx), _p(d_table), _p(d_pos), _p(cu), B, T, D, _s()),
               "vtp_embed_tokens_bwd_packed")


def gather_rows_packed(x, cu, out, B, D):
    _lib.check(_lib_().vtp_gather_rows_packed(_p(x), _p(cu), _p(out), B, D, _s()), "vtp_gather_rows_packed")


def scatter_rows_packed(dy, cu, dx, dxb, B, T, D):
    _lib.check(_lib_().vtp_scatter_rows_packed(_p(dy), _p(cu), _p(dx), _p(dxb), B, T, D, _s()), "vtp_scatter_rows_packed")


def l2norm_fwd(x, y, inv, B, D, eps=1e-12):
    _lib.check(_lib_().vtp_l2norm_fwd(_p(x), _p(y), _p(inv), B, D, eps, _s()), "vtp_l2norm_fwd")


def l2norm_bwd(dy, y, inv, dx, B, D):
    _lib.check(_lib_().vtp_l2norm_bwd(_p(dy), _p(y), _p(inv), _p(dx), B, D, _s()), "vtp_l2norm_bwd")


def clip_loss(img_l, txt_l, img_all, txt_all, logit_scale, Bl, Bg, D, label_offset, loss_sum, d_img_l, d_txt_l, d_img_all,
              d_txt_all, d_logit_scale, scratch):
    _lib.check(_lib_().vtp_clip_loss(_p(img_l), _p(txt_l), _p(img_all), _p(txt_all), _p(logit_scale), Bl, Bg, D, label_offset,
                                     _p(loss_sum), _p(d_img_l), _p(d_txt_l), _p(d_img_all), _p(d_txt_all), _p(d_logit_scale),
                                     _p(scratch), _s()), "vtp_clip_loss")


def qk_norm_fwd(qkv, wq, wk, out, inv, M, D, eps=1e-5):
    _lib.check(_lib_().vtp_qk_norm_fwd(_p(qkv), _p(wq), _p(wk), _p(out), _p(inv), M, D, eps, _s()), "vtp_qk_norm_fwd")


def qk_norm_bwd(dqkv, qkv, inv, wq, wk, dwq, dwk, M, D):
    _lib.check(_lib_().vtp_qk_norm_bwd(_p(dqkv), _p(qkv), _p(inv), _p(wq), _p(wk), _p(dwq), _p(dwk), M, D, _s()), "vtp_qk_norm_bwd")


def gemm_dgrad_swiglu(dy, wT, x12, dx12, M, H, K):
    """dx12[M, 2H] = SwiGLU'(x12) (.) (dy[M, K] @ wT[H, K]^T): the w3 dgrad with swiglu_bwd in its epilogue"""
    _lib.check(_lib_().vtp_gemm_dgrad_swiglu(_p(dy), dy.stride(0), _p(wT), wT.stride(0), _p(x12), x12.stride(0), _p(dx12), dx12.stride(0),
                                             M, H, K, _s()), "vtp_gemm_dgrad_swiglu")


def clip_logits(a, b, logit_scale, out, M, N, D):
    """out f32 [M, N] = exp(logit_scale) * a[M, D] @ b[N, D]^T  (the logits of modeling_vtp.py:326-329)"""
    _lib.check(_lib_().vtp_clip_logits(_p(a), _p(b), _p(logit_scale), _p(out), M, N, D, _s()), "vtp_clip_logits")


def siglip_loss(img_l, txt_all, logit_scale, logit_bias, Bl, Bg, D, label_offset, loss_sum, d_img_l, d_txt_all, d_logit_scale,
                d_logit_bias, scratch):
    """SigLIP (pairwise sigmoid) loss of the local images against all (gathered) texts: loss, feature gradients (local image rows
    / gathered text columns -- reduce-scatter the latter across ranks), d log-scale, d bias.  weight = 1 / B_local."""
    L, s = _lib_(), _s()
    _lib.check(L.vtp_clip_logits(_p(img_l), _p(txt_all), _p(logit_scale), _p(scratch), Bl, Bg, D, s), "vtp_clip_logits")
    _lib.check(L.vtp_siglip_pairs(_p(scratch), _p(logit_bias), Bl, Bg, label_offset, 1.0 / Bl, _p(loss_sum), _p(d_logit_scale),
                                  _p(d_logit_bias), s), "vtp_siglip_pairs")
    _lib.check(L.vtp_clip_grad_rows(_p(scratch), _p(txt_all), _p(logit_scale), _p(d_img_l), Bl, Bg, D, 0, s), "vtp_clip_grad_rows")
    _lib.check(L.vtp_clip_grad_cols(_p(scratch), _p(img_l), _p(logit_scale), _p(d_txt_all), Bl, Bg, D, 0, s), "vtp_clip_grad_cols")


def koleo(xn, nn_scratch, d_xn, loss_sum, B, D, weight, eps=1e-8):
    _lib.check(_lib_().vtp_koleo(_p(xn), _p(nn_scratch), _p(d_xn), _p(loss_sum), B, D, weight, eps, _s()), "vtp_koleo")


def sinkhorn_knopp(logits, inv_temp, probs, u, v, scratch, T, K, count, n_iters=3, phase=-1, count_dev=None, n_rows_dev=None):
    _lib.check(_lib_().vtp_sinkhorn_knopp(_p(logits), inv_temp, _p(probs), _p(u), _p(v), _p(scratch), T, K, float(count), _p(count_dev),
                                          _p(n_rows_dev), n_iters, phase, _s()), "vtp_sinkhorn_knopp")


def gather_token_rows(src, idx, dst, T, D):
    _lib.check(_lib_().vtp_gather_token_rows(_p(src), _p(idx), _p(dst), T, D, _s()), "vtp_gather_token_rows")


def scatter_token_rows(d_dst, idx, d_src, T, D):
    _lib.check(_lib_().vtp_scatter_token_rows(_p(d_dst), _p(idx), _p(d_src), T, D, _s()), "vtp_scatter_token_rows")


def weight_norm_prep(v, g, weff, weffT, inv_norm, K, C):
    _lib.check(_lib_().vtp_weight_norm_prep(_p(v), _p(g), _p(weff), _p(weffT), _p(inv_norm), K, C, _s()), "vtp_weight_norm_prep")


def weight_norm_bwd(dW, v, g, inv_norm, dv, dg, K, C):
    _lib.check(_lib_().vtp_weight_norm_bwd(_p(dW), _p(v), _p(g), _p(inv_norm), _p(dv), _p(dg), K, C, _s()), "vtp_weight_norm_bwd")


def softmax_center(logits, center, inv_temp, probs, T, K):
    """inv_temp: float, or a device f32 tensor (read by the kernel: graph-replay safe schedules)"""
    if isinstance(inv_temp, torch.Tensor):
        _lib.check(_lib_().vtp_softmax_center_dev(_p(logits), _p(center), _p(inv_temp), _p(probs), T, K, _s()), "vtp_softmax_center_dev")
    else:
        _lib.check(_lib_().vtp_softmax_center(_p(logits), _p(center), inv_temp, _p(probs), T, K, _s()), "vtp_softmax_center")


def dino_ce(s_logits, t_probs, t0, t1, w, inv_temp, loss_sum, d_logits, T, K):
    _lib.check(_lib_().vtp_dino_ce(_p(s_logits), _p(t_probs), _p(t0), _p(t1), _p(w), inv_temp, _p(loss_sum), _p(d_logits), T, K,
                                   _s()), "vtp_dino_ce")


def center_ema(center, col_sum, inv_count, momentum, K, count=None):
    _lib.check(_lib_().vtp_center_ema(_p(center), _p(col_sum), inv_count, _p(count), momentum, K, _s()), "vtp_center_ema")


def ema_dev(t, s, n, momentum_dev):
    _lib.check(_lib_().vtp_ema_dev(_p(t), _p(s), n, _p(momentum_dev), _s()), "vtp_ema_dev")


def adamw_ema_dev(p, g, m, v, teacher, n, hyper, nodecay4=None):
    """AdamW over one gradient bucket with the EMA update of the teacher's copy of the same elements fused in (teacher: f32 [n] or
    None; momentum = hyper[9]) -- the per-bucket optimizer lane of VTPTrainer"""
    _lib.check(_lib_().vtp_adamw_ema_dev(_p(p), _p(g), _p(m), _p(v), _p(teacher), _p(nodecay4), n, _p(hyper), _s()), "vtp_adamw_ema_dev")



def adamw_dev_grouped(p, g, m, v, p_bf16, n, hyper, group4, group_tab, ngroups):
    """adamw_dev with per-group scales.  group4: uint8 [n / 4], the group of each float4; group_tab: device f32 [ngroups, 2] rows
    (lr_scale, wd_scale): group g steps with lr * lr_scale[g] and decays with weight_decay * wd_scale[g]"""
    _lib.check(_lib_().vtp_adamw_dev_grouped(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(group4), _p(group_tab), ngroups, n, _p(hyper),
                                             _s()), "vtp_adamw_dev_grouped")


def adamw_ema_dev_grouped(p, g, m, v, teacher, n, hyper, group4, group_tab, ngroups):
    """adamw_ema_dev with per-group scales (see adamw_dev_grouped)"""
    _lib.check(_lib_().vtp_adamw_ema_dev_grouped(_p(p), _p(g), _p(m), _p(v), _p(teacher), _p(group4), _p(group_tab), ngroups, n,
                                                 _p(hyper), _s()), "vtp_adamw_ema_dev_grouped")


# ---- global gradient-norm clipping (vtp_amd/csrc/gradnorm.hip; torch.nn.utils.clip_grad_norm_, norm_type 2) ---------------------
def sumsq_partials_count(n: int) -> int:
    """number of fp64 partials sumsq_partials writes for a range of n elements (depends on n only)"""
    return int(_lib_().vtp_sumsq_partials_count(n))


def sumsq_partials(g, n, partials):
    """partials[j] = sum of g[i]^2 over chunk j of g[0, n); g f32, partials f64 (a view at the range's slot base)"""
    _lib.check(_lib_().vtp_sumsq_partials(_p(g), n, _p(partials), _s()), "vtp_sumsq_partials")


def sum_partials(partials, count, out):
    """out f64 [1] = partials[0:count].sum(), in a fixed order"""
    _lib.check(_lib_().vtp_sum_partials(_p(partials), count, _p(out), _s()), "vtp_sum_partials")


def grad_clip_finalize(partials, count, hyper, total_norm, coef):
    """total_norm = hyper[7] * sqrt(sum(partials[0:count])); coef = clamp(hyper[10] / (total_norm + 1e-6), max=1); hyper[7] *= coef"""
    _lib.check(_lib_().vtp_grad_clip_finalize(_p(partials), count, _p(hyper), _p(total_norm), _p(coef), _s()), "vtp_grad_clip_finalize")


# ---- skipping a step whose gradient norm is not finite (VTPTrainer(skip_nonfinite=True)) -----------------------------------------
def grad_clip_finalize_guarded(partials, count, hyper, total_norm, coef, state, betas):
    """grad_clip_finalize, then the decision on the device.  state: device int32 [4] {applied_steps, skipped_steps, skip_now, -}: a
    non-finite total_norm leaves hyper[7] alone and counts as skipped; hyper[5:7] get the bias corrections of Adam step
    t = applied_steps (after the increment).  betas: (beta1, beta2), host numbers"""
    import ctypes
    b = (ctypes.c_double * 2)(float(betas[0]), float(betas[1]))
    _lib.check(_lib_().vtp_grad_clip_finalize_guarded(_p(partials), count, _p(hyper), _p(total_norm), _p(coef), _p(state), b, _s()),
               "vtp_grad_clip_finalize_guarded")


def adamw_dev_guarded(p, g, m, v, p_bf16, n, hyper, skip, idx4=None, group_tab=None, ngroups=0):
    """adamw_dev (group_tab None; idx4 = nodecay4 or None) or adamw_dev_grouped (idx4 = group4) that stores nothing when the device
    int32 skip[0] is not zero"""
    _lib.check(_lib_().vtp_adamw_dev_guarded(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(idx4), _p(group_tab), ngroups, n, _p(hyper),
                                             _p(skip), _s()), "vtp_adamw_dev_guarded")


def adamw_ema_dev_guarded(p, g, m, v, teacher, n, hyper, skip, idx4=None, group_tab=None, ngroups=0):
    """adamw_ema_dev / adamw_ema_dev_grouped that store nothing when skip[0] is not zero (see adamw_dev_guarded)"""
    _lib.check(_lib_().vtp_adamw_ema_dev_guarded(_p(p), _p(g), _p(m), _p(v), _p(teacher), _p(idx4), _p(group_tab), ngroups, n,
                                                 _p(hyper), _p(skip), _s()), "vtp_adamw_ema_dev_guarded")


def ema_dev_guarded(t, s, n, momentum_dev, skip):
    _lib.check(_lib_().vtp_ema_dev_guarded(_p(t), _p(s), n, _p(momentum_dev), _p(skip), _s()), "vtp_ema_dev_guarded")


# ---- LPIPS (vtp_amd/csrc/lpips.hip, conv mode of gemm.hip) ---------------------------------------------------------------
def _f3(v):
    import ctypes
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def conv3x3(x, w, bias, y, NB, H, W, Cin, Cout, taps=9, mode=0, relu_mask=None):
    _lib.check(_lib_().vtp_conv3x3(_p(x), _p(w), _p(bias), _p(y), _p(relu_mask), NB, H, W, Cin, Cout, taps, mode, _s()), "vtp_conv3x3")


def lpips_unfold3(tok, img, out, n, H, W, shift, scale):
    _lib.check(_lib_().vtp_lpips_unfold3(_p(tok), _p(img), _p(out), n, H, W, _f3(shift), _f3(scale), _s()), "vtp_lpips_unfold3")


def lpips_fold3_bwd(dA, dt, n, H, W, scale):
    _lib.check(_lib_().vtp_lpips_fold3_bwd(_p(dA), _p(dt), n, H, W, _f3(scale), _s()), "vtp_lpips_fold3_bwd")


def maxpool2_fwd(x, y, NB, H, W, C):
    _lib.check(_lib_().vtp_maxpool2_fwd(_p(x), _p(y), NB, H, W, C, _s()), "vtp_maxpool2_fwd")


def maxpool2_bwd(Y, dP, tap, dY, NB, H, W, C):
    _lib.check(_lib_().vtp_maxpool2_bwd(_p(Y), _p(dP), _p(tap), _p(dY), NB, H, W, C, _s()), "vtp_maxpool2_bwd")


def lpips_tap(f0, f1, w, val, df0, n, H, W, C, gscale):
    _lib.check(_lib_().vtp_lpips_tap(_p(f0), _p(f1), _p(w), _p(val), _p(df0), n, H, W, C, float(gscale), _s()), "vtp_lpips_tap")


def _f3(vals):
    import ctypes
    return (ctypes.c_float * 3)(*[float(v) for v in vals])


def u8_to_images(u8_nhwc, img_nchw, mean, std, flip=False):
    """ToTensor + Normalize (+ horizontal flip): uint8 [B,H,W,3] -> f32 [B,3,H,W]  (vtp_tokenizer.py:74-81)"""
    B, H, W, _ = u8_nhwc.shape
    m, s = _f3(mean), _f3(std)
    _lib.check(_lib_().vtp_u8_to_images(_p(u8_nhwc), _p(img_nchw), B, H, W, m, s, int(bool(flip)), _s()), "vtp_u8_to_images")


def images_to_u8(img_nchw, u8_nhwc, sub, div):
    """Normalize(sub, div) -> *255 -> clamp -> uint8 -> NHWC  (vtp_tokenizer.py:105-111)"""
    B, _, H, W = img_nchw.shape
    a, d = _f3(sub), _f3(div)
    _lib.check(_lib_().vtp_images_to_u8(_p(img_nchw), _p(u8_nhwc), B, H, W, a, d, _s()), "vtp_images_to_u8")


def latent_channel_stats(latents, sums):
    B, C = latents.shape[:2]
    hw = latents[0, 0].numel()
    _lib.check(_lib_().vtp_latent_channel_stats(_p(latents), _p(sums), B, C, hw, _s()), "vtp_latent_channel_stats")


# ---- fp8 (e4m3) forward path: BASELINE config 5
E4M3_MAX = 448.0


def quantize_e4m3(src, dst, scale):
    """dst uint8 [n] = e4m3(clamp(src * scale)); src bf16 or f32; scale: float or a device f32 tensor"""
    n = src.numel()
    sd, sf = (scale, 0.0) if isinstance(scale, torch.Tensor) else (None, float(scale))
    _lib.check(_lib_().vtp_quantize_e4m3(_p(src), int(src.dtype == torch.float32), _p(dst), n, _p(sd), sf, _s()), "vtp_quantize_e4m3")


def norm_fwd_e4m3(x, w, b, y8, q_scale, stats, M, D, eps, kind):
    _lib.check(_lib_().vtp_norm_fwd_e4m3(_p(x), _p(w), _p(b), _p(y8), _p(q_scale), _p(stats), M, D, eps, kind, _s()), "vtp_norm_fwd_e4m3")


def amax(src, out):
    _lib.check(_lib_().vtp_amax(_p(src), int(src.dtype == torch.float32), src.numel(), _p(out), _s()), "vtp_amax")


def dequantize_e4m3(src, dst, inv_scale):
    _lib.check(_lib_().vtp_dequantize_e4m3(_p(src), _p(dst), src.numel(), float(inv_scale), _s()), "vtp_dequantize_e4m3")


def gemm_nt_fp8(a8, b8, c, *, M, N, K, alpha, lda=None, ldb=None, ldc=None, c2=None, ldc2=0, bias=None, resid=None, epi=EPI_BF16,
                rope=None):
    """c[M,N] = alpha * a8[M,K] @ b8[N,K]^T (+ bias, + resid | SwiGLU); a8 / b8 uint8 tensors holding e4m3;
    rope = (rope_pos, rope_sin, rope_cos, rope_cols): apply_rope fused into the bf16 epilogue"""
    lda = K if lda is None else lda
    ldb = K if ldb is None else ldb
    ldc = c.stride(0) if ldc is None else ldc
    rp = (None, None, None, 0) if rope is None else rope
    _lib.check(_lib_().vtp_gemm_nt_fp8(_p(a8), lda, _p(b8), ldb, _p(c), ldc, _p(c2), ldc2, _p(bias), _p(resid), M, N, K, epi, float(alpha),
                                       _p(rp[0]), _p(rp[1]), _p(rp[2]), rp[3], _s()), "vtp_gemm_nt_fp8")


def probe_logits(x, w, bias, logits, B, N, K):
    """logits f32 [B, N] = x[B, K] @ w[N, K]^T + bias, exact fp32 (every head of a linear-probe feature group at once);
    x may be a column slice of a wider matrix (row stride x.stride(0))"""
    _lib.check(_lib_().vtp_probe_logits(_p(x), x.stride(0), _p(w), _p(bias), _p(logits), logits.stride(0), B, N, K, _s()),
               "vtp_probe_logits")


def probe_ce(logits, labels, B, H, C, inv_rows, loss, correct=None, dlogits=None):
    """per-head mean cross-entropy (loss f32 [H] accumulated), top-1 counts (correct i32 [H] accumulated, optional) and
    dlogits = (softmax - onehot) * inv_rows (optional: None = evaluation); labels int64 [B]"""
    ldl = logits.stride(0)
    if dlogits is not None and dlogits.stride(0) != ldl:
        raise ValueError("probe_ce: dlogits must have the row stride of logits")
    _lib.check(_lib_().vtp_probe_ce(_p(logits), ldl, _p(labels), B, H, C, inv_rows, _p(loss), _p(correct), _p(dlogits), _s()),
               "vtp_probe_ce")


def probe_sgd(w, bias, mw, mb, dlogits, x, lr, B, H, C, K, momentum):
    """SGD-with-momentum step of all H heads (w [H*C, K], bias [H*C] and their momentum buffers, updated in place) from dlogits
    [B, H*C] and x [B, K]; lr f32 [H] on the device, one rate per head"""
    _lib.check(_lib_().vtp_probe_sgd(_p(w), _p(bias), _p(mw), _p(mb), _p(dlogits), dlogits.stride(0), _p(x), x.stride(0), _p(lr),
                                     B, H, C, K, momentum, _s()), "vtp_probe_sgd")


def _size_or_raise(fn, *args):
    """the size a library entry point returns; a negative one is a refusal: ValueError with the library's message"""
    n = fn(*args)
    if n < 0:
        raise ValueError(_lib_().vtp_last_error().decode(errors="replace"))
    return n


def _need_token_map(rows, cols, **tensors):
    """z / g of the dense probes: [rows = B h w, >= cols = H C] with unit column stride (a column slice of a wider matrix is fine)"""
    for name, t in tensors.items():
        if t.dim() != 2 or t.shape[0] != rows or t.stride(1) != 1:
            raise ValueError(f"{name} must be [{rows}, >= {cols}] with unit column stride, got {tuple(t.shape)}")


def seg_ce_workspace_bytes(B, h, w, Hl, Wl, H, C):
    """bytes of workspace seg_ce needs; ValueError for arguments the kernel refuses or a workspace above 2 GiB"""
    return _size_or_raise(_lib_().vtp_seg_ce_workspace_bytes, B, h, w, Hl, Wl, H, C)


def seg_ce(z, labels, hw, H, C, ignore_index, loss, call_counts, workspace, lse=None, conf=None, totals=None):
    """pixel pass of the segmentation probe: z f32 [B*h*w, >= H*C] low-resolution logits (probe_logits), labels u8 [B, Hl, Wl] ->
    loss f32 [H] (mean over the valid pixels, overwritten), call_counts i32 [2] (valid, out of range; overwritten); optional lse
    f32 [H, B, Hl, Wl] (training), conf int64 [H, C, C] (accumulated; row = target) and totals int64 [2] (accumulated)"""
    h, w = hw
    _need(labels, "labels", torch.uint8, dims=3)
    B, Hl, Wl = labels.shape
    _need(loss, "loss", torch.float32, (H,))
    _need(call_counts, "call_counts", torch.int32, (2,))
    if lse is not None:
        _need(lse, "lse", torch.float32, (H, B, Hl, Wl))
    if conf is not None:
        _need(conf, "conf", torch.int64, (H, C, C))
    if totals is not None:
        _need(totals, "totals", torch.int64, (2,))
    _need(workspace, "workspace", torch.uint8, dims=1)
    _need_f32(z=z)
    _need_gpu(labels=labels, loss=loss, call_counts=call_counts, lse=lse, conf=conf, totals=totals, workspace=workspace)
    _need_token_map(B * h * w, H * C, z=z)
    _lib.check(_lib_().vtp_seg_ce(_p(z), z.stride(0), _p(labels), B, h, w, Hl, Wl, H, C, ignore_index, _p(lse), _p(conf), _p(loss),
                                  _p(call_counts), _p(totals), _p(workspace), workspace.numel(), _s()), "vtp_seg_ce")


def seg_dlogits(z, labels, hw, H, C, ignore_index, lse, call_counts, g):
    """cell pass: g f32 [B*h*w, >= H*C] = d (mean pixel cross-entropy) / d z, gathered per cell from lse and call_counts of seg_ce"""
    h, w = hw
    _need(labels, "labels", torch.uint8, dims=3)
    B, Hl, Wl = labels.shape
    _need(lse, "lse", torch.float32, (H, B, Hl, Wl))
    _need(call_counts, "call_counts", torch.int32, (2,))
    _need_f32(z=z, g=g)
    _need_gpu(labels=labels, lse=lse, call_counts=call_counts)
    _need_token_map(B * h * w, H * C, z=z, g=g)
    _lib.check(_lib_().vtp_seg_dlogits(_p(z), z.stride(0), _p(labels), _p(lse), _p(call_counts), _p(g), g.stride(0), B, h, w, Hl, Wl,
                                       H, C, ignore_index, _s()), "vtp_seg_dlogits")


def seg_sgd_slice():
    """token rows per weight-gradient slice of seg_sgd: a constant of the kernel"""
    return _lib_().vtp_seg_sgd_slice()


def _dense_sgd_workspace_bytes(name, M, N, K):
    return _size_or_raise(getattr(_lib_(), name), M, N, K)


def _dense_sgd(name, w, bias, mw, mb, g, x, lr, M, H, C, K, momentum, workspace):
    _need(workspace, "workspace", torch.uint8, dims=1)
    _need_f32(w=w, bias=bias, mw=mw, mb=mb, g=g, x=x, lr=lr)
    _need_gpu(workspace=workspace)
    _lib.check(getattr(_lib_(), name)(_p(w), _p(bias), _p(mw), _p(mb), _p(g), g.stride(0), _p(x), x.stride(0), _p(lr), M, H, C, K,
                                      momentum, _p(workspace), workspace.numel(), _s()), name)


def seg_sgd_workspace_bytes(M, N, K):
    """bytes of workspace seg_sgd needs for M token rows and N = H * C outputs; ValueError for refused arguments or above 2 GiB"""
    return _dense_sgd_workspace_bytes("vtp_seg_sgd_workspace_bytes", M, N, K)


def seg_sgd(w, bias, mw, mb, g, x, lr, M, H, C, K, momentum, workspace):
    """probe_sgd for M token rows, sliced over the rows and folded in slice order: w [H*C, K], bias [H*C] and their momentum buffers
    updated in place from g [M, >= H*C] and x [M, K] (a column slice); lr f32 [H] on the device"""
    _dense_sgd("vtp_seg_sgd", w, bias, mw, mb, g, x, lr, M, H, C, K, momentum, workspace)


def depth_pix_workspace_bytes(B, h, w, Hl, Wl, H, C, aux=False):
    """bytes of workspace depth_pix needs, or with aux=True bytes of its aux plane; ValueError for refused arguments or above 2 GiB"""
    return _size_or_raise(_lib_().vtp_depth_pix_workspace_bytes, B, h, w, Hl, Wl, H, C, int(bool(aux)))


def _need_aux(aux, B, h, w, Hl, Wl, H, C):
    _need(aux, "aux", torch.uint8, dims=1)
    if aux.numel() < depth_pix_workspace_bytes(B, h, w, Hl, Wl, H, C, aux=True) or aux.data_ptr() % 4:
        raise ValueError("aux is smaller than depth_pix_workspace_bytes(..., aux=True) or not 4-byte aligned")


def depth_pix(z, gt, hw, H, C, min_depth, max_depth, lam, *, out_hw=None, dhat=None, aux=None, loss=None, stats=None, workspace=None,
              eval_counts=None, eval_sums=None):
    """pixel pass of the depth probe: z f32 [B*h*w, >= H*C] low-resolution logits (probe_logits), gt f32 [B, Hl, Wl] -> loss f32 [H]
    and stats f64 [H, 4] = (n, m1, m2, L) (overwritten); optional dhat f32 [H, B, Hl, Wl] (every pixel), aux u8 [depth_pix_workspace_bytes(
    ..., aux=True)] (training), eval_counts int64 [H, 4] and eval_sums f64 [H, 6] (accumulated).  gt=None with out_hw=(Hl, Wl): only
    dhat is written (prediction)"""
    h, w = hw
    if gt is None:
        _need(dhat, "dhat", torch.float32, dims=4)
        B, (Hl, Wl) = dhat.shape[1], out_hw
    else:
        _need(gt, "gt", torch.float32, dims=3)
        B, Hl, Wl = gt.shape
    if dhat is not None:
        _need(dhat, "dhat", torch.float32, (H, B, Hl, Wl))
    if gt is not None:
        _need(loss, "loss", torch.float32, (H,))
        _need(stats, "stats", torch.float64, (H, 4))
        _need(workspace, "workspace", torch.uint8, dims=1)
    if aux is not None:
        _need_aux(aux, B, h, w, Hl, Wl, H, C)
    if eval_counts is not None:
        _need(eval_counts, "eval_counts", torch.int64, (H, 4))
    if eval_sums is not None:
        _need(eval_sums, "eval_sums", torch.float64, (H, 6))
    _need_f32(z=z)
    _need_gpu(gt=gt, dhat=dhat, aux=aux, loss=loss, stats=stats, workspace=workspace, eval_counts=eval_counts, eval_sums=eval_sums)
    _need_token_map(B * h * w, H * C, z=z)
    _lib.check(_lib_().vtp_depth_pix(_p(z), z.stride(0), _p(gt), B, h, w, Hl, Wl, H, C, min_depth, max_depth, lam, _p(dhat), _p(aux),
                                     _p(loss), _p(stats), _p(eval_counts), _p(eval_sums), _p(workspace),
                                     0 if workspace is None else workspace.numel(), _s()), "vtp_depth_pix")


def depth_dlogits(z, label_hw, hw, H, C, min_depth, max_depth, lam, aux, stats, g):
    """cell pass: g f32 [B*h*w, >= H*C] = d L / d z, gathered per cell from aux and stats of depth_pix; label_hw = (B, Hl, Wl)"""
    h, w = hw
    B, Hl, Wl = label_hw
    _need_aux(aux, B, h, w, Hl, Wl, H, C)
    _need(stats, "stats", torch.float64, (H, 4))
    _need_f32(z=z, g=g)
    _need_gpu(aux=aux, stats=stats)
    _need_token_map(B * h * w, H * C, z=z, g=g)
    _lib.check(_lib_().vtp_depth_dlogits(_p(z), z.stride(0), _p(aux), _p(stats), _p(g), g.stride(0), B, h, w, Hl, Wl, H, C, min_depth,
                                         max_depth, lam, _s()), "vtp_depth_dlogits")


def depth_sgd_workspace_bytes(M, N, K):
    """bytes of workspace depth_sgd needs for M token rows and N = H * C outputs; ValueError for refused arguments or above 2 GiB"""
    return _dense_sgd_workspace_bytes("vtp_depth_sgd_workspace_bytes", M, N, K)


def depth_sgd(w, bias, mw, mb, g, x, lr, M, H, C, K, momentum, workspace):
    """seg_sgd for up to 1024 outputs per head: the same kernels, the same bits"""
    _dense_sgd("vtp_depth_sgd", w, bias, mw, mb, g, x, lr, M, H, C, K, momentum, workspace)


def zs_class_mean(feat, wt, C, T, D, eps=1e-12):
    """wt[c] f32 [C, D] = F.normalize(mean over t of feat[c * T + t]) (feat f32 [C * T, D], template t of class c in row c * T + t);
    feat and wt may be row / column slices of wider matrices (row strides taken from the tensors)"""
    _lib.check(_lib_().vtp_zs_class_mean(_p(feat), feat.stride(0), _p(wt), wt.stride(0), C, T, D, eps, _s()), "vtp_zs_class_mean")


def zs_topk(f, wt, targets, scale, B, C, D, counts, per_class=None, rank=None, pred=None, logits=None):
    """logits = (scale * f[B, D]) @ wt[C, D]^T and the top-1 / top-5 statistics of targets int64 [B] in one launch: counts int64 [3]
    += (top-1 hits, top-5 hits, rows); optional per_class i32 [2, C] (accumulated), rank i32 [B], pred i32 [B, 5], logits f32 [B, C]"""
    _lib.check(_lib_().vtp_zs_topk(_p(f), f.stride(0), _p(wt), wt.stride(0), _p(targets), scale, B, C, D, _p(counts), _p(per_class),
                                   _p(rank), _p(pred), _p(logits), 0 if logits is None else logits.stride(0), _s()), "vtp_zs_topk")


KNN_MAX_K = 256


def knn_workspace_bytes(B, K, splits=0):
    """bytes of workspace knn_topk needs for B queries, lists of K and that many splits (0: whatever the heuristic may pick at this
    B); ValueError for arguments the kernel refuses or a workspace above 2 GiB"""
    return _size_or_raise(_lib_().vtp_knn_workspace_bytes, B, K, splits)


def knn_topk(q, x, index_base, K, sims, idx, workspace, splits=0, sims_out=None):
    """merges the bank chunk x f32 [N, D] (global index of its row 0: index_base) into the neighbour lists sims f32 [B, K] / idx
    int64 [B, K] of the queries q f32 [B, D]: the first K bank rows by (similarity descending, index ascending), empty entries
    (-inf, -1) last; similarities with the bits of gemm_nt_f32(q, x).  q and x may be column slices of wider matrices (row strides
    from the tensors).  workspace: uint8, knn_workspace_bytes(B, K, splits) bytes.  sims_out f32 [B, N]: the chunk's similarities."""
    for name, t, dt in (("q", q, torch.float32), ("x", x, torch.float32), ("sims", sims, torch.float32), ("idx", idx, torch.int64),
                        ("workspace", workspace, torch.uint8), ("sims_out", sims_out, torch.float32)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt):
            raise ValueError(f"{name} must be a {dt} tensor, got {getattr(t, 'dtype', type(t))}")
    _need_gpu(q=q, x=x, sims=sims, idx=idx, workspace=workspace, sims_out=sims_out)
    if q.dim() != 2 or x.dim() != 2 or q.shape[1] != x.shape[1] or q.stride(1) != 1 or x.stride(1) != 1:
        raise ValueError(f"q and x must be [B, D] and [N, D] with unit column stride, got {tuple(q.shape)} and {tuple(x.shape)}")
    B, D = q.shape
    N = x.shape[0]
    _need(sims, "sims", torch.float32, (B, K))
    _need(idx, "idx", torch.int64, (B, K))
    if sims_out is not None and (tuple(sims_out.shape) != (B, N) or sims_out.stride(1) != 1):
        raise ValueError(f"sims_out must be [{B}, {N}] with unit column stride, got {tuple(sims_out.shape)}")
    _lib.check(_lib_().vtp_knn_topk(_p(q), q.stride(0), _p(x), x.stride(0), int(index_base), B, N, D, K, _p(sims), _p(idx),
                                    _p(workspace), workspace.numel(), splits, _p(sims_out),
                                    0 if sims_out is None else sims_out.stride(0), _s()), "vtp_knn_topk")


def knn_vote(sims, idx, labels, targets, ks, inv_T, num_classes, counts=None, rank_out=None, pred_out=None):
    """the weighted vote over neighbour lists sims f32 [B, K] / idx int64 [B, K] (knn_topk): labels int32 [N_total] of the bank rows,
    targets int64 [B], ks ascending ints <= K (at most 8): counts int64 [nk, 3] += (top-1 hits, top-5 hits, rows); optional
    rank_out int32 [B, nk] (classes ranked before the target; num_classes for a target out of range), pred_out int32 [B, nk, 5]"""
    import ctypes
    _need(sims, "sims", torch.float32, dims=2)
    B, K = sims.shape
    ks = [int(k) for k in ks]
    nk = len(ks)
    _need(idx, "idx", torch.int64, (B, K))
    _need(labels, "labels", torch.int32, dims=1)
    _need(targets, "targets", torch.int64, (B,))
    if counts is not None:
        _need(counts, "counts", torch.int64, (nk, 3))
    if rank_out is not None:
        _need(rank_out, "rank_out", torch.int32, (B, nk))
    if pred_out is not None:
        _need(pred_out, "pred_out", torch.int32, (B, nk, 5))
    _need_gpu(sims=sims, idx=idx, labels=labels, targets=targets, counts=counts, rank_out=rank_out, pred_out=pred_out)
    ks_c = (ctypes.c_int * max(nk, 1))(*ks)
    _lib.check(_lib_().vtp_knn_vote(_p(sims), _p(idx), _p(labels), labels.numel(), _p(targets), ctypes.cast(ks_c, ctypes.c_void_p), nk,
                                    inv_T, num_classes, B, K, _p(counts), _p(rank_out), _p(pred_out), _s()), "vtp_knn_vote")


PR_MAX_K = 8


def _pr_rows(**tensors):
    """f32 [n, D] matrices with unit column stride (row strides go to the kernel); the device is checked by _need_gpu, last"""
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a {torch.float32} tensor, got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{name} must be [n, D] with unit column stride, got {tuple(t.shape)} with strides {t.stride()}")


def pr_workspace_bytes(B, splits=0):
    """bytes of workspace pr_knn_dist needs for B queries and that many splits (0: whatever the heuristic may pick at this B):
    splits * B * 32; ValueError for arguments the kernel refuses or a workspace above 2 GiB"""
    return _size_or_raise(_lib_().vtp_pr_workspace_bytes, B, splits)


def pr_sqnorm(x, out):
    """out f32 [N] = the squared norm of every row of x f32 [N, D]: one fmaf chain over k ascending, the bits of the diagonal of
    gemm_nt_f32(x, x).  x may be a column slice of a wider matrix."""
    _pr_rows(x=x)
    N, D = x.shape
    _need(out, "out", torch.float32, (N,))
    _need_gpu(x=x, out=out)
    _lib.check(_lib_().vtp_pr_sqnorm(_p(x), x.stride(0), N, D, _p(out), _s()), "vtp_pr_sqnorm")


def pr_knn_dist(q, qn, x, xn, dist, workspace, query_base=-1, index_base=0, splits=0, d2_out=None):
    """merges the bank chunk x f32 [N, D] (norms xn f32 [N], global index of its row 0: index_base) into dist f32 [B, PR_MAX_K]: per
    query of q f32 [B, D] (norms qn f32 [B]) the 8 smallest d2 = max(qn + xn - 2 q.x, 0) seen so far, ascending, +inf for an empty
    entry (fill dist with +inf before the first chunk).  query_base >= 0: the pair with query_base + b == index_base + n is skipped
    (a set against itself); -1: no exclusion.  q and x may be column slices of wider matrices.  workspace: uint8,
    pr_workspace_bytes(B, splits) bytes.  d2_out f32 [B, N]: the chunk's distances."""
    _pr_rows(q=q, x=x)
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"q and x must be [B, D] and [N, D], got {tuple(q.shape)} and {tuple(x.shape)}")
    B, D = q.shape
    N = x.shape[0]
    _need(qn, "qn", torch.float32, (B,))
    _need(xn, "xn", torch.float32, (N,))
    _need(dist, "dist", torch.float32, (B, PR_MAX_K))
    _need(workspace, "workspace", torch.uint8, dims=1)
    if d2_out is not None:
        _pr_rows(d2_out=d2_out)
        if tuple(d2_out.shape) != (B, N):
            raise ValueError(f"d2_out must be [{B}, {N}], got {tuple(d2_out.shape)}")
    _need_gpu(q=q, qn=qn, x=x, xn=xn, dist=dist, workspace=workspace, d2_out=d2_out)
    _lib.check(_lib_().vtp_pr_knn_dist(_p(q), q.stride(0), _p(qn), _p(x), x.stride(0), _p(xn), int(query_base), int(index_base), B, N, D,
                                       _p(dist), _p(workspace), workspace.numel(), splits, _p(d2_out),
                                       0 if d2_out is None else d2_out.stride(0), _s()), "vtp_pr_knn_dist")


def pr_cover(q, qn, x, xn, r2, hits, splits=0):
    """hits int32 [B] += per query of q f32 [B, D] (norms qn) the number of rows n of the bank chunk x f32 [N, D] (norms xn) with
    d2(q_b, x_n) <= r2[n] (r2 f32 [N]: the squared radii of the bank rows); integer atomics only"""
    _pr_rows(q=q, x=x)
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"q and x must be [B, D] and [N, D], got {tuple(q.shape)} and {tuple(x.shape)}")
    B, D = q.shape
    N = x.shape[0]
    _need(qn, "qn", torch.float32, (B,))
    _need(xn, "xn", torch.float32, (N,))
    _need(r2, "r2", torch.float32, (N,))
    _need(hits, "hits", torch.int32, (B,))
    _need_gpu(q=q, qn=qn, x=x, xn=xn, r2=r2, hits=hits)
    _lib.check(_lib_().vtp_pr_cover(_p(q), q.stride(0), _p(qn), _p(x), x.stride(0), _p(xn), _p(r2), B, N, D, _p(hits), splits, _s()),
               "vtp_pr_cover")


MMD_TILE = 128  # bank rows per tile of mmd_poly_part: index_base is a multiple of it
MMD_MAX_DEGREE = 8


def mmd_workspace_bytes(B, N, P=1):
    """bytes of the part buffer of mmd_poly_part for B queries, N bank rows and P problems: P * ceil(N / 128) * B * 8; ValueError for
    arguments the kernel refuses or a buffer above 2 GiB"""
    return _size_or_raise(_lib_().vtp_mmd_workspace_bytes, B, N, P)


def mmd_poly_part(q, x, part, gamma, coef0=1.0, degree=3, query_base=-1, index_base=0, qi=None, xi=None):
    """part f64 [P, tiles, B] (tiles = ceil(N / 128)): per problem, bank tile and query the sum of (gamma q.x + coef0)^degree over the
    tile's rows, the products with the bits of gemm_nt_f32 and everything after in fp64, in the fixed order of csrc/mmd.hip.  q f32
    [., D] / x f32 [., D] may be column slices of wider matrices.  qi int32 [P, B] / xi int32 [P, N] on the device (None: identity, q is
    [B, D] / x is [N, D]) pick the rows of q / x that a problem's queries / bank rows are.  query_base >= 0: the pair with query_base
    + b == index_base + n (positions in the lists) is skipped; -1: no exclusion.  index_base: a multiple of 128."""
    import ctypes
    _pr_rows(q=q, x=x)
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"q and x must be [., D] and [., D], got {tuple(q.shape)} and {tuple(x.shape)}")
    D = q.shape[1]
    _need(part, "part", torch.float64, dims=3)
    P = part.shape[0]
    if qi is not None:
        _need(qi, "qi", torch.int32, dims=2)
    if xi is not None:
        _need(xi, "xi", torch.int32, dims=2)
    B = q.shape[0] if qi is None else qi.shape[1]
    N = x.shape[0] if xi is None else xi.shape[1]
    for name, t in (("qi", qi), ("xi", xi)):
        if t is not None and t.shape[0] != P:
            raise ValueError(f"{name} must hold one list per problem ({P}, the first dimension of part), got {tuple(t.shape)}")
    tiles = (N + MMD_TILE - 1) // MMD_TILE
    if tuple(part.shape) != (P, tiles, B):
        raise ValueError(f"part must be [P, {tiles}, {B}], got {tuple(part.shape)}")
    _need_gpu(q=q, x=x, part=part, qi=qi, xi=xi)
    kparams = (ctypes.c_double * 2)(float(gamma), float(coef0))
    _lib.check(_lib_().vtp_mmd_poly_part(_p(q), q.stride(0), q.shape[0], _p(qi), _p(x), x.stride(0), x.shape[0], _p(xi), int(query_base),
                                         int(index_base), B, N, D, P, ctypes.cast(kparams, ctypes.c_void_p), int(degree), _p(part),
                                         part.numel() * 8, _s()), "vtp_mmd_poly_part")


def mmd_fold(part, rowsum):
    """rowsum f64 [P, B] += part f64 [P, tiles, B] summed over the tiles in ascending order, one owner thread per element"""
    _need(part, "part", torch.float64, dims=3)
    P, tiles, B = part.shape
    _need(rowsum, "rowsum", torch.float64, (P, B))
    _need_gpu(part=part, rowsum=rowsum)
    _lib.check(_lib_().vtp_mmd_fold(_p(part), _p(rowsum), B, tiles, P, _s()), "vtp_mmd_fold")


def mmd_total(rowsum, total):
    """total f64 [P] = the sum of each row of rowsum f64 [P, B] by the tree that pairs neighbours level by level: its shape depends
    on B alone"""
    _need(rowsum, "rowsum", torch.float64, dims=2)
    P, B = rowsum.shape
    _need(total, "total", torch.float64, (P,))
    _need_gpu(rowsum=rowsum, total=total)
    _lib.check(_lib_().vtp_mmd_total(_p(rowsum), B, P, _p(total), _s()), "vtp_mmd_total")


RETR_MAX_KS = 8  # recall levels per retr_count call


def retr_best(q, x, gt_ptr, gt_idx, best_s, best_j):
    """per query of q f32 [B, D] the best of its ground-truth rows in the whole gallery x f32 [N, D]: best_s f32 [B] and best_j int64
    [B], the first under (similarity descending, row ascending); (-inf, -1) for an empty list.  The lists are a CSR: gt_ptr int32
    [B + 1] ascending, gt_idx int64 [nnz] gallery rows (one outside [0, N) is ignored).  Similarities with the bits of
    gemm_nt_f32(q, x).  q and x may be column slices of wider matrices."""
    _pr_rows(q=q, x=x)
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"q and x must be [B, D] and [N, D], got {tuple(q.shape)} and {tuple(x.shape)}")
    B, D = q.shape
    N = x.shape[0]
    _need(gt_ptr, "gt_ptr", torch.int32, (B + 1,))
    _need(gt_idx, "gt_idx", torch.int64, dims=1)
    _need(best_s, "best_s", torch.float32, (B,))
    _need(best_j, "best_j", torch.int64, (B,))
    _need_gpu(q=q, x=x, gt_ptr=gt_ptr, gt_idx=gt_idx, best_s=best_s, best_j=best_j)
    nnz = gt_idx.numel()
    _lib.check(_lib_().vtp_retr_best(_p(q), q.stride(0), _p(x), x.stride(0), N, _p(gt_ptr), _p(gt_idx) if nnz else None, nnz, B, D,
                                     _p(best_s), _p(best_j), _s()), "vtp_retr_best")


def retr_rank(q, x, index_base, best_s, best_j, beats, splits=0, sims_out=None):
    """beats int32 [B] += per query of q f32 [B, D] the number of rows of the gallery chunk x f32 [N, D] (global index of its row 0:
    index_base) strictly before (best_s[b], best_j[b]) under (similarity descending, global row ascending); best_j[b] == -1 counts
    every row.  Integer atomics only.  sims_out f32 [B, N]: the chunk's similarities (the bits of gemm_nt_f32(q, x))."""
    _pr_rows(q=q, x=x)
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"q and x must be [B, D] and [N, D], got {tuple(q.shape)} and {tuple(x.shape)}")
    B, D = q.shape
    N = x.shape[0]
    _need(best_s, "best_s", torch.float32, (B,))
    _need(best_j, "best_j", torch.int64, (B,))
    _need(beats, "beats", torch.int32, (B,))
    if sims_out is not None:
        _pr_rows(sims_out=sims_out)
        if tuple(sims_out.shape) != (B, N):
            raise ValueError(f"sims_out must be [{B}, {N}], got {tuple(sims_out.shape)}")
    _need_gpu(q=q, x=x, best_s=best_s, best_j=best_j, beats=beats, sims_out=sims_out)
    _lib.check(_lib_().vtp_retr_rank(_p(q), q.stride(0), _p(x), x.stride(0), int(index_base), B, N, D, _p(best_s), _p(best_j), _p(beats),
                                     splits, _p(sims_out), 0 if sims_out is None else sims_out.stride(0), _s()), "vtp_retr_rank")


def retr_count(beats, ks, counts, rank=None, rank_offset=0):
    """counts int64 [nk + 1] += (#{beats < k} for k of ks, rows); ks ascending positive ints (at most 8).  rank int32 [>= rank_offset
    + B]: rank[rank_offset + b] = beats[b]."""
    import ctypes
    _need(beats, "beats", torch.int32, dims=1)
    B = beats.shape[0]
    ks = [int(k) for k in ks]
    nk = len(ks)
    _need(counts, "counts", torch.int64, (nk + 1,))
    if rank is not None:
        _need(rank, "rank", torch.int32, dims=1)
        if rank_offset < 0 or rank_offset + B > rank.shape[0]:
            raise ValueError(f"rank holds {rank.shape[0]} entries, rows {rank_offset} .. {rank_offset + B} asked for")
    _need_gpu(beats=beats, counts=counts, rank=rank)
    ks_c = (ctypes.c_int * max(nk, 1))(*ks)
    _lib.check(_lib_().vtp_retr_count(_p(beats), B, ctypes.cast(ks_c, ctypes.c_void_p), nk, _p(counts), _p(rank), int(rank_offset), _s()),
               "vtp_retr_count")


IS_ONE_SPLIT = (1 << 63) - 1  # split_size of is_accum for "one split over everything"


def is_rows(logits, C, p, h):
    """per row of logits f32 [B, ld >= C] (unit column stride; only the columns c < C count) the softmax p f64 [B, C] and
    h f64 [B] = sum_c p_c (l_c - lse) in fp64 (vtp_is_rows): one wave per row, a row's bits depend on that row alone"""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be an f32 [B, >= C] tensor with unit column stride")
    B = logits.shape[0]
    if not 1 <= C <= logits.shape[1]:
        raise ValueError(f"C must be 1 .. {logits.shape[1]} (the width of logits), got {C}")
    _need(p, "p", torch.float64, (B, C))
    _need(h, "h", torch.float64, (B,))
    _need_gpu(logits=logits, p=p, h=h)
    _lib.check(_lib_().vtp_is_rows(_p(logits), logits.stride(0), B, C, _p(p), p.stride(0), _p(h), _s()), "vtp_is_rows")


def is_accum(p, h, state, row_base, split_size=None):
    """adds the rows of p f64 [B, C] and h f64 [B], global rows row_base .. row_base + B - 1, to the slots [H | S_0 .. S_C-1] of
    state f64 [n_slots, 1 + C]: row r goes to slot r // split_size (None: slot 0), rows in order, one thread per element
    (vtp_is_accum): any split of the same rows over calls leaves the same bits"""
    _need(p, "p", torch.float64, dims=2)
    B, C = p.shape
    _need(h, "h", torch.float64, (B,))
    _need(state, "state", torch.float64, dims=2)
    if state.shape[1] != 1 + C:
        raise ValueError(f"state must be [n_slots, 1 + C = {1 + C}], got {tuple(state.shape)}")
    _need_gpu(p=p, h=h, state=state)
    _lib.check(_lib_().vtp_is_accum(_p(p), p.stride(0), _p(h), int(row_base), IS_ONE_SPLIT if split_size is None else int(split_size),
                                    B, C, _p(state), state.shape[0], _s()), "vtp_is_accum")


def recon_scratch_size(B, H, W):
    """number of f64 elements the scratch of recon_metrics / recon_finalize must hold for a [B, 3, H, W] batch (two per tile of
    window positions); ValueError for a shape the kernels refuse (H or W below 11, W % 4 != 0, B < 1)"""
    return _size_or_raise(_lib_().vtp_recon_scratch_doubles, B, H, W)


def recon_metrics(images, recon, sub, div, scratch, ref_u8=None, rec_u8=None, ref_lp=None, rec_lp=None):
    """one launch over images / recon f32 [B, 3, H, W] (contiguous): with d = clamp((x - sub[c]) / div[c], 0, 1), optional byte
    images uint8 [B, H, W, 3] = trunc(d * 255) and LPIPS inputs f32 [B, 3, H, W] = d * 2 - 1, and the per-tile squared-error and
    SSIM partials in scratch (f64, recon_scratch_size elements)"""
    B, _, H, W = images.shape
    _lib.check(_lib_().vtp_recon_metrics(_p(images), _p(recon), B, H, W, _f3(sub), _f3(div), _p(ref_u8), _p(rec_u8), _p(ref_lp),
                                         _p(rec_lp), _p(scratch), scratch.numel(), _s()), "vtp_recon_metrics")


def recon_finalize(scratch, B, H, W, psnr, ssim, acc, sse=None, lpips=None):
    """psnr / ssim f32 [B] (and sse f64 [B]) from the partials of recon_metrics, tiles summed in a fixed order; acc f64 [8] +=
    (sum psnr, images, images with sse == 0, sum ssim, sum of batch-mean ssim, batches, sum of batch-mean lpips, sum lpips)"""
    _lib.check(_lib_().vtp_recon_finalize(_p(scratch), scratch.numel(), B, H, W, _p(psnr), _p(ssim), _p(sse), _p(lpips), _p(acc), _s()),
               "vtp_recon_finalize")


def augment_scratch_size(N, S):
    """number of f32 elements the scratch of augment_crops must hold for N crops of S x S (the resampled crops and the per-tile
    gray sums); ValueError for a shape the kernels refuse (N < 1, S < 5)"""
    return _size_or_raise(_lib_().vtp_augment_scratch_floats, N, S)


def augment_crops(u8_nhwc, table, out, mean, std, scratch):
    """uint8 [B, Hs, Ws, 3] -> out f32 [N, 3, S, S] (N = views * B, crop n from image n % B), one row of table f32 [N, 16] (device)
    per crop: resized crop, flip, colour jitter, grayscale, blur, solarize, normalise (csrc/augment.hip); two launches"""
    B, Hs, Ws, _ = u8_nhwc.shape
    N, _, S, _ = out.shape
    _lib.check(_lib_().vtp_augment_crops(_p(u8_nhwc), B, Hs, Ws, _p(table), N, S, _f3(mean), _f3(std), _p(out), _p(scratch),
                                         scratch.numel(), _s()), "vtp_augment_crops")


def preprocess(src_u8, scratch, jobs, tab, launches, out, out_u8, mean, std):
    """PIL's 8-bit resize / crop / flip + ToTensor + Normalize over a ragged batch (csrc/preprocess.hip): src_u8 uint8 [bytes] and
    scratch uint8 [bytes] on the device, jobs int64 [n * 16] and tab int32 on the device, launches int32 [L, 3] numpy on the host
    -> out f32 [B, 3, Ho, Wo] (and out_u8 uint8 [B, Ho, Wo, 3] unless None); one launch per row of launches.  The job rows must have
    passed vtp_amd.preprocess.check_jobs: the kernels cannot refuse a bad offset."""
    import ctypes
    import numpy as np
    ln = np.ascontiguousarray(launches, dtype=np.int32)
    B, _, Ho, Wo = out.shape
    _lib.check(_lib_().vtp_preprocess(_p(src_u8), src_u8.numel(), _p(scratch), 0 if scratch is None else scratch.numel(), _p(jobs),
                                      _p(tab), ln.ctypes.data_as(ctypes.c_void_p), len(ln), B, Ho, Wo, _f3(mean), _f3(std), _p(out),
                                      _p(out_u8), _s()), "vtp_preprocess")


POOL_MAX, POOL_AVG, POOL_AVG_INSIDE = 0, 1, 2  # vtp_pool3x3_f32 modes: max; average / 9; average over the taps inside the image


def conv_out_size(H, W, kh, kw, stride, ph, pw):
    return (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1


def _need(t, name, dtype, shape=None, dims=None):
    """the C entry points see pointers only: dtype, shape and contiguity of a tensor are checked here (the device by _need_gpu, last)"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"{name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{name} must have {dims} dimensions, got {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous, got strides {t.stride()} for {tuple(t.shape)}")


def _need_gpu(**tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise ValueError(f"{name} must live on the MI355X (got a CPU tensor): there is no CPU path")


def conv2d_f32(x, w, bias, y, stride=1, pad=(0, 0), relu=True, c0=0, blocked=False):
    """exact-fp32 implicit-GEMM convolution (csrc/fid.hip): x f32 NHWC [B, H, W, Cin], w f32 [Cout, kh, kw, Cin], bias f32 [Cout] or
    None -> the channels [c0, c0 + Cout) of y f32 [B, Ho, Wo, Ctot]; every output is one fmaf chain over (ky, kx, ci) -- with
    blocked=True a chain per 32 consecutive k whose sums are added in k order (vtp_conv2d_f32_blocked: long reductions)"""
    _need(x, "x", torch.float32, dims=4)
    B, H, W, Cin = x.shape
    _need(w, "w", torch.float32, dims=4)
    Cout, kh, kw, wc = w.shape
    if wc != Cin:
        raise ValueError(f"w must be [Cout, kh, kw, Cin = {Cin}] like x, got {tuple(w.shape)}")
    if bias is not None:
        _need(bias, "bias", torch.float32, (Cout,))
    ho, wo = conv_out_size(H, W, kh, kw, stride, pad[0], pad[1])
    _need(y, "y", torch.float32, dims=4)
    if tuple(y.shape[:3]) != (B, ho, wo) or c0 < 0 or c0 + Cout > y.shape[3]:
        raise ValueError(f"y must be [{B}, {ho}, {wo}, Ctot >= c0 + Cout = {c0 + Cout}], got {tuple(y.shape)}")
    _need_gpu(x=x, w=w, bias=bias, y=y)
    fn, name = (_lib_().vtp_conv2d_f32_blocked, "vtp_conv2d_f32_blocked") if blocked else (_lib_().vtp_conv2d_f32, "vtp_conv2d_f32")
    _lib.check(fn(_p(x), _p(w), _p(bias), _p(y), B, H, W, Cin, Cout, kh, kw, stride, pad[0], pad[1], int(bool(relu)), c0, y.shape[3], _s()),
               name)


def pool3x3_f32(x, y, stride, mode, c0=0):
    """3 x 3 pooling of x f32 NHWC [B, H, W, C] into the channels [c0, c0 + C) of y f32 [B, Ho, Wo, Ctot]: stride 1 pads by 1, stride 2
    by 0; mode POOL_MAX / POOL_AVG / POOL_AVG_INSIDE"""
    _need(x, "x", torch.float32, dims=4)
    B, H, W, C = x.shape
    ho, wo = (H, W) if stride == 1 else ((H - 3) // 2 + 1, (W - 3) // 2 + 1)
    _need(y, "y", torch.float32, dims=4)
    if tuple(y.shape[:3]) != (B, ho, wo) or c0 < 0 or c0 + C > y.shape[3]:
        raise ValueError(f"y must be [{B}, {ho}, {wo}, Ctot >= c0 + C = {c0 + C}], got {tuple(y.shape)}")
    _need_gpu(x=x, y=y)
    _lib.check(_lib_().vtp_pool3x3_f32(_p(x), _p(y), B, H, W, C, stride, mode, c0, y.shape[3], _s()), "vtp_pool3x3_f32")


def global_avgpool_f32(x, y):
    """x f32 NHWC [B, H, W, C] -> y f32 [B, C]"""
    _need(x, "x", torch.float32, dims=4)
    B, H, W, C = x.shape
    _need(y, "y", torch.float32, (B, C))
    _need_gpu(x=x, y=y)
    _lib.check(_lib_().vtp_global_avgpool_f32(_p(x), _p(y), B, H * W, C, _s()), "vtp_global_avgpool_f32")


def resize_bilinear_nhwc(x, y, scale=1.0, shift=0.0):
    """x f32 NCHW [B, C, H, W] -> y f32 NHWC [B, Ho, Wo, C] = scale * F.interpolate(x, (Ho, Wo), 'bilinear', align_corners=False) +
    shift; at equal sizes the NCHW -> NHWC repack"""
    _need(x, "x", torch.float32, dims=4)
    B, C, H, W = x.shape
    _need(y, "y", torch.float32, dims=4)
    if y.shape[0] != B or y.shape[3] != C:
        raise ValueError(f"y must be [{B}, Ho, Wo, {C}], got {tuple(y.shape)}")
    _need_gpu(x=x, y=y)
    _lib.check(_lib_().vtp_resize_bilinear_nhwc(_p(x), _p(y), B, C, H, W, y.shape[1], y.shape[2], scale, shift, _s()),
               "vtp_resize_bilinear_nhwc")


def fid_accum(feats, sum_, outer):
    """adds the rows of feats f32 [n, D] (row stride >= D), in order, to sum_ f64 [D] and outer f64 [D, D] (x and x x^T); one launch"""
    if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float32 or feats.dim() != 2 or feats.stride(1) != 1 \
            or feats.stride(0) < feats.shape[1]:
        raise ValueError("feats must be an f32 [n, D] tensor with unit column stride and a row stride >= D")
    n, D = feats.shape
    _need(sum_, "sum_", torch.float64, (D,))
    _need(outer, "outer", torch.float64, (D, D))
    _need_gpu(feats=feats, sum_=sum_, outer=outer)
    _lib.check(_lib_().vtp_fid_accum(_p(feats), feats.stride(0), _p(sum_), _p(outer), n, D, _s()), "vtp_fid_accum")


# ---- fp32 inference forward (fp32.hip): every tensor f32, products on the f32-input MFMA, one fmaf chain per output element
F32_PLAIN, F32_RESID, F32_SWIGLU, F32_GELU, F32_QUICK_GELU = 0, 1, 2, 3, 4


def _need_f32(**tensors):
    for name, t in tensors.items():
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda):
            raise ValueError(f"{name} must be a float32 tensor on the device, got {t.dtype} on {t.device}")


def gemm_nt_f32(a, w, c, *, M=None, N=None, K=None, lda=None, ldw=None, ldc=None, w2=None, bias=None, bias2=None, gamma=None,
                resid=None, ldr=None, epi=F32_PLAIN):
    """c[M,N] = epi(a[M,K] @ w[N,K]^T) in exact fp32 (vtp_gemm_nt_f32): a, w, c f32, K-contiguous rows with leading dimensions.
    epi F32_RESID: resid + gamma * (. + bias); F32_SWIGLU: silu(a w^T + bias) * (a w2^T + bias2); F32_GELU / F32_QUICK_GELU."""
    _need_f32(a=a, w=w, c=c, w2=w2, bias=bias, bias2=bias2, gamma=gamma, resid=resid)
    M = a.shape[0] if M is None else M
    K = a.shape[1] if K is None else K
    N = w.shape[0] if N is None else N
    lda = a.stride(0) if lda is None else lda
    ldw = w.stride(0) if ldw is None else ldw
    ldc = c.stride(0) if ldc is None else ldc
    if resid is not None and ldr is None:
        ldr = resid.stride(0)
    _lib.check(_lib_().vtp_gemm_nt_f32(_p(a), lda, _p(w), ldw, _p(w2), _p(c), ldc, _p(bias), _p(bias2), _p(gamma), _p(resid), ldr or 0,
                                       M, N, K, epi, _s()), "vtp_gemm_nt_f32")


def attn_fwd_f32(q, k, v, o, B, N, heads, sb, sn, sbo, sno, scale, causal=False):
    """o = softmax(scale q k^T) v, head dimension 64, all f32 (vtp_attn_fwd_f32); strides in elements as attn_fwd"""
    _need_f32(q=q, k=k, v=v, o=o)
    _lib.check(_lib_().vtp_attn_fwd_f32(_p(q), _p(k), _p(v), _p(o), B, N, heads, sb, sn, sbo, sno, scale, int(causal), _s()),
               "vtp_attn_fwd_f32")


def norm_fwd_f32(x, w, b, y, stats, M, D, eps, kind):
    """norm_fwd with the un-rounded f32 output y"""
    _need_f32(x=x, w=w, b=b, y=y, stats=stats)
    _lib.check(_lib_().vtp_norm_fwd_f32(_p(x), _p(w), _p(b), _p(y), _p(stats), M, D, eps, kind, _s()), "vtp_norm_fwd_f32")


def rope_qk_f32(qkv, sin, cos, B, N, heads, prefix):
    """apply_rope in place on the q and k thirds of qkv f32 [B*N, 3*heads*64]: rounded to bf16, rotated as rope_qk, widened back"""
    _need_f32(qkv=qkv)
    assert sin.dtype == torch.bfloat16 and cos.dtype == torch.bfloat16
    _lib.check(_lib_().vtp_rope_qk_f32(_p(qkv), _p(sin), _p(cos), B, N, heads, prefix, _s()), "vtp_rope_qk_f32")


def im2col16_rows_f32(img, rows, B, H, W, prefix=1):
    _need_f32(img=img, rows=rows)
    _lib.check(_lib_().vtp_im2col16_rows_f32(_p(img), _p(rows), B, H, W, prefix, _s()), "vtp_im2col16_rows_f32")


def pixel_shuffle16_f32(t, img, B, h, w):
    _need_f32(t=t, img=img)
    _lib.check(_lib_().vtp_pixel_shuffle16_f32(_p(t), _p(img), B, h, w, _s()), "vtp_pixel_shuffle16_f32")


def pool_patch_rows_f32(x, out, B, N, D, scale=None):
    """pool_patch_rows on f32 token rows"""
    _need_f32(x=x, out=out)
    assert x.is_contiguous() and x.numel() >= B * N * D and out.is_contiguous() and out.numel() >= B * D
    s = 1.0 / (N - 1) if scale is None else float(scale)
    _lib.check(_lib_().vtp_pool_patch_rows_f32(_p(x), _p(out), B, N, D, s, _s()), "vtp_pool_patch_rows_f32")


# ---- LPIPS in fp32 (lpips_f32.hip): f32 NHWC activations without borders around conv2d_f32
LPIPS_HEAD_SEG = 256  # pixels per partial sum of lpips_head_f32


def lpips_head_segments(HW):
    return (HW + LPIPS_HEAD_SEG - 1) // LPIPS_HEAD_SEG


def lpips_scale_nhwc_f32(x, y, shift, scale):
    """ScalingLayer + repack: x f32 NCHW [B, 3, H, W] -> y f32 NHWC [B, H, W, 3 or 4] = (x - shift_c) / scale_c (one subtraction, one
    division: torch's bits); a fourth channel is written as zeros"""
    _need(x, "x", torch.float32, dims=4)
    B, C, H, W = x.shape
    if C != 3:
        raise ValueError(f"x must be [B, 3, H, W], got {tuple(x.shape)}")
    _need(y, "y", torch.float32, dims=4)
    if tuple(y.shape[:3]) != (B, H, W) or y.shape[3] not in (3, 4):
        raise ValueError(f"y must be [{B}, {H}, {W}, 3 or 4], got {tuple(y.shape)}")
    _need_gpu(x=x, y=y)
    _lib.check(_lib_().vtp_lpips_scale_nhwc_f32(_p(x), _p(y), B, H, W, y.shape[3], _f3(shift), _f3(scale), _s()),
               "vtp_lpips_scale_nhwc_f32")


def maxpool2_f32(x, y):
    """F.max_pool2d(., 2, 2) on f32 NHWC: x [B, H, W, C] -> y [B, H / 2, W / 2, C]; H, W even, C % 4 == 0"""
    _need(x, "x", torch.float32, dims=4)
    B, H, W, C = x.shape
    if H % 2 or W % 2 or C % 4:
        raise ValueError(f"x must be [B, H, W, C] with H, W even and C a multiple of 4, got {tuple(x.shape)}")
    _need(y, "y", torch.float32, (B, H // 2, W // 2, C))
    _need_gpu(x=x, y=y)
    _lib.check(_lib_().vtp_maxpool2_f32(_p(x), _p(y), B, H, W, C, _s()), "vtp_maxpool2_f32")


def lpips_head_f32(f, w, part):
    """one LPIPS tap in fp32: f f32 NHWC [2 n, H, W, C] (features of image b and of image n + b), w f32 [C] -> part f64
    [n, lpips_head_segments(H W)]: per pair the fp64 sums of the per-pixel distances over segments of 256 pixels"""
    _need(f, "f", torch.float32, dims=4)
    NB, H, W, C = f.shape
    if NB % 2:
        raise ValueError(f"f must hold 2 n images (n of the input, then n of the target), got {tuple(f.shape)}")
    _need(w, "w", torch.float32, (C,))
    _need(part, "part", torch.float64, (NB // 2, lpips_head_segments(H * W)))
    _need_gpu(f=f, w=w, part=part)
    _lib.check(_lib_().vtp_lpips_head_f32(_p(f), _p(w), _p(part), NB // 2, H * W, C, _s()), "vtp_lpips_head_f32")


def lpips_finalize_f32(part, val, n, H, W):
    """val f32 [n] = (((r_0 + r_1) + r_2) + r_3) + r_4, r_k = float(sum of tap k's segment sums / (H_k W_k)); part f64 = the five
    [n, segments_k] blocks of lpips_head_f32 back to back for an H x W input"""
    total = n * sum(lpips_head_segments((H >> k) * (W >> k)) for k in range(5))
    _need(part, "part", torch.float64, (total,))
    _need(val, "val", torch.float32, (n,))
    _need_gpu(part=part, val=val)
    _lib.check(_lib_().vtp_lpips_finalize_f32(_p(part), _p(val), n, H, W, _s()), "vtp_lpips_finalize_f32")
