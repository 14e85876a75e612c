"""ctypes binding of libvtp_hip.so (include/vtp_hip.h).  The product path has NO fallback: if the library is
missing or a call is rejected, a RuntimeError is raised (never a silent eager/CPU path)."""
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_long, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VTP_HIP_LIB") or os.path.join(_HERE, "lib", "libvtp_hip.so")  # override: A/B runs of two builds

_P, _I, _L, _F = c_void_p, c_int, c_long, c_float

# name -> argtypes (must mirror include/vtp_hip.h exactly; tests/test_abi.py checks the export list)
SIGNATURES = {
    "vtp_gemm_nt": [_P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P],
    "vtp_norm_fwd": [_P, _P, _P, _P, _P, _I, _I, _F, _I, _P],
    "vtp_norm_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],  # dy x w stats dres dx dxb dw db dxsum M D kind stream
    # ... + pvec prow0 pB pN in front of M
    "vtp_norm_bwd_pvec": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "vtp_norm_bwd_rows": [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P],  # ... dres dres_rows dres_M dx ...
    "vtp_pool_patch_rows": [_P, _P, _I, _I, _I, _F, _P],
    "vtp_rope_qk": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vtp_attn_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _L, _F, _I, _P],
    "vtp_attn_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _L, _L, _L, _L, _F, _I, _P],
    "vtp_im2col16": [_P, _P, _I, _I, _I, _P],
    "vtp_im2col16_rows": [_P, _P, _I, _I, _I, _I, _P],
    "vtp_col2im16": [_P, _P, _I, _I, _I, _P],
    "vtp_assemble_tokens": [_P, _P, _P, _P, _I, _I, _I, _P],
    "vtp_transpose_bf16": [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P],  # in ld out ld colsum swiglu_h in_grp in_pre R C stream
    "vtp_strided_rowsum": [_P, _L, _P, _I, _I, _P],
    "vtp_mask_rows_bwd": [_P, _P, _P, _P, _I, _I, _I, _P],
    "vtp_token_rows_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "vtp_cast_f32_bf16": [_P, _P, _L, _P],
    "vtp_cast_transpose_f32_bf16": [_P, _P, _I, _I, _P],
    "vtp_prep_weights": [_P, _I, _I, _P],
    "vtp_prep_weights_range": [_P, _I, _I, _I, _P],
    "vtp_swiglu_bwd": [_P, _P, _P, _P, _I, _I, _P],
    "vtp_gemm_dgrad_swiglu": [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P],
    "vtp_gelu_bwd": [_P, _P, _P, _L, _P],
    "vtp_quick_gelu_bwd": [_P, _P, _P, _L, _P],
    "vtp_pixel_shuffle16": [_P, _P, _I, _I, _I, _P],
    "vtp_pixel_unshuffle16": [_P, _P, _I, _I, _I, _P],
    "vtp_l1_loss_fwd_bwd": [_P, _P, _P, _P, _I, _I, _I, _F, _P],
    "vtp_adamw": [_P, _P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _F, _P],
    "vtp_adamw_dev": [_P, _P, _P, _P, _P, _L, _P, _P],
    "vtp_adamw_dev_masked": [_P, _P, _P, _P, _P, _P, _L, _P, _P],
    "vtp_reduce_slabs": [_P, _L, _I, _P, _L, _I, _P],
    "vtp_gemm_splits": [_I, _I],
    "vtp_gemm_tn_splits": [_I, _I, _I],
    "vtp_gemm_qkv_rope": [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P],
    "vtp_gemm_tn": [_P, _I, _P, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P],
    "vtp_gemm_tn_grouped": [_P, _I, _I, _I, _I, _P, _P, _P],
    "vtp_gemm_tn_grouped_items": [_P, _I, _I, _I, _P, _I, _I, _P, _P, _P],
    "vtp_colsum_bf16": [_P, _I, _P, _I, _I, _I, _I, _I, _P],
    "vtp_colsum_bf16_rows": [_P, _I, _P, _P, _I, _I, _P],
    "vtp_gather_image_rows": [_P, _P, _P, _P, _I, _L, _I, _F, _P],
    "vtp_scatter_image_rows": [_P, _P, _P, _I, _L, _I, _F, _I, _P],
    "vtp_gather_tail_rows": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vtp_tail_row_map": [_P, _P, _I, _I, _I, _P],
    "vtp_expand_rows_bf16": [_P, _P, _P, _I, _I, _I, _P],
    "vtp_layerscale_wgrad": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "vtp_scaled_transpose": [_P, _P, _P, _I, _I, _P],
    "vtp_qk_norm_fwd": [_P, _P, _P, _P, _P, _L, _I, _F, _P],
    "vtp_qk_norm_bwd": [_P, _P, _P, _P, _P, _P, _P, _L, _I, _P],
    "vtp_set_gemm_tuning": [_I, _I],
    "vtp_gemm_nt_config": [_I, _I, _I, _I],
    "vtp_gemm_debug": [_P, _I, _I],
    "vtp_attn_debug": [_P, _I, _I, _I],
    "vtp_cu_thief": [_I, _I, _P, _P],
    "vtp_set_gemm_dynamic": [_I],
    "vtp_norm_fwd_e4m3": [_P, _P, _P, _P, _P, _P, _I, _I, _F, _I, _P],
    "vtp_quantize_e4m3": [_P, _I, _P, _L, _P, _F, _P],
    "vtp_amax": [_P, _I, _L, _P, _P],
    "vtp_dequantize_e4m3": [_P, _P, _L, _F, _P],
    "vtp_gemm_nt_fp8": [_P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _I, _P],
    "vtp_u8_to_images": [_P, _P, _L, _I, _I, _P, _P, _I, _P],
    "vtp_images_to_u8": [_P, _P, _L, _I, _I, _P, _P, _P],
    "vtp_latent_channel_stats": [_P, _P, _L, _I, _I, _P],
    "vtp_ema": [_P, _P, _L, _F, _P],
    "vtp_gather_token_rows": [_P, _P, _P, _I, _I, _P],
    "vtp_scatter_token_rows": [_P, _P, _P, _I, _I, _P],
    "vtp_weight_norm_prep": [_P, _P, _P, _P, _P, _I, _I, _P],
    "vtp_weight_norm_bwd": [_P, _P, _P, _P, _P, _P, _I, _I, _P],
    "vtp_softmax_center": [_P, _P, _F, _P, _I, _I, _P],
    "vtp_softmax_center_dev": [_P, _P, _P, _P, _I, _I, _P],
    "vtp_dino_ce": [_P, _P, _P, _P, _P, _F, _P, _P, _I, _I, _P],
    "vtp_center_ema": [_P, _P, _F, _P, _F, _I, _P],
    "vtp_conv3x3": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "vtp_lpips_unfold3": [_P, _P, _P, _I, _I, _I, _P, _P, _P],
    "vtp_lpips_fold3_bwd": [_P, _P, _I, _I, _I, _P, _P],
    "vtp_maxpool2_fwd": [_P, _P, _I, _I, _I, _I, _P],
    "vtp_maxpool2_bwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vtp_lpips_tap": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "vtp_ema_dev": [_P, _P, _L, _P, _P],
    "vtp_adamw_ema_dev": [_P, _P, _P, _P, _P, _P, _L, _P, _P],
    "vtp_adamw_dev_grouped": [_P, _P, _P, _P, _P, _P, _P, _I, _L, _P, _P],
    "vtp_adamw_ema_dev_grouped": [_P, _P, _P, _P, _P, _P, _P, _I, _L, _P, _P],
    "vtp_sumsq_partials_count": [_L],
    "vtp_sumsq_partials": [_P, _L, _P, _P],
    "vtp_sum_partials": [_P, _I, _P, _P],
    "vtp_grad_clip_finalize": [_P, _I, _P, _P, _P, _P],
    "vtp_grad_clip_finalize_guarded": [_P, _I, _P, _P, _P, _P, _P, _P],
    "vtp_adamw_dev_guarded": [_P, _P, _P, _P, _P, _P, _P, _I, _L, _P, _P, _P],
    "vtp_adamw_ema_dev_guarded": [_P, _P, _P, _P, _P, _P, _P, _I, _L, _P, _P, _P],
    "vtp_ema_dev_guarded": [_P, _P, _L, _P, _P, _P],
    "vtp_embed_tokens": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "vtp_embed_tokens_bwd": [_P, _P, _P, _P, _I, _I, _I, _P],
    "vtp_gather_rows": [_P, _P, _P, _I, _I, _I, _P],
    "vtp_scatter_rows": [_P, _P, _P, _P, _I, _I, _I, _P],
    "vtp_text_row_plan": [_P, _P, _P, _P, _I, _I, _P],  # ids eot cu rows B T stream
    "vtp_embed_tokens_packed": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "vtp_embed_tokens_bwd_packed": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "vtp_gather_rows_packed": [_P, _P, _P, _I, _I, _P],
    "vtp_scatter_rows_packed": [_P, _P, _P, _P, _I, _I, _I, _P],
    # device row limits (m_rows: device int in front of the stream)
    "vtp_gelu_bwd_limit": [_P, _P, _P, _I, _I, _I, _P, _P],
    "vtp_norm_fwd_limit": [_P, _P, _P, _P, _P, _I, _I, _F, _I, _P, _P],
    "vtp_norm_bwd_limit": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P],
    "vtp_gemm_nt_limit": [_P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P],
    "vtp_attn_fwd_varlen": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _L, _L, _F, _P],
    "vtp_attn_bwd_varlen": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _L, _L, _F, _P],
    "vtp_gemm_tn_grouped_limit": [_P, _I, _I, _I, _P, _P],
    "vtp_l2norm_fwd": [_P, _P, _P, _I, _I, _F, _P],
    "vtp_l2norm_bwd": [_P, _P, _P, _P, _I, _I, _P],
    "vtp_clip_logits": [_P, _P, _P, _P, _I, _I, _I, _P],
    "vtp_clip_grad_rows": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vtp_clip_grad_cols": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vtp_siglip_pairs": [_P, _P, _I, _I, _I, _F, _P, _P, _P, _P],
    "vtp_koleo": [_P, _P, _P, _P, _I, _I, _F, _F, _P],
    "vtp_sinkhorn_knopp": [_P, _F, _P, _P, _P, _P, _I, _I, _F, _P, _P, _I, _I, _P],
    "vtp_clip_loss": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P],
    "vtp_probe_logits": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P],  # X ldx W bias logits ldl B N K stream
    "vtp_probe_ce": [_P, _I, _P, _I, _I, _I, _F, _P, _P, _P, _P],  # logits ldl labels B H C inv_rows loss correct dlogits stream
    "vtp_probe_sgd": [_P, _P, _P, _P, _P, _I, _P, _I, _P, _I, _I, _I, _I, _F, _P],  # W bias mW mb dlogits ldl X ldx lr B H C K momentum stream
    # linear segmentation probe (segprobe.hip)
    "vtp_seg_ce_workspace_bytes": [_I, _I, _I, _I, _I, _I, _I],  # B h w Hl Wl H C -> bytes, or -1
    # Z ldz labels B h w Hl Wl H C ignore_index lse conf loss call_counts totals workspace workspace_bytes stream
    "vtp_seg_ce": [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P],
    # Z ldz labels lse call_counts G ldg B h w Hl Wl H C ignore_index stream
    "vtp_seg_dlogits": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "vtp_seg_sgd_slice": [],
    "vtp_seg_sgd_workspace_bytes": [_I, _I, _I],  # M N K -> bytes, or -1
    # W bias mW mb G ldg X ldx lr M H C K momentum workspace workspace_bytes stream
    "vtp_seg_sgd": [_P, _P, _P, _P, _P, _I, _P, _I, _P, _I, _I, _I, _I, _F, _P, _L, _P],
    # linear depth probe (depthprobe.hip)
    "vtp_depth_pix_workspace_bytes": [_I, _I, _I, _I, _I, _I, _I, _I],  # B h w Hl Wl H C aux_plane -> bytes, or -1
    # Z ldz gt B h w Hl Wl H C min_depth max_depth lam dhat aux loss stats eval_counts eval_sums workspace workspace_bytes stream
    "vtp_depth_pix": [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _P, _P, _P, _P, _P, _P, _P, _L, _P],
    # Z ldz aux stats G ldg B h w Hl Wl H C min_depth max_depth lam stream
    "vtp_depth_dlogits": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _P],
    "vtp_depth_sgd_workspace_bytes": [_I, _I, _I],  # M N K -> bytes, or -1
    # W bias mW mb G ldg X ldx lr M H C K momentum workspace workspace_bytes stream
    "vtp_depth_sgd": [_P, _P, _P, _P, _P, _I, _P, _I, _P, _I, _I, _I, _I, _F, _P, _L, _P],
    "vtp_zs_class_mean": [_P, _I, _P, _I, _I, _I, _I, _F, _P],  # feat ldf Wt ldw C T D eps stream
    # F ldf Wt ldw targets scale B C D counts per_class rank pred logits ldl stream
    "vtp_zs_topk": [_P, _I, _P, _I, _P, _F, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P],
    "vtp_recon_scratch_doubles": [_L, _I, _I],  # B H W -> doubles of scratch, or -1
    # images recon B H W sub3 div3 ref_u8 rec_u8 ref_lp rec_lp scratch scratch_len stream
    "vtp_recon_metrics": [_P, _P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _L, _P],
    "vtp_recon_finalize": [_P, _L, _L, _I, _I, _P, _P, _P, _P, _P, _P],  # scratch scratch_len B H W psnr ssim sse lpips acc stream
    "vtp_augment_scratch_floats": [_L, _I],  # N S -> floats of scratch, or -1
    # src_u8 B Hs Ws table N S mean3 std3 out scratch scratch_len stream
    "vtp_augment_crops": [_P, _L, _I, _I, _P, _L, _I, _P, _P, _P, _P, _L, _P],
    # src_u8 src_len scratch scratch_len jobs tab launches n_launches B Ho Wo mean3 std3 out out_u8 stream
    "vtp_preprocess": [_P, _L, _P, _L, _P, _P, _P, _I, _L, _I, _I, _P, _P, _P, _P, _P],
    # x w bias y B H W Cin Cout kh kw stride ph pw relu c0 Ctot stream
    "vtp_conv2d_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "vtp_conv2d_f32_blocked": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "vtp_pool3x3_f32": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],  # x y B H W C stride mode c0 Ctot stream
    "vtp_global_avgpool_f32": [_P, _P, _I, _I, _I, _P],  # x y B HW C stream
    "vtp_resize_bilinear_nhwc": [_P, _P, _I, _I, _I, _I, _I, _I, _F, _F, _P],  # x y B C H W Ho Wo scale shift stream
    "vtp_fid_accum": [_P, _I, _P, _P, _I, _I, _P],  # feats ldf sum outer n D stream
    # fp32 inference forward.  A lda W ldw W2 C ldc bias bias2 gamma resid ldr M N K epilogue stream
    "vtp_gemm_nt_f32": [_P, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vtp_attn_fwd_f32": [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _L, _F, _I, _P],
    "vtp_norm_fwd_f32": [_P, _P, _P, _P, _P, _I, _I, _F, _I, _P],
    "vtp_rope_qk_f32": [_P, _P, _P, _I, _I, _I, _I, _P],
    "vtp_im2col16_rows_f32": [_P, _P, _I, _I, _I, _I, _P],
    "vtp_pixel_shuffle16_f32": [_P, _P, _I, _I, _I, _P],
    "vtp_pool_patch_rows_f32": [_P, _P, _I, _I, _I, _F, _P],
    # LPIPS in fp32 (lpips_f32.hip)
    "vtp_lpips_scale_nhwc_f32": [_P, _P, _I, _I, _I, _I, _P, _P, _P],  # x y B H W Cout shift3 scale3 stream
    "vtp_maxpool2_f32": [_P, _P, _I, _I, _I, _I, _P],  # x y B H W C stream
    "vtp_lpips_head_f32": [_P, _P, _P, _I, _I, _I, _P],  # f w part n HW C stream
    "vtp_lpips_finalize_f32": [_P, _P, _I, _I, _I, _P],  # part val n H W stream
    # weighted k-NN evaluation (knn.hip)
    "vtp_knn_workspace_bytes": [_I, _I, _I],  # B K splits -> bytes, or -1
    # Q ldq X ldx index_base B N D K sims idx workspace workspace_bytes splits sims_out lds stream
    "vtp_knn_topk": [_P, _I, _P, _I, _L, _I, _I, _I, _I, _P, _P, _P, _L, _I, _P, _I, _P],
    # sims idx labels n_total targets ks nk inv_T num_classes B K counts rank_out pred_out stream
    "vtp_knn_vote": [_P, _P, _P, _L, _P, _P, _I, _F, _I, _I, _I, _P, _P, _P, _P],
    # k-NN manifold precision / recall (precision_recall.hip)
    "vtp_pr_workspace_bytes": [_I, _I],  # B splits -> bytes, or -1
    "vtp_pr_sqnorm": [_P, _I, _I, _I, _P, _P],  # X ldx N D out stream
    # Q ldq qn X ldx xn query_base index_base B N D dist workspace workspace_bytes splits d2_out ldo stream
    "vtp_pr_knn_dist": [_P, _I, _P, _P, _I, _P, _L, _L, _I, _I, _I, _P, _P, _L, _I, _P, _I, _P],
    "vtp_pr_cover": [_P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P, _I, _P],  # Q ldq qn X ldx xn r2 B N D hits splits stream
    # image-text retrieval (retrieval.hip)
    "vtp_retr_best": [_P, _I, _P, _I, _L, _P, _P, _I, _I, _I, _P, _P, _P],  # Q ldq X ldx n_total gt_ptr gt_idx nnz B D best_s best_j stream
    # Q ldq X ldx index_base B N D best_s best_j beats splits sims_out lds stream
    "vtp_retr_rank": [_P, _I, _P, _I, _L, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P],
    "vtp_retr_count": [_P, _I, _P, _I, _P, _P, _L, _P],  # beats B ks nk counts rank rank_offset stream
    # Inception Score (inception_score.hip)
    "vtp_is_rows": [_P, _I, _I, _I, _P, _I, _P, _P],  # logits ldl B C p ldp h stream
    "vtp_is_accum": [_P, _I, _P, _L, _L, _I, _I, _P, _I, _P],  # p ldp h row_base split_size B C state n_slots stream
    # Kernel Inception Distance (mmd.hip)
    "vtp_mmd_workspace_bytes": [_I, _I, _I],  # B N P -> bytes, or -1
    # Q ldq q_rows qi X ldx x_rows xi query_base index_base B N D P kparams degree part part_bytes stream
    "vtp_mmd_poly_part": [_P, _I, _I, _P, _P, _I, _I, _P, _L, _L, _I, _I, _I, _I, _P, _I, _P, _L, _P],
    "vtp_mmd_fold": [_P, _P, _I, _I, _I, _P],  # part rowsum B tiles P stream
    "vtp_mmd_total": [_P, _I, _I, _P, _P],  # rowsum B P total stream
}

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"vtp_amd: {LIB_PATH} not found. The HIP library is mandatory (there is no fallback path): "
            "run `python -c 'import __graft_entry__ as g; g.build()'` or `python vtp_amd/build.py`.")
    # On a GPU box the HIP runtime must be up BEFORE the library's fat binaries register themselves (dlopen): loading it first
    # (e.g. __graft_entry__.build() followed by smoke() in one process) left every later launch of ours failing with "no
    # ROCm-capable device is detected" although torch's own kernels ran (ROCm 7.2, measured round 4).  No GPU: nothing to do.
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:  # the ABI / symbol check of tests/test_abi.py does not need torch
        pass
    lib = ctypes.CDLL(LIB_PATH)
    lib.vtp_abi_version.restype = c_int
    lib.vtp_last_error.restype = c_char_p
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale -> loud
        fn.argtypes = args
        fn.restype = c_int
    if lib.vtp_abi_version() != 1:
        raise RuntimeError("vtp_amd: ABI version mismatch between vtp_amd/_lib.py and libvtp_hip.so")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = _lib.vtp_last_error().decode(errors="replace") if _lib is not None else ""
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")
