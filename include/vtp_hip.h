/* vtp_hip.h -- C ABI of libvtp_hip.so: the MI355X (gfx950 / CDNA4) kernels of the VTP training hot path.
 *
 * The reference (MiniMax-AI/VTP) is pure PyTorch: it has no FFI / plugin registry, every device
 * "kernel" is an ATen call issued from an nn.Module.forward.  Each entry point below
 * therefore names the reference ATen call site(s) (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless stated; bf16 = raw uint16
 *     storage (IEEE bfloat16, round-to-nearest-even); "f32" = float.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Kernels are enqueued
 *     asynchronously; nothing synchronises the device.
 *   - return 0 on success, VTP_ERR_ARG (-1) on a rejected argument (message via vtp_last_error()),
 *     or a positive hipError_t if the launch failed.  The library never aborts the process.
 *   - no hidden global state apart from the last-error string (thread-local) and kernel attributes;
 *     callers own every buffer (ownership never transfers).
 *   - token matrices are row-major [rows, features] with an explicit leading dimension where given.
 */
#ifndef VTP_HIP_H
#define VTP_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define VTP_ABI_VERSION 1

int vtp_abi_version(void);
const char* vtp_last_error(void);

/* ---- GEMM ------------------------------------------------------------------------------------
 * C[M,N] = epilogue(alpha * A[M,K] * B[N,K]^T).  A, B bf16 K-contiguous.  Replaces every nn.Linear /
 * 1x1-conv / patch-embed conv `addmm`: attention.py:92,94 (qkv, proj), ffn.py:78-81 (w1,w2,w3),
 * vision_transformer_bottleneck.py:68-74, pixel_decoder.py:138,157, embeddings.py:64 (after im2col),
 * block.py:412-414 + nn.MultiheadAttention in/out proj (text tower), modeling_vtp.py:274,306, and (with
 * transposed operands) their autograd dgrad/wgrad.
 *   a_grp/a_pre, c_grp/c_pre: optional row remap row(m) = m + (m / grp + 1) * pre (grp = 0: none) used to
 *   read/write only the patch rows of a [B, 1+hw, D] token stream.  c_grp = -1 selects the SwiGLU de-interleave
 *   row(m) = ((m>>4)<<3) + (m&7) + ((m&8) ? c_pre : 0) (wgrad of the interleaved [w1|w2] matrix, c_pre = H).
 * Epilogues:
 *   VTP_EPI_BF16        C bf16 = acc + bias
 *   VTP_EPI_F32         C f32  = resid + gamma * (acc + bias)            (bias/gamma/resid optional; block.py:293-294)
 *   VTP_EPI_SWIGLU      B rows interleaved [8 x w1 | 8 x w2] per 16; C bf16 [M, N/2] = silu(x1) * x2, C2 bf16 [M,N] = (x1|x2)
 *   VTP_EPI_GELU        C bf16 = gelu_erf(acc + bias), C2 bf16 = acc + bias (optional)
 *   VTP_EPI_QUICK_GELU  the same with QuickGELU x * sigmoid(1.702 x) (text_quick_gelu; layers/activation.py:5-12)
 *   VTP_EPI_F32_ATOMIC  C f32 += alpha * acc, split-K over `splits` slices with fp32 atomics
 *   VTP_EPI_F32_SLAB    split-K slice z writes alpha * acc to C + z * (4*ldc2) floats with plain stores (wgrad; sum the
 *                       slabs with vtp_reduce_slabs).  The slice count actually used is vtp_gemm_splits(K, splits).
 */
enum { VTP_EPI_BF16 = 0, VTP_EPI_F32 = 1, VTP_EPI_SWIGLU = 2, VTP_EPI_GELU = 3, VTP_EPI_F32_ATOMIC = 4, VTP_EPI_F32_SLAB = 5,
       VTP_EPI_QUICK_GELU = 8 };
int vtp_gemm_splits(int K, int splits);
/* split-K factor the weight-gradient GEMM C[M,N] = A[K,M]^T B[K,N] should be launched with (tile configuration aware:
 * 256x256 8-phase kernel -> tiles x splits = one round of the CUs; ring kernel -> just under 512 workgroups) */
int vtp_gemm_tn_splits(int M, int N, int K);
/* C[M,N] f32 = A[K,M]^T * B[K,N]: A, B bf16 row-major with the reduction dimension (tokens) as ROWS -- the weight-gradient
 * GEMM dW = dY^T X of every linear, read straight from the activation layouts (fragments are formed with the gfx950 LDS
 * transpose read; no transposed copies).  epilogue VTP_EPI_F32 (C = resid + acc, pass resid = C to accumulate),
 * a_colsum (optional, f32 [M], ACCUMULATED, rows mapped like C's): column sums of A over the tokens = the bias gradient of the
 * same linear layer (nn.Linear backward: db = dY.sum(0)); fused into the GEMM where the tile configuration allows, else a
 * column-sum pass on the same stream.
 * VTP_EPI_F32_SLAB (split-K slabs, see above) or VTP_EPI_F32_ATOMIC (split-K slices add into C with fp32 atomics: no slab
 * round trip through HBM; the summation order, hence the last bits, vary from run to run).  a_/b_ remaps act on the token rows of A / B, c_ on the rows of C. */
int vtp_gemm_tn(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int ldc2, const float* resid, int M, int N,
                int K, int epilogue, int a_grp, int a_pre, int b_grp, int b_pre, int c_grp, int c_pre, int splits,
                float* a_colsum, void* stream);
/* The weight gradients of one transformer block as ONE launch: up to 8 problems C_g[M_g, N_g] (+)= A_g[K, M_g]^T B_g[K, N_g] that
 * reduce over the same K token rows (nn.Linear backward dW = dY^T X of attn.qkv / attn.proj / mlp.w1|w2 / mlp.w3, block.py:290-296),
 * (sum of 256 x 256 tiles) x splits workgroups; the K slices of a tile are combined inside the launch by the last-arriving
 * workgroup, which applies the epilogue (accumulate or overwrite, SwiGLU row de-interleave c_grp = -1, bias-gradient column sums).
 * probs: device array of nprob records of 16 int64 {A, B, C, colsum | lda, ldb, ldc | M, N | c_grp, c_pre | tile0 | accumulate | K 0 0}
 * (K: the problem's own token count in an item-list launch, 0 = the launch's K; the uniform-grid launch takes one K for all);
 * part: ntiles * splits_eff * 65536 floats, ticket: ntiles ints, zero before the first launch (the kernel leaves them zero). */
int vtp_gemm_tn_grouped(const void* probs, int nprob, int ntiles, int K, int splits, void* part, void* ticket, void* stream);
/* the same launch over the token rows [0, min(K, *k_rows)) (k_rows: device int): always ONE K slice per tile (no ticket is ever waited on,
 * no scratch), and no operand row >= *k_rows is read */
int vtp_gemm_tn_grouped_limit(const void* probs, int nprob, int ntiles, int K, const int* k_rows, void* stream);
/* the same launch on the one-wave-per-SIMD kernel with the hand-scheduled k loop (K % 8 == 0; bit-identical results per K slice), from an
 * explicit work-item list, so that the tiles need not be cut alike: items = device array of nitems records of 8 int32 {tile, kbeg, kcount,
 * nparts, part, 0, 0, 0}, one workgroup each; the items of a tile partition [0, K) (kbeg multiples of 64); slots = the largest nparts;
 * part: ntiles * slots * 65536 floats.  The tiles that also form a bias gradient (column sums of dY beside the MFMAs: 27 % more time per
 * k-tile) get one slice more than the rest -- same reference call sites as above. */
int vtp_gemm_tn_grouped_items(const void* probs, int nprob, int ntiles, int K, const void* items, int nitems, int slots, void* part,
                              void* ticket, void* stream);
/* tuning knob (benchmarks / experiments / tests): force a kernel configuration id and toggle the XCD-aware workgroup remap.
 * force_cfg: -1 = heuristic | ring kernel tiles 0 = 128x128 4 waves, 3 = 256x128 3 stages, 4 = 256x256, 5 = 128x128 8 waves,
 * 7 = 128x64, 21 = 5 software-pipelined | 8 = 256x256 8-phase kernel | 9 = 128x256 half-size kernel | 10 = one-wave-per-SIMD kernel
 * (8 / 9 / 10 fall back to 5 where their limits do not hold; vtp_gemm_tn knows 8 and runs 5 for every other id).  Any other id is
 * refused and leaves the state as it was.  Process-global; not part of the reference-facing surface. */
int vtp_set_gemm_tuning(int force_cfg, int xcd_swizzle);
/* persistent 256 x 256 NT launches draw their tiles from per-XCD queues in device memory (1) instead of owning a static tile list (0,
 * default): a launch that cannot get every CU at once -- RCCL channels hold some for the whole backward -- then ends when the tiles
 * are done, not when the last late-starting workgroup's list is.  Process-global; VTP_GEMM_DYN=0 / 1 in the environment overrides.
 * VTP_GEMM_CUS=n caps the workgroup slots of every one-workgroup-per-CU GEMM launch (INTEGRATION.md "Running beside RCCL"). */
int vtp_set_gemm_dynamic(int on);
/* diagnostics (tools/gemm8p_timeline.py): `timing` = device buffer of [workgroups][16 tiles][4] 64-bit s_memrealtime stamps
 * {tile start, k loop done, epilogue issued} written by the 256x256 kernel (null = off); grid_limit caps its persistent grid
 * (0 = every CU); delay_ticks > 0 starts every second workgroup of an XCD that many 10-ns ticks late (lock-step experiments).
 * Process-global; not part of the reference-facing surface. */
int vtp_gemm_debug(void* timing, int grid_limit, int delay_ticks);
/* diagnostics (tools/attn_timing.py, tools/attn_bwd_timeline.py; VTP_DIAG=1 for anything but all off): `timing` = device buffer of
 * [workgroups][16 waves][8] 64-bit s_memrealtime stamps, null = off: slots 0..6 of the resident attention forward, slots 0..3 {start,
 * operands staged, loop done, gradients stored} of the backward kernels (per-head backward: 2 x the buffer, dQ kernel, then the
 * dK/dV kernel).  Process-global; not part of the reference-facing surface. */
/* diagnostics (tools/cu_thief.py; VTP_DIAG=1): nwg workgroups that hold one CU each (160 KiB LDS) for ticks x 10 ns on `stream` -- the
 * footprint of a communication kernel beside the step; out: null or nwg u64 (ticks held) */
int vtp_cu_thief(int nwg, int ticks, void* out, void* stream);
int vtp_attn_debug(void* timing, int lds_pad, int waves_per_wg, int stagger_ticks);  /* lds_pad: extra dynamic LDS bytes per workgroup; waves_per_wg: 0 = heuristic */
/* host-only: the kernel configuration vtp_gemm_nt picks for a shape (8 = 256x256 8-phase, 7 = 128x64 ring tiles, other ids = ring
 * configurations; bits 8.. = in-launch split-K slices when > 1); -1 for a bad shape.  No launch, no device needed. */
int vtp_gemm_nt_config(int M, int N, int K, int epilogue);
int vtp_gemm_nt(const void* A, int lda, const void* B, int ldb, void* C, int ldc, void* C2, int ldc2,
                const float* bias, const float* gamma, const float* resid, int M, int N, int K, int epilogue,
                int a_grp, int a_pre, int c_grp, int c_pre, int splits, float alpha, void* stream);

/* qkv projection with apply_rope fused into the epilogue: replaces attention.py:115 (qkv Linear) + attention.py:70-89
 * (cast to the rope dtype, rotate the patch rows of q and k, cast back; bit-identical to vtp_gemm_nt + vtp_rope_qk).
 * C bf16 [M, N = 3*D] = A[M,K] W[N,K]^T + bias; columns < rope_cols (= 2*D) of row m are rotated with row rope_pos[m] of the
 * bf16 tables sin / cos [*, 64] (rope_pos[m] < 0: prefix (cls) rows, untouched).  rope_pos lets several images / resolutions
 * share one launch (the list forward, vision_transformer.py:221-258): it indexes a concatenation of the per-resolution tables. */
int vtp_gemm_qkv_rope(const void* A, int lda, const void* W, int ldb, const float* bias, void* C, int ldc, int M, int N, int K,
                      const int* rope_pos, const void* rope_sin, const void* rope_cos, int rope_cols, void* stream);

/* ---- residual-wiring extras of SelfAttentionBlock (block.py:20-118,207-289; misc.py:7-26) ---------------------------------
 * Stochastic depth ("sample drop"): the residual branch runs on a random subset of the images of a segment (an image = N
 * consecutive token rows) and is added back with alpha = batch / kept (torch.index_add(x, 0, residual, idx, alpha), block.py:216-232).
 *   vtp_gather_image_rows : dst[i*N + t, :] = src[idx[i]*N + t, :] as f32 (dst, optional) and/or as bf16(scale * .) (dst_bf16, optional)
 *   vtp_scatter_image_rows: dst[idx[i]*N + t, :] = (accumulate ? dst : 0) + alpha * src[i*N + t, :]      (idx entries are distinct)
 * LayerScale (y = x + gamma * f(x), misc.py:24-25) backward without storing f: with G = dy^T x_in (the unscaled weight-gradient
 * GEMM) and cs = colsum(dy):  dW += gamma (.) G,  db += gamma (.) cs,  dgamma += rowsum(W (.) G) + b (.) cs;
 * vtp_scaled_transpose writes bf16 (gamma (.) W)^T, the dgrad operand. */
int vtp_gather_image_rows(const float* src, const int* img_idx, float* dst, void* dst_bf16, int n_img, long N, int D, float scale,
                          void* stream);
int vtp_scatter_image_rows(const float* src, const int* img_idx, float* dst, int n_img, long N, int D, float alpha, int accumulate,
                           void* stream);
/* Tail rows of the last block: everything behind its attention is row-wise and runs on the Mc = L + T rows a consumer reads.  Compact
 * row j < L is full row j; compact row L + t is full row L + idx[t] (idx int32 [T], -1 = padding: an all-zero compact row).
 *   vtp_gather_tail_rows : o_c bf16 / x_c f32 [L + T, D] = those rows of o / x [M, D], one launch (either pair may be null)
 *   vtp_tail_row_map     : map int32 [M] = full row -> compact row, -1 where no compact row reads it (reads no host-side count)
 *   vtp_expand_rows_bf16 : dst[r, :] = map[r] >= 0 ? src[map[r], :] : 0 for all M rows of dst in one pass (src bf16 [Mc, D]) */
int vtp_gather_tail_rows(const void* o, const float* x, const int* idx, void* o_c, float* x_c, int T, int L, int M, int D,
                         void* stream);
int vtp_tail_row_map(const int* idx, int* map, int T, int L, int M, void* stream);
int vtp_expand_rows_bf16(const void* src, const int* map, void* dst, int M, int Mc, int D, void* stream);
int vtp_layerscale_wgrad(const float* G, const float* W, const float* bias, const float* colsum, const float* gamma, float* dW,
                         float* db, float* dgamma, int N, int K, void* stream);
int vtp_scaled_transpose(const float* W, const float* gamma, void* dstT, int N, int K, void* stream);
/* QK normalisation (attention.py:67-68,119-120): q = RMSNorm(64)(q), k likewise (weights wq / wk [64], shared by the heads), before
 * RoPE.  qkv bf16 [M, 3D] -> out (v copied), inv f32 [M, 2 D / 64] = rsqrt(mean x^2 + eps) per (row, part, head);
 * backward in place on the q / k parts of dqkv, dwq / dwk accumulated. */
int vtp_qk_norm_fwd(const void* qkv, const float* wq, const float* wk, void* out, float* inv, long M, int D, float eps, void* stream);
int vtp_qk_norm_bwd(void* dqkv, const void* qkv, const float* inv, const float* wq, const float* wk, float* dwq, float* dwk, long M, int D,
                    void* stream);

/* ---- normalisation ---------------------------------------------------------------------------
 * kind 0 = RMSNorm (normalization.py:17-22, eps 1e-5, no bias), 1 = LayerNorm (vision_transformer.py:30-34
 * eps 1e-6 decoder; normalization.py:25-31 text).  x f32 [M, D] -> y bf16 [M, D]; stats f32 [M,2] = (mean, rstd).
 * bwd: dx f32 [M,D] = (dres ? dres : 0) + norm_bwd(dy bf16), optionally also written as bf16 (dx_bf16, the A operand
 * of the next dgrad GEMM); dw/db f32 [D] are ACCUMULATED (+=) atomically.  dx_colsum (optional, f32 [D], accumulated):
 * column sums of dx_bf16 = the bias gradient of the linear layer that receives dx_bf16 as its dy (no separate pass). */
int vtp_norm_fwd(const float* x, const float* w, const float* b, void* y, float* stats, int M, int D, float eps,
                 int kind, void* stream);
int vtp_norm_bwd(const void* dy, const float* x, const float* w, const float* stats, const float* dres, float* dx,
                 void* dx_bf16, float* dw, float* db, float* dx_colsum, int M, int D, int kind, void* stream);
/* vtp_norm_bwd where the patch rows of one list item -- rows prow0 + b*pN + t, b < pB, 1 <= t < pN -- take pvec[b] (f32 [pB, D]) on
 * top of dy, summed in f32 inside the kernel: the gradient of a feature mean-pooled over those rows (vision_clip_feat = 'pooled',
 * modeling_vtp.py:261-276) rides in the trunk's final-norm backward instead of a pass over dy.  D <= 1024. */
int vtp_norm_bwd_pvec(const void* dy, const float* x, const float* w, const float* stats, const float* dres, float* dx,
                      void* dx_bf16, float* dw, float* db, float* dx_colsum, const float* pvec, int prow0, int pB, int pN, int M,
                      int D, int kind, void* stream);
/* vtp_norm_bwd whose residual gradient lives in a compact buffer dres f32 [dres_M, D]: row r adds dres[dres_rows[r]], or nothing when
 * the entry is -1 (dres_rows int32 [M]; null: exactly vtp_norm_bwd).  With a row map: D <= 1024. */
int vtp_norm_bwd_rows(const void* dy, const float* x, const float* w, const float* stats, const float* dres, const int* dres_rows,
                      int dres_M, float* dx, void* dx_bf16, float* dw, float* db, float* dx_colsum, int M, int D, int kind,
                      void* stream);
/* out f32 [B, D] = scale * sum_{t=1}^{N-1} x[b*N + t] over the bf16 token rows x [B*N, D] of one list item (row 0 of every image is
 * its cls token and is skipped); scale = 1 / (N - 1) is the mean of the patch tokens.  N >= 2, D % 4 == 0. */
int vtp_pool_patch_rows(const void* x, float* out, int B, int N, int D, float scale, void* stream);

/* ---- RoPE (attention.py:12-23,70-89) ----------------------------------------------------------
 * In place on the q and k thirds of a packed qkv bf16 [B*N, 3*D] buffer (head h at column h*64 of each third).
 * Rows n < prefix (cls) are untouched; sin/cos are the reference's bf16 tables [N-prefix, 64].  Rounding follows
 * eager bf16: bf16(bf16(x*cos) + bf16(rot(x)*sin)).  inverse != 0 applies the transpose (backward). */
int vtp_rope_qk(void* qkv, const void* sin, const void* cos, int B, int N, int heads, int prefix, int inverse,
                void* stream);

/* ---- attention (attention.py:124 F.scaled_dot_product_attention; text: nn.MultiheadAttention causal) ----
 * q/k/v/o are bf16 with element strides: batch stride `sb`, token stride `sn`, head h at +h*64 (head_dim is 64).
 * lse f32 [B, heads, N] (natural-log-sum-exp of scale*q.k).  causal != 0 masks key > query.
 * bwd: delta f32 [B, heads, N] is scratch (rowsum(dO*O)).  rope_sin / rope_cos (bf16 [N - rope_prefix, 64], both or neither):
 * dq and dk are returned as gradients w.r.t. the UN-rotated q, k (the inverse of vtp_rope_qk applied with the same eager-bf16
 * rounding) -- fused into the kernels' stores for short sequences, a follow-up pass otherwise (needs the packed qkv layout). */
int vtp_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int N, int heads,
                 long sb_qkv, long sn_qkv, long sb_o, long sn_o, float scale, int causal, void* stream);
int vtp_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                 float* delta, void* dq, void* dk, void* dv, const void* rope_sin, const void* rope_cos, int rope_prefix,
                 int B, int N, int heads, long sb_qkv, long sn_qkv, long sb_o, long sn_o, float scale, int causal,
                 void* stream);

/* ---- data movement / elementwise --------------------------------------------------------------- */
/* im2col for the 16x16/s16 patch-embed conv (embeddings.py:58,64-69): img f32 [B,3,H,W] -> patches bf16 [B*h*w, 768],
 * K order (c, ky, kx), token order (y, x). */
int vtp_im2col16(const float* img, void* patches, int B, int H, int W, void* stream);
/* the same into a row layout with `prefix` rows in front of every image's patches (prefix = 1: the trunk's token rows, row 0 = cls, cf.
 * prepare_tokens_with_masks, vision_transformer.py:189-219): patch p of image b -> row b*(h*w+prefix) + prefix + p of rows bf16
 * [B*(h*w+prefix), 768]; the prefix rows are not written */
int vtp_im2col16_rows(const float* img, void* rows, int B, int H, int W, int prefix, void* stream);
/* gradient w.r.t. the input image of PatchEmbed (embeddings.py:61-70 backward; the reference's autograd returns it when the image
 * requires grad): d_patches f32 [B*hw, 768] (= d_tokens[patch rows] W_pe, K order (c, ky, kx)) folded back to d_img f32 [B,3,H,W] */
int vtp_col2im16(const float* dpatches, float* dimg, int B, int H, int W, void* stream);

/* rows [B, N, D] f32: write row 0 of every batch element = cls[D] (vision_transformer.py:198,210-217);
 * optionally substitute mask_token on masked patch rows (vision_transformer.py:195). masks: uint8 [B, N-1] or NULL. */
int vtp_assemble_tokens(float* x, const float* cls, const float* mask_token, const unsigned char* masks, int B, int N,
                        int D, void* stream);

/* out[c, r] = in[r, c] for a bf16 [R, C] matrix (ld_in) -> [C, ld_out]; columns r in [R, ld_out) are zero-filled.
 * If colsum != NULL, colsum[c'] += sum_r in[r,c] (bias gradients); c' = c, or, when colsum_swiglu_h = H > 0, the
 * de-interleaved SwiGLU index ((c>>4)<<3) + (c&7) + ((c&8) ? H : 0)  (b1 then b2, each [H]).
 * in_grp/in_pre: input row remap row(r) = r + (r / in_grp + 1) * in_pre (in_grp = 0: none), as in vtp_gemm_nt. */
int vtp_transpose_bf16(const void* in, int ld_in, void* out, int ld_out, float* colsum, int colsum_swiglu_h, int in_grp,
                       int in_pre, int R, int C, void* stream);
/* out[c'] += sum_r in[r, c] for a bf16 [R, C] matrix (bias gradient); same column / row remaps as vtp_transpose_bf16. */
int vtp_colsum_bf16(const void* in, int ld, float* out, int colsum_swiglu_h, int in_grp, int in_pre, int R, int C, void* stream);
/* the same with the row count in DEVICE memory (rows >= n_rows_dev[0] are skipped; R_max sizes the launch): the masked-token
 * count of an iBOT batch changes every step while the padded token buffers (vtp.py:432-439 `upperbound`) and a captured
 * hipGraph do not */
int vtp_colsum_bf16_rows(const void* in, int ld, float* out, const int* n_rows_dev, int R_max, int C, void* stream);
/* backward of vtp_assemble_tokens' mask substitution: for masked patch rows d_mask_token += dx[row] and dx_bf16[row] = 0
 * (so the patch-embed wgrad / bias-grad skip them).  dx f32 / dx_bf16 [B*N, D], masks uint8 [B, N-1]. */
int vtp_mask_rows_bwd(const float* dx, void* dx_bf16, const unsigned char* masks, float* d_mask_token, int B, int N, int D,
                      void* stream);
/* out[d] += sum_b in[b*stride + d], f32 (gradient of the broadcast cls token, vision_transformer.py:210-217). */
/* backward of vtp_assemble_tokens as a whole (vision_transformer.py:189-219 backward): the mask substitution as above (masks and
 * d_mask_token may both be null: an item without masks) AND the cls row: d_cls_token += dx[row 0 of every image], dx_bf16[row 0] = 0 --
 * afterwards dx_bf16 is the gradient of the patch-embed output in the token-row layout (zero in every row that is not a visible patch) */
int vtp_token_rows_bwd(const float* dx, void* dx_bf16, const unsigned char* masks, float* d_mask_token, float* d_cls_token, int B, int N,
                       int D, void* stream);
int vtp_strided_rowsum(const float* in, long stride, float* out, int B, int D, void* stream);

/* f32 -> bf16 cast (n elements); f32 [R,C] -> bf16 transposed [C,R] (weight caches W, W^T). */
int vtp_cast_f32_bf16(const float* in, void* out, long n, void* stream);
int vtp_cast_transpose_f32_bf16(const float* in, void* out, int R, int C, void* stream);
/* Batched refresh of the bf16 compute copies of all fp32 master weights in ONE launch.  `descs` is a device array of
 * n records of 8 x int64: {src f32*, src2 f32*, dst, dstT, R, C, mode, tile_start}; mode 0: dst bf16 [R,C] = src,
 * dstT bf16 [C,R] = src^T (either may be NULL); mode 1: the logical matrix is the SwiGLU interleave of src=w1 and
 * src2=w2 (16-row groups = [8 rows w1 | 8 rows w2], R = 2H); mode 2: dst f32 [R] = interleave of two bias vectors.
 * tile_start = exclusive prefix sum of per-record tile counts (64x64 tiles; mode 2: 256 elements per tile). */
int vtp_prep_weights(const void* descs, int n, int total_tiles, void* stream);
/* the same over a RUN of the table (the layers of one gradient bucket, refreshed right behind that bucket's optimizer update while the
 * backward of the other layers is still running): descs = the run's first record, n records, tile_base = that record's tile_start,
 * n_tiles = tiles of the run. */
int vtp_prep_weights_range(const void* descs, int n, int tile_base, int n_tiles, void* stream);

/* SwiGLU backward (ffn.py:80): given dh bf16 [M,H] and saved x12 bf16 [M,2H] (interleaved 8|8), writes dx12 bf16 [M,2H].
 * db12 (optional, f32 [2H] = [b1 | b2], accumulated): column sums of dx12 = the bias gradients of w1 / w2. */
int vtp_swiglu_bwd(const void* dh, const void* x12, void* dx12, float* db12, int M, int H, void* stream);
/* the same backward fused into the w3 dgrad GEMM: dx12[M, 2H] from dy[M, K] W3^T[H, K]^T and the saved x12 -- dh never reaches HBM */
int vtp_gemm_dgrad_swiglu(const void* A, int lda, const void* WT, int ldb, const void* x12, int ldx, void* dx12, int ldc, int M, int H,
                          int K, void* stream);
/* GELU backward (text MLP, block.py:399): dx = dy * gelu'(pre). */
int vtp_gelu_bwd(const void* dy, const void* pre, void* dx, long n, void* stream);
/* dx = dy * QuickGELU'(pre)  (x sigmoid(1.702 x), layers/activation.py:5-12); bf16, n % 8 == 0 */
int vtp_quick_gelu_bwd(const void* dy, const void* pre, void* dx, long n, void* stream);
/* Device row limits: m_rows points to a DEVICE int, and the kernels below work on the rows [0, min(M, *m_rows)) of their [M, .] operands
 * -- rows beyond are neither read nor written, and add nothing to the sums -- while the launch geometry stays that of the static M (one
 * captured graph serves every count).  GELU / QuickGELU backward over [M, H] (quick != 0: QuickGELU); the norms as vtp_norm_fwd /
 * vtp_norm_bwd; vtp_gemm_nt_limit as vtp_gemm_nt with one K slice and no row remaps, on the ring kernel only (the persistent 256-wide
 * kernels take no limit: their shapes run the ring configuration of the dispatch table; a forced configuration >= 8 is refused). */
int vtp_gelu_bwd_limit(const void* dy, const void* pre, void* dx, int M, int H, int quick, const int* m_rows, void* stream);
int vtp_norm_fwd_limit(const float* x, const float* w, const float* b, void* y, float* stats, int M, int D, float eps, int kind,
                       const int* m_rows, void* stream);
int vtp_norm_bwd_limit(const void* dy, const float* x, const float* w, const float* stats, const float* dres, float* dx, void* dx_bf16,
                       float* dw, float* db, float* dx_colsum, int M, int D, int kind, const int* m_rows, void* stream);
int vtp_gemm_nt_limit(const void* A, int lda, const void* B, int ldb, void* C, int ldc, void* C2, int ldc2, const float* bias,
                      const float* gamma, const float* resid, int M, int N, int K, int epilogue, float alpha, const int* m_rows,
                      void* stream);
/* The causal tiled attention kernels over packed captions: batch b = rows [cu[b], cu[b + 1]) (at most Nmax) of the packed qkv / o buffers
 * (token strides sn_qkv / sn_o); grid and the [B, heads, Nmax] lse / delta layout are the padded launch's. */
int vtp_attn_fwd_varlen(const void* q, const void* k, const void* v, void* o, float* lse, const int* cu, int B, int Nmax, int heads,
                        long sn_qkv, long sn_o, float scale, void* stream);
int vtp_attn_bwd_varlen(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse, float* delta,
                        void* dq, void* dk, void* dv, const int* cu, int B, int Nmax, int heads, long sn_qkv, long sn_o, float scale,
                        void* stream);

/* PixelShuffle(16) (pixel_decoder.py:160): t bf16 [B*h*w, 768] token-major -> img f32 [B,3,16h,16w]. */
int vtp_pixel_shuffle16(const void* t, float* img, int B, int h, int w, void* stream);
/* backward of F.pixel_shuffle(., 16) (pixel_decoder.py:160): image gradient f32 [B,3,16h,16w] -> token-major bf16 [B*h*w, 768] */
int vtp_pixel_unshuffle16(const float* d_img, void* dt, int B, int h, int w, void* stream);
/* L1 reconstruction loss on the token-major decoder output: loss_sum[0] += sum |shuffle(t) - target|;
 * dt bf16 [B*h*w,768] = sign(shuffle(t) - target) * gscale  (gscale = loss_weight / numel). */
int vtp_l1_loss_fwd_bwd(const void* t, const float* target, void* dt, float* loss_sum, int B, int h, int w,
                        float gscale, void* stream);

/* fused AdamW over one flat f32 parameter buffer (torch.optim.AdamW semantics); also refreshes the bf16 copy. */
int vtp_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, long n, float lr, float beta1, float beta2,
              float eps, float weight_decay, int step, float grad_scale, void* stream);
/* same, hyper-parameters read from DEVICE memory: hyper[8] = {lr, beta1, beta2, eps, weight_decay, 1-beta1^t,
 * sqrt(1-beta2^t), grad_scale} -- lets a captured hipGraph of the training step replay with per-step values. */
int vtp_adamw_dev(float* p, const float* g, float* m, float* v, void* p_bf16, long n, const float* hyper, void* stream);
/* the same with a weight-decay exemption table: nodecay4[i] != 0 exempts elements [4i, 4i + 4) (one flag per float4 -- parameters are
 * padded to 4 elements in the flat buffer): biases / norm gains / tokens / logit scale follow the usual AdamW recipe */
int vtp_adamw_dev_masked(float* p, const float* g, float* m, float* v, void* p_bf16, const void* nodecay4, long n, const float* hyper,
                         void* stream);
/* dst[i] (+)= sum_{s<S} slabs[s*stride + i], f32 (split-K partials -> gradient buffer). */
int vtp_reduce_slabs(const float* slabs, long stride, int S, float* dst, long n, int accumulate, void* stream);
/* EMA teacher update t = m*t + (1-m)*s over a flat buffer (vtp.py:388-401). */
int vtp_ema(float* t, const float* s, long n, float momentum, void* stream);
int vtp_ema_dev(float* t, const float* s, long n, const float* momentum /* device scalar */, void* stream);
/* AdamW (vtp_adamw_dev_masked; nodecay4 may be NULL) with the EMA update of the teacher's copy of the same elements fused in
 * (teacher = mom * teacher + (1 - mom) * p_new, vtp.py:388-401; teacher may be NULL; mom = hyper[9]): ONE pass over a gradient
 * bucket for the per-bucket optimizer lane of the training step.  Short-lived blocks (4096 elements each). */
int vtp_adamw_ema_dev(float* p, const float* g, float* m, float* v, float* teacher, const void* nodecay4, long n, const float* hyper,
                      void* stream);
/* Per-parameter-group learning-rate / weight-decay scales (VTPTrainer(param_groups=...)): vtp_adamw_dev_masked and vtp_adamw_ema_dev
 * with a group index in place of the exemption flag.  group4: uint8 [n / 4], the group of elements [4i, 4i + 4) (parameters are padded
 * to 4 elements, so a float4 lies in one parameter); group_tab: DEVICE f32 [ngroups][2] rows {lr_scale, wd_scale}, 8-byte aligned,
 * 1 <= ngroups <= 256.  Group g runs torch.optim.AdamW with lr = hyper[0] * lr_scale[g] and weight_decay = hyper[4] * wd_scale[g]:
 * p *= 1 - lr_g * wd_g; m, v as in vtp_adamw_dev; p -= (lr_g / bc1) * m / (sqrt(v) / bc2_sqrt + eps).  lr_scale = 0 leaves p
 * bit-unchanged while m, v and the fused EMA teacher still move (torch with lr = 0).  Rows {(1,1), (1,0)} with group4 = nodecay4
 * reproduce the masked entry points bit for bit.  An index >= ngroups in group4 is clamped to the last row by the kernels (the table
 * is never read past its end).  The table is device memory like hyper: a captured hipGraph replays with the values of each step.
 * Same argument checks and error codes as their siblings; group4 and group_tab must not be NULL. */
int vtp_adamw_dev_grouped(float* p, const float* g, float* m, float* v, void* p_bf16, const void* group4, const float* group_tab,
                          int ngroups, long n, const float* hyper, void* stream);
int vtp_adamw_ema_dev_grouped(float* p, const float* g, float* m, float* v, float* teacher, const void* group4, const float* group_tab,
                              int ngroups, long n, const float* hyper, void* stream);
/* Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2): total_norm = ||g||_2 over every
 * gradient, coef = clamp(max_norm / (total_norm + 1e-6), max=1), g *= coef) in front of the AdamW kernels above, without float
 * atomics: bitwise reproducible for a given gradient and partials layout.
 * vtp_sumsq_partials: partials[j] = sum of g[i]^2 (fp64) over chunk j of g[0, n) (n % 4 == 0); writes vtp_sumsq_partials_count(n)
 *   partials, a number that depends on n only (one per 8192 elements).  Several ranges may share one partials buffer at different
 *   offsets.  Short-lived workgroups (one chunk each).
 * vtp_sum_partials: *sum = partials[0] + ... + partials[count - 1], fp64, in a fixed order (one workgroup).
 * vtp_grad_clip_finalize: the same sum, then with gs = hyper[7] (the gradient multiplier of vtp_adamw_dev / vtp_adamw_ema_dev) and
 *   max_norm = hyper[10]: *total_norm = gs * sqrt(sum), *coef = clamp(max_norm / (*total_norm + 1e-6), max=1) (NaN stays NaN, as in
 *   torch), hyper[7] = gs * coef -- the AdamW kernels launched behind it read the clipped multiplier. */
int vtp_sumsq_partials_count(long n);
int vtp_sumsq_partials(const float* g, long n, double* partials, void* stream);
int vtp_sum_partials(const double* partials, int count, double* sum, void* stream);
int vtp_grad_clip_finalize(const double* partials, int count, float* hyper, float* total_norm, float* coef, void* stream);
/* Skipping the optimizer step on a non-finite gradient norm (VTPTrainer(skip_nonfinite=True)), decided on the device: no host sync,
 * and a captured hipGraph replays the decision of each step.
 * state: DEVICE int32 [4], owned by the caller: state[0] = applied_steps (Adam's step count), state[1] = skipped_steps,
 *   state[2] = skip_now (1 when the step in flight is skipped, else 0), state[3] unused.
 * vtp_grad_clip_finalize_guarded: vtp_grad_clip_finalize (same *total_norm and *coef, bit for bit, the inf or NaN included), then
 *   skip = !isfinite(*total_norm) -- the reported f32 norm: a finite sum whose scaled root overflows f32 skips as well.  Skipped:
 *   hyper[7] keeps its value, skipped_steps += 1, skip_now = 1.  Applied: hyper[7] = gs * coef, applied_steps += 1, skip_now = 0.
 *   Either way it writes this step's bias corrections from the device counter, hyper[5] = (float)(1 - beta1^t) and hyper[6] =
 *   (float)sqrt(1 - beta2^t) with t = applied_steps after the increment (applied_steps + 1 on a skipped step, where nothing reads
 *   them), in fp64 with the power formed by squaring and multiplying.  betas: HOST double [2] = {beta1, beta2}, each in [0, 1), read
 *   during the call (they become launch arguments).
 * vtp_adamw_dev_guarded / vtp_adamw_ema_dev_guarded / vtp_ema_dev_guarded: the AdamW, AdamW + EMA and EMA launches above with
 *   skip = &state[2] (any DEVICE int32; must not be NULL): a non-zero *skip makes every workgroup return before its first store, so
 *   p, m, v, p_bf16 and teacher keep their bits (-0.0 and NaN payloads included); *skip == 0 gives the unguarded entry point's bits.
 *   group_tab == NULL: idx4 is nodecay4 of vtp_adamw_dev_masked / vtp_adamw_ema_dev (may be NULL) and ngroups is ignored;
 *   otherwise idx4 is group4 of the _grouped entry points (must not be NULL) and 1 <= ngroups <= 256. */
int vtp_grad_clip_finalize_guarded(const double* partials, int count, float* hyper, float* total_norm, float* coef, int* state,
                                   const double* betas, void* stream);
int vtp_adamw_dev_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, const void* idx4, const float* group_tab,
                          int ngroups, long n, const float* hyper, const int* skip, void* stream);
int vtp_adamw_ema_dev_guarded(float* p, const float* g, float* m, float* v, float* teacher, const void* idx4, const float* group_tab,
                              int ngroups, long n, const float* hyper, const int* skip, void* stream);
int vtp_ema_dev_guarded(float* t, const float* s, long n, const float* momentum, const int* skip, void* stream);

/* ---- CLIP text-tower glue + contrastive head (fp32; clip.hip) -------------------------------------------------
 * embed: x f32 [B*T, D] = table[ids] + pos (modeling_vtp.py:296-297); eot[b] = argmax_t ids[b,t] (text_global_pool
 * 'argmax', text_transformer.py:222-224).  ids are int64 [B, T].  bwd: d_table[ids] += dx (atomics), d_pos += sum_b dx. */
int vtp_embed_tokens(const long* ids, const float* table, const float* pos, float* x, int* eot, int B, int T, int D,
                     void* stream);
int vtp_embed_tokens_bwd(const long* ids, const float* dx, float* d_table, float* d_pos, int B, int T, int D, void* stream);
/* out f32 [B, D] = x[b*T + idx[b]] ; scatter: dx f32 [B*T, D] (and optional bf16 copy) = 0 except those rows = dy. */
int vtp_gather_rows(const float* x, const int* idx, float* out, int B, int T, int D, void* stream);
int vtp_scatter_rows(const float* dy, const int* idx, float* dx, void* dx_bf16, int B, int T, int D, void* stream);
/* Packed captions (causal text tower with arg-max pooling: the rows behind a caption's EOT are dead).  vtp_text_row_plan builds, on the
 * device, eot[b] = argmax_t ids[b, t] (first maximum), cu int32 [B + 1] = exclusive prefix sum of eot + 1 and rows[0] = cu[B]; caption b
 * is then the rows [cu[b], cu[b + 1]) of every packed token buffer (row cu[b] + t = its token t).  The packed variants of the four
 * kernels above read / write live rows only: the pooled row is cu[b + 1] - 1, and the scatter zeroes live rows only. */
int vtp_text_row_plan(const long* ids, int* eot, int* cu, int* rows, int B, int T, void* stream);
int vtp_embed_tokens_packed(const long* ids, const float* table, const float* pos, float* x, const int* cu, int B, int T, int D,
                            void* stream);
int vtp_embed_tokens_bwd_packed(const long* ids, const float* dx, float* d_table, float* d_pos, const int* cu, int B, int T, int D,
                                void* stream);
int vtp_gather_rows_packed(const float* x, const int* cu, float* out, int B, int D, void* stream);
int vtp_scatter_rows_packed(const float* dy, const int* cu, float* dx, void* dx_bf16, int B, int T, int D, void* stream);
/* F.normalize(x, dim=-1, eps) (modeling_vtp.py:276,310): y = x * inv_norm, inv_norm = 1 / max(||x||, eps); and its backward. */
int vtp_l2norm_fwd(const float* x, float* y, float* inv_norm, int B, int D, float eps, void* stream);
int vtp_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, float* dx, int B, int D, void* stream);
/* Contrastive loss (OpenCLIP ClipLoss, local_loss + gather_with_grad convention; NOT in the reference -> parity unpinned):
 *   logits_i2t = exp(ls) * img_local @ txt_all^T, logits_t2i = exp(ls) * txt_local @ img_all^T  (modeling_vtp.py:329),
 *   labels = label_offset + arange(B_local); loss_sum += 0.5 * (mean CE_i2t + mean CE_t2i).
 * Outputs (overwritten): d_img_local, d_txt_local [B_local, D]; d_img_all, d_txt_all [B_all, D] = the gradient this rank
 * contributes to EVERY rank's features (reduce-scatter them across ranks and add the local slice); d_logit_scale[0] +=
 * dL/d(logit_scale).  scratch: 2 * B_local * B_all floats.  All features f32, L2-normalised by the caller. */
int vtp_clip_loss(const float* img_local, const float* txt_local, const float* img_all, const float* txt_all,
                  const float* logit_scale, int B_local, int B_all, int D, int label_offset, float* loss_sum,
                  float* d_img_local, float* d_txt_local, float* d_img_all, float* d_txt_all, float* d_logit_scale,
                  float* scratch, void* stream);

/* ---- loss-head variants the reference names but does not ship (parity unpinned, KATs = fp64 restatements) ----
 * SigLIP (vtp.py:180,185-188 creates `logit_bias` when init_logit_bias is set; OpenCLIP SigLipLoss):
 *   z = exp(logit_scale) <I_m, T_n> + logit_bias, y = +1 on matching pairs else -1, loss = weight * sum softplus(-y z).
 *   vtp_clip_logits writes exp(ls) <A_m, B_n>; vtp_siglip_pairs turns them IN PLACE into G = dloss/dz and accumulates loss,
 *   d log-scale and d bias; vtp_clip_grad_rows / _cols map G back to the feature gradients (local rows / gathered columns). */
int vtp_clip_logits(const float* A, const float* B, const float* logit_scale, float* logits, int M, int N, int D, void* stream);
int vtp_clip_grad_rows(const float* G, const float* B, const float* logit_scale, float* out, int M, int N, int D, int accumulate,
                       void* stream);
int vtp_clip_grad_cols(const float* G, const float* A, const float* logit_scale, float* out, int M, int N, int D, int accumulate,
                       void* stream);
int vtp_siglip_pairs(float* logits, const float* logit_bias, int B_local, int B_all, int label_offset, float weight,
                     float* loss_sum, float* d_logit_scale, float* d_logit_bias, void* stream);
/* KoLeo (DINOv2 KoLeoLoss) on L2-normalised rows xn [B, D]: loss += -weight * sum_i log(|xn_i - xn_nn(i) + 1e-8| + eps), nn(i) = the
 * other row with the largest dot product; d_xn (ACCUMULATED) receives the gradient w.r.t. xn (both ends of every pair). */
int vtp_koleo(const float* xn, int* nn_scratch, float* d_xn, float* loss_sum, int B, int D, float weight, float eps, void* stream);
/* Sinkhorn-Knopp centring (DINOv2 sinkhorn_knopp_teacher): probs bf16 [T, K] from teacher logits bf16 [T, K] at temperature
 * 1 / inv_temp, n_iters alternating normalisations over prototypes and samples (count = total samples; count_dev / n_rows_dev:
 * the same from device memory for padded buffers).  u [T], v [K], scratch [8 + K + T] f32.  phase -1 = everything (one process);
 * phases 0..3 expose the steps between which a data-parallel caller all-reduces scratch[0] (max), scratch[8..8+K) (sums). */
int vtp_sinkhorn_knopp(const void* logits, float inv_temp, void* probs, float* u, float* v, float* scratch, int T, int K, float count,
                       const float* count_dev, const int* n_rows_dev, int n_iters, int phase, void* stream);

/* ---- fp8 forward path (BASELINE config 5: VTP-L encode -> decode with fp8 MFMA; fp8.hip, gemm8p.hip) --------
 * e4m3 = the OCP fp8 format of gfx950, per-tensor scales:  q = e4m3(clamp(x * scale, -448, 448)).
 * vtp_quantize_e4m3: src bf16 (src_is_f32 = 0) or f32 [n] -> dst bytes [n]; scale from device memory (scale_dev) or the argument.
 *   +-inf saturates to +-448; a NaN leaves as a NaN code (S.1111.111), here and in vtp_norm_fwd_e4m3.
 * vtp_amax: amax[0] = max(amax[0], max |src|)  (calibration of the scales); a NaN in src leaves a NaN in amax[0].
 * vtp_dequantize_e4m3: bytes -> f32 * inv_scale.
 * vtp_gemm_nt_fp8: C[M,N] = alpha * A8[M,K] B8[N,K]^T (+ bias, + residual | SwiGLU), epilogues VTP_EPI_BF16 / F32 / SWIGLU as
 *   in vtp_gemm_nt, alpha = 1 / (scale_A * scale_B); K, lda, ldb in fp8 elements, multiples of 16; rope_pos / rope_sin / rope_cos /
 *   rope_cols (or nulls / 0): apply_rope fused into the bf16 epilogue exactly as in vtp_gemm_qkv_rope.  M x lda and N x ldb bytes
 *   must stay below 4 GiB (32-bit staging offsets; there is no other kernel to fall back to). */
/* norm_fwd with the quantisation fused: y8[M, D] = e4m3(bf16(norm(x)) * q_scale[0]) (q_scale in device memory) */
int vtp_norm_fwd_e4m3(const float* x, const float* w, const float* b, void* y8, const float* q_scale, float* stats, int M, int D,
                      float eps, int kind, void* stream);
int vtp_quantize_e4m3(const void* src, int src_is_f32, void* dst, long n, const float* scale_dev, float scale, void* stream);
int vtp_amax(const void* src, int src_is_f32, long n, float* amax, void* stream);
int vtp_dequantize_e4m3(const void* src, float* dst, long n, float inv_scale, void* stream);
int vtp_gemm_nt_fp8(const void* A8, int lda, const void* B8, int ldb, void* C, int ldc, void* C2, int ldc2, const float* bias,
                    const float* resid, int M, int N, int K, int epilogue, float alpha, const int* rope_pos, const void* rope_sin,
                    const void* rope_cos, int rope_cols, void* stream);

/* ---- tokenizer boundary (tokenizer.hip): the byte-image ends of generation/tokenizer/vtp_tokenizer.py --------
 * vtp_u8_to_images: ToTensor + Normalize(mean, std) (+ horizontal flip) of img_transform (vtp_tokenizer.py:74-81):
 *   img[b,c,y,x] = (float(u8[b,y,xs,c]) / 255 - mean[c]) / std[c], xs = flip ? W-1-x : x.   u8 NHWC -> f32 NCHW, W % 4 == 0.
 * vtp_images_to_u8: the tail of decode_to_images (vtp_tokenizer.py:105-111): Normalize(sub, div) -> * 255 -> clamp(0,255) ->
 *   uint8 (truncation) -> NHWC.   mean3 / std3 / sub3 / div3 are HOST pointers to 3 floats.
 * vtp_latent_channel_stats: sums[0..C) += sum, sums[C..2C) += sum of squares of latents f32 [B, C, hw] per channel, in fp64
 *   (the latents_stats.pt mean / std of the LightningDiT latent dataset, extract_features_vtp.py:124-126). */
int vtp_u8_to_images(const void* u8_nhwc, float* img_nchw, long B, int H, int W, const float* mean3, const float* std3, int flip,
                     void* stream);
int vtp_images_to_u8(const float* img_nchw, void* u8_nhwc, long B, int H, int W, const float* sub3, const float* div3, void* stream);
int vtp_latent_channel_stats(const float* latents, double* sums, long B, int C, int hw, void* stream);

/* ---- self-supervised (DINO / iBOT) head (ssl.hip) -----------------------------------------------------------
 * Token buffers of VTP.get_teacher_forward_outputs / get_student_ssl_outputs (vtp.py:432-439,470-473):
 * dst bf16 [T, D] row t = src row idx[t] (idx[t] < 0: zero row); scatter is the backward (indices are unique). */
int vtp_gather_token_rows(const void* src, const int* idx, void* dst, int T, int D, void* stream);
int vtp_scatter_token_rows(const void* d_dst, const int* idx, void* d_src, int T, int D, void* stream);
/* weight_norm(Linear(C -> K, bias=False)) of DINOHead.last_layer (dino_head.py:47-49): weff bf16 [K,C] = g * v / ||v||_row,
 * weffT bf16 [C,K] (optional), inv_norm f32 [K] = 1/||v||.  bwd: given dW_eff f32 [K,C]: dv += ..., dg += <dW, v/||v||>. */
int vtp_weight_norm_prep(const float* v, const float* g, void* weff, void* weffT, float* inv_norm, int K, int C, void* stream);
int vtp_weight_norm_bwd(const float* dW, const float* v, const float* g, const float* inv_norm, float* dv, float* dg, int K, int C,
                        void* stream);
/* teacher targets: probs bf16 [T,K] = softmax((logits - center) * inv_temp) row-wise (center f32 [K] or NULL). */
int vtp_softmax_center(const void* logits, const float* center, float inv_temp, void* probs, int T, int K, void* stream);
/* the same with the inverse temperature read from device memory (teacher-temperature schedules under hipGraph replay) */
int vtp_softmax_center_dev(const void* logits, const float* center, const float* inv_temp, void* probs, int T, int K, void* stream);
/* student cross-entropy (DINO cls / iBOT patch loss; OUR spec, DINOv2 convention): for student row r with teacher target rows
 * t_idx0[r], t_idx1[r] (-1 = none; t_idx0 < 0 or row_weight 0 = padding row):
 *   loss_sum += w_r * sum_targets( -sum_k p_t[k] * log_softmax(s_r * inv_temp)[k] ),
 *   d_student_logits[r] = w_r * inv_temp * (n_targets * softmax(s_r * inv_temp) - sum_targets p_t)     (bf16). */
int vtp_dino_ce(const void* student_logits, const void* teacher_probs, const int* t_idx0, const int* t_idx1,
                const float* row_weight, float inv_temp, float* loss_sum, void* d_student_logits, int T, int K, void* stream);
/* center = momentum * center + (1 - momentum) * col_sum * inv_count   (teacher-output centering, f32 [K]). */
int vtp_center_ema(float* center, const float* col_sum, float inv_count, const float* count_ptr, float momentum, int K,
                   void* stream);  /* count_ptr != NULL: inv_count = 1 / max(*count_ptr, 1) read on the device */

/* ---- LPIPS perceptual distance (reference: vtp/utils/lpips.py:61-175; VGG16 taps relu1_2 .. relu5_3) ----------------------
 * Activations are zero-bordered NHWC stacks, bf16 [NB, H+2, W+2, C] flattened to pixel rows, preceded and followed by
 * >= W+3 guard rows of zeros; every pointer below addresses row 0 of the stack (after the guard).
 *
 * vtp_conv3x3: y = epilogue(conv3x3_pad1(x)) as an implicit GEMM on the MFMA GEMM kernel.  w bf16 [Cout, taps*Cin] with the
 *   reduction index ordered (ky, kx, ci); taps = 9, or 1 for rows that are already unfolded (first VGG layer: Cin = 32 =
 *   27 unfolded values + 5 zeros, replaces nn.Conv2d(3, 64, 3, padding=1)).  mode 0: y = relu(acc + bias), border rows = 0
 *   (Conv2d + ReLU, lpips.py:131-146).  mode 1 (input gradient; w = flipped-tap transposed weights): y = acc masked by
 *   relu_mask > 0 (bf16 [rows, Cout], the activation this gradient flows into; NULL = no ReLU in front), border rows = 0. */
int vtp_conv3x3(const void* x, const void* w, const float* bias, void* y, const void* relu_mask, int NB, int H, int W, int Cin,
                int Cout, int taps, int mode, void* stream);
/* first-layer unfold with ScalingLayer (lpips.py:103-114) fused: source = reconstruction tokens bf16 [n*hw, 768] (tok; the
 * PixelShuffle(16) of pixel_decoder.py:158-161 is folded into the addressing) or an f32 NCHW image [n,3,H,W] (img); exactly
 * one is non-NULL.  out bf16 [n*(H+2)*(W+2), 32].  shift / scale: host float[3]. */
int vtp_lpips_unfold3(const void* tok, const float* img, void* out, int n, int H, int W, const float* shift, const float* scale,
                      void* stream);
/* dt bf16 [n*hw, 768] += fold(dA bf16 [n*(H+2)*(W+2), 32]) / scale_c: gradient of vtp_lpips_unfold3 w.r.t. tok. */
int vtp_lpips_fold3_bwd(const void* dA, void* dt, int n, int H, int W, const float* scale, void* stream);
/* nn.MaxPool2d(2, 2) on the bordered layout; bwd fuses the ReLU mask of Y and an optional tap gradient:
 * dY = (Y > 0) * (route(dP) + tap), route = first maximum of each 2x2 window in row-major order. */
int vtp_maxpool2_fwd(const void* in, void* out, int NB, int H, int W, int C, void* stream);
int vtp_maxpool2_bwd(const void* Y, const void* dP, const void* tap, void* dY, int NB, int H, int W, int C, void* stream);
/* one LPIPS tap: val[b] += mean_pixels sum_c w_c (f0/|f0| - f1/|f1|)^2_c  (normalize_tensor + NetLinLayer + spatial_average,
 * lpips.py:84-100,169-175); df0 (bf16, may be NULL) = gscale * d val / d f0, masked by f0 > 0.  f0, f1 bf16 [n*(H+2)*(W+2), C]. */
int vtp_lpips_tap(const void* f0, const void* f1, const float* w, float* val, void* df0, int n, int H, int W, int C,
                  float gscale, void* stream);

/* ---- linear probing (probe.hip; reference: tools/test_linear_probing_hf.py) ----------------------------------------------
 * Every classifier of a feature group in one fused step, fp32 in and out on the f32-input MFMA (the reference keeps this
 * arithmetic in fp32, outside its autocast context).  Heads are stacked: W f32 [N = H*C, K] row-major, bias f32 [N].
 * K % 4 == 0, ldx % 4 == 0, ldx >= K, X and W 16-byte aligned (X is a column slice of a wider matrix); B, C >= 1 arbitrary.
 *
 * logits[b, n] = sum_k X[b, k] * W[n, k] + bias[n]   (LinearClassifier.forward, :164-170, for every head of the group at once) */
int vtp_probe_logits(const float* X, int ldx, const float* W, const float* bias, float* logits, int ldl, int B, int N, int K,
                     void* stream);
/* per head h < H and row b < B: CrossEntropyLoss(mean) of logits[b, h*C : (h+1)*C] against labels[b] in [0, C)  (:285, :489)
 *   loss[h]    += sum_b CE * inv_rows
 *   correct[h] += #{b : argmax == labels[b]}, lowest index on ties (torch.argmax; :327-328)   -- NULL: not counted
 *   dlogits[b, h*C + c] = (softmax - onehot) * inv_rows  (row stride ldl)                      -- NULL: evaluation, not written */
int vtp_probe_ce(const float* logits, int ldl, const long* labels, int B, int H, int C, float inv_rows, float* loss, int* correct,
                 float* dlogits, void* stream);
/* torch.optim.SGD(momentum, weight_decay 0, dampening 0) step of every head from dlogits and X; dW is never stored (:487, :288-290):
 *   dW[n, k] = sum_b dlogits[b, n] * X[b, k];  db[n] = sum_b dlogits[b, n]
 *   mW = fmaf(momentum, mW, dW);  W = fmaf(-lr[n / C], mW, W)      (the same for mb / bias; lr f32 [H] in DEVICE memory)
 * Zeroed momentum buffers make the first step torch's (buf = grad).  Each element of W, mW, bias, mb has exactly one writer. */
int vtp_probe_sgd(float* W, float* bias, float* mW, float* mb, const float* dlogits, int ldl, const float* X, int ldx, const float* lr,
                  int B, int H, int C, int K, float momentum, void* stream);

/* ---- linear segmentation probe (segprobe.hip): a linear layer on frozen patch tokens, logits upsampled bilinearly to the label
 * map, per-pixel cross-entropy, confusion counts for mIoU -- the protocol of the DINOv2 / iBOT papers restated (parity with their
 * programs is unpinned).  Z f32 [M = B*h*w, H*C] (row stride ldz) are the low-resolution logits of vtp_probe_logits, token row
 * (b, i, j) at b*h*w + i*w + j; labels u8 [B, Hl, Wl] with any Hl, Wl >= 1; 1 <= C <= 255.  A label equal to ignore_index is
 * skipped; a label >= C that is not ignore_index is skipped too and counted as out of range.  Upsampling is ATen's
 * upsample_bilinear2d(align_corners=False): per axis scale = (float)in / out, src = max(scale * (dst + 0.5f) - 0.5f, 0), i0 =
 * (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1; value = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11).
 * Nothing of size [B, C, Hl, Wl] is stored and no float is accumulated with atomics: every result repeats bit for bit.
 *
 * vtp_seg_ce, per head h < H over the valid pixels p of the batch (n_valid of them):
 *   loss[h]        = sum_p (lse(z_p) - z_p[y_p]) / n_valid, 0 without a valid pixel            (overwritten)
 *   lse[h,b,y,x]   = log-sum-exp of the interpolated logits, f32 [H, B, Hl, Wl]                -- NULL: evaluation, not written
 *   conf[h,t,c]   += #{p : y_p = t, argmax z_p = c}, lowest index on ties; int64 [H, C, C]     -- NULL: not counted
 *   call_counts    = (n_valid, out of range) of this call, i32 [2]                             (overwritten)
 *   totals        += the same two, int64 [2]                                                   -- NULL: not kept
 * workspace: vtp_seg_ce_workspace_bytes(...) bytes, 4-byte aligned (one loss partial per workgroup and head, folded in workgroup
 * order); that function returns the bytes, or -1 (bad argument or more than 2 GiB). */
int vtp_seg_ce_workspace_bytes(int B, int h, int w, int Hl, int Wl, int H, int C);
int vtp_seg_ce(const float* Z, int ldz, const unsigned char* labels, int B, int h, int w, int Hl, int Wl, int H, int C,
               int ignore_index, float* lse, long* conf, float* loss, int* call_counts, long* totals, void* workspace,
               long workspace_bytes, void* stream);
/* G[(b,i,j), h*C + c] = (1 / n_valid) sum_p w_p(i,j) (exp(z_p[c] - lse_p) - [y_p = c]) over the valid pixels that have cell (i, j)
 * among their four taps (row stride ldg); lse and call_counts as vtp_seg_ce left them.  A gather: one writer and one summation
 * order (raster) per element; a cell without a pixel in its support gets exactly 0, and so does everything when n_valid is 0. */
int vtp_seg_dlogits(const float* Z, int ldz, const unsigned char* labels, const float* lse, const int* call_counts, float* G, int ldg,
                    int B, int h, int w, int Hl, int Wl, int H, int C, int ignore_index, void* stream);
/* vtp_probe_sgd's step for M token rows: dW = G^T X and db = column sums of G are formed in slices of vtp_seg_sgd_slice() rows
 * (a constant of the kernel, a multiple of 64), each a k-ordered fmaf chain written to the workspace; the slices are added in
 * ascending order by one owner per element, which applies mW = fmaf(momentum, mW, dW); W = fmaf(-lr[n / C], mW, W) in the same
 * pass (likewise mb / bias).  The result depends on the inputs and the slice constant alone.  X f32 [M, K] with row stride ldx:
 * K % 4 == 0, ldx % 4 == 0, ldx >= K; X, W, mW and the workspace 16-byte aligned.  workspace: vtp_seg_sgd_workspace_bytes(M, N = H*C, K)
 * bytes (returns -1 for a bad argument or more than 2 GiB: pass fewer heads per call). */
int vtp_seg_sgd_slice(void);
int vtp_seg_sgd_workspace_bytes(int M, int N, int K);
int vtp_seg_sgd(float* W, float* bias, float* mW, float* mb, const float* G, int ldg, const float* X, int ldx, const float* lr, int M,
                int H, int C, int K, float momentum, void* workspace, long workspace_bytes, void* stream);

/* ---- linear depth probe (depthprobe.hip): a linear layer on frozen patch tokens whose 2 <= C <= 1024 outputs per head are uniform
 * bins of depth, logits upsampled bilinearly to the label map exactly as above (the same tap and blend functions), AdaBins' linear
 * normalisation and the scale-invariant log loss of Eigen et al. -- the DINOv2 "lin." depth protocol restated from the papers
 * (parity with their programs is unpinned).  Z f32 [M = B*h*w, H*C] as for the segmentation probe; gt f32 [B, Hl, Wl] metric depth.
 * Bin centres e_c = min_depth + ((max_depth - min_depth) * c) / (C - 1) in fp32, 0 < min_depth < max_depth.  Per pixel p and head:
 *   a_c = max(z_p[c], 0) + 0.1;  S_p = sum_c a_c;  dhat_p = (sum_c a_c e_c) / S_p   (both sums in ascending c, the second an fmaf chain)
 * A pixel is valid iff gt_p > 0 && gt_p <= max_depth (NaN and inf are invalid); n = valid pixels of the call.  Over the valid pixels
 *   g_p = logf(dhat_p) - logf(gt_p);  m1 = sum g / n;  m2 = sum g^2 / n   (fp64: one partial per workgroup, folded in workgroup order)
 *   L = sqrt(max(m2 - lam * m1^2, 0)), 0 when n = 0.
 * No atomics: every result repeats bit for bit.
 *
 * vtp_depth_pix:
 *   dhat[h,b,y,x]   f32 [H, B, Hl, Wl], written for EVERY pixel, valid or not                      -- NULL: not written
 *   aux             opaque per-pixel planes for vtp_depth_dlogits,
 *                   vtp_depth_pix_workspace_bytes(..., aux_plane = 1) bytes                        -- NULL: an evaluation call
 *   loss[h]         = (float)L                                                                     (overwritten)
 *   stats[h]        = (n, m1, m2, L), f64 [H, 4]                                                   (overwritten)
 *   eval_counts[h] += (valid, #{max(dhat/gt, gt/dhat) < 1.25^k}, k = 1, 2, 3), int64 [H, 4]        -- NULL (both): not kept
 *   eval_sums[h]   += sums over the valid pixels of |dhat-gt|/gt, (dhat-gt)^2/gt, (dhat-gt)^2, formed in fp64 from the fp32 dhat,
 *                     stored as f64 [H, 6] = (g, g^2, abs_rel, sq_rel, sq, |g| / ln 10).  Each image's sums are formed in the tile
 *                     order of the image alone and one owner adds them to the accumulator image by image in batch order: any split
 *                     of an image sequence into batches leaves the same bits.
 * gt may be NULL when dhat is given (prediction: only dhat is written; loss, stats and workspace may then be NULL too).
 * workspace: vtp_depth_pix_workspace_bytes(..., aux_plane = 0) bytes, 8-byte aligned; that function returns the bytes, or -1 (bad
 * argument or more than 2 GiB). */
int vtp_depth_pix_workspace_bytes(int B, int h, int w, int Hl, int Wl, int H, int C, int aux_plane);
int vtp_depth_pix(const float* Z, int ldz, const float* gt, int B, int h, int w, int Hl, int Wl, int H, int C, float min_depth,
                  float max_depth, float lam, float* dhat, float* aux, float* loss, double* stats, long* eval_counts, double* eval_sums,
                  void* workspace, long workspace_bytes, void* stream);
/* G[(b,i,j), h*C + c] = sum_p w_p(i,j) q_p [z_p[c] > 0] (e_c - dhat_p),  q_p = (g_p - lam m1) / (n L dhat_p S_p), over the valid pixels
 * that have cell (i, j) among their four taps (row stride ldg); aux and stats as vtp_depth_pix left them, z_p[c] re-blended from the
 * cell's 3 x 3 neighbourhood.  A gather: one writer and one raster-order sum per element; a cell without support gets exactly 0, and
 * so does everything when n = 0 or L = 0. */
int vtp_depth_dlogits(const float* Z, int ldz, const float* aux, const double* stats, float* G, int ldg, int B, int h, int w, int Hl,
                      int Wl, int H, int C, float min_depth, float max_depth, float lam, void* stream);
/* vtp_seg_sgd for 1 <= C <= 1024: the same two kernels through the same launcher, the same bits for the same operands. */
int vtp_depth_sgd_workspace_bytes(int M, int N, int K);
int vtp_depth_sgd(float* W, float* bias, float* mW, float* mb, const float* G, int ldg, const float* X, int ldx, const float* lr, int M,
                  int H, int C, int K, float momentum, void* workspace, long workspace_bytes, void* stream);

/* ---- zero-shot classification (zeroshot.hip; reference: tools/test_zero_shot_hf.py at precision 'fp32') ------------------
 * The tool's own arithmetic, fp32 in and out, products on the f32-input MFMA.  D % 4 == 0, leading dimensions % 4 == 0 and
 * >= D, feat / F / Wt 16-byte aligned.  The classifier is kept as Wt f32 [C, D] (one row per class); the tool's [D, C]
 * classifier is its transposed view.
 *
 * Wt[c] = normalize(mean_t feat[c*T + t]) : the sum runs over t = 0..T-1 in order and is divided by T, then the row is divided
 * by max(||row||_2, eps) (F.normalize; :383-385).  An all-zero class gives a zero row.  Rows are independent of each other and
 * of C, so class batches may fill one Wt call by call. */
int vtp_zs_class_mean(const float* feat, int ldf, float* Wt, int ldw, int C, int T, int D, float eps, void* stream);
/* z[b, c] = sum_k (scale * F[b, k]) * Wt[c, k] (the feature scaled and rounded first: (100.0 * f) @ classifier, :436; one
 * sequential chain over k per element) and accuracy(z, targets, (1, 5)) (:312-316) in ONE launch, no host synchronisation:
 *   rank[b] = #{c : z[b,c] > z[b,t]} + #{c < t : z[b,c] == z[b,t]}, t = targets[b] (the lower index wins a tie);
 *             t outside [0, C) reads nothing, gets rank C and counts as a miss
 *   counts    int64 [3]   += #{rank < 1}, #{rank < 5}, B
 *   per_class int32 [2,C] += rows seen / top-1 hits per target class (targets in range only)        -- may be NULL
 *   rank      int32 [B]                                                                              -- may be NULL
 *   pred      int32 [B,5]  the five best classes by (logit descending, index ascending)              -- may be NULL
 *   logits    f32 [B,C], row stride ldl: exactly the values the ranks were computed from             -- may be NULL
 * counts may be NULL as well; a NULL output changes no other output.  B >= 1, C >= 5 (any size: a row block's logits are
 * kept in LDS 1024 classes at a time).  Only integer atomics: counts and ranks are reproducible bit for bit. */
int vtp_zs_topk(const float* F, int ldf, const float* Wt, int ldw, const long* targets, float scale, int B, int C, int D,
                long* counts, int* per_class, int* rank, int* pred, float* logits, int ldl, void* stream);

/* ---- reconstruction evaluation (recon_eval.hip; reference: tools/test_reconstruction_hf.py:360-409) -----------------------
 * images / recon f32 [B,3,H,W], ImageNet-normalised as get_latents_decoded_images returns them; H, W >= 11, W % 4 == 0, both
 * 16-byte aligned.  sub3 / div3: HOST float[3], fp32(-mean/std) and fp32(1/std) (transform_rev, :265-268).  Every output is
 * formed from d = clamp((x - sub[c]) / div[c], 0, 1) (:371-376), a subtraction, an IEEE division and the clamp:
 *   ref_u8 / rec_u8  uint8 [B,H,W,3] = (uint8) trunc(d * 255.0f), bit-identical to (:401-402)               -- may be NULL
 *   ref_lp / rec_lp  f32 [B,3,H,W]   = d * 2 - 1, bit-identical to (:381-382)                                -- may be NULL
 *   scratch          f64 [B, tiles, 2]: per tile of an image the sum of (o*255 - r*255)^2 over the pixels the tile owns (every
 *                    pixel of the image has exactly one owner; :395-397) and the sum of the SSIM map over its window positions
 * SSIM: 11x11 Gaussian window (sigma 1.5, sum 1), c1 = 1e-4, c2 = 9e-4, var = max(E[x^2] - mu^2, 0) for both variances, the
 * covariance unclamped, ssim = ((2 mu_p mu_t + c1)(2 cov + c2)) / ((mu_p^2 + mu_t^2 + c1)(var_p + var_t + c2)) at each of the
 * (H-10) x (W-10) window positions of each channel: StructuralSimilarityIndexMeasure(data_range=1.0), whose reflect-pad,
 * convolution and crop is this valid convolution (:392).  Windowed sums in fp64.  No atomics: results repeat bit for bit.
 * vtp_recon_scratch_doubles returns the number of doubles scratch must hold (2 * B * tiles), or -1. */
int vtp_recon_scratch_doubles(long B, int H, int W);
int vtp_recon_metrics(const float* images, const float* recon, long B, int H, int W, const float* sub3, const float* div3,
                      void* ref_u8, void* rec_u8, float* ref_lp, float* rec_lp, double* scratch, long scratch_len, void* stream);
/* One small launch after vtp_recon_metrics (and after LPIPS, if its values are passed): per image b, tiles summed in order,
 *   psnr[b] = 20 log10(255 / sqrt(sse / (3 H W))), +inf when sse == 0 (calculate_psnr, :49-63);  ssim[b] = sum / (3 (H-10)(W-10))
 *   sse[b]  (f64) the squared error itself                                                                    -- may be NULL
 * and adds to acc, f64 [8] on the device (the tool averages PSNR over images, SSIM and LPIPS over batch means: :386, :392,
 * :395-397, :428-430; both kinds of sum are kept):
 *   acc[0] sum of psnr   acc[1] images   acc[2] images with sse == 0   acc[3] sum of ssim   acc[4] sum of per-batch mean ssim
 *   acc[5] batches       acc[6] sum of per-batch mean lpips            acc[7] sum of lpips   (6, 7 only with lpips f32 [B]) */
int vtp_recon_finalize(const double* scratch, long scratch_len, long B, int H, int W, float* psnr, float* ssim, double* sse,
                       const float* lpips, double* acc, void* stream);

/* ---- SSL crops (augment.hip): the DINO multi-crop augmentation from decoded byte images, two launches, no host synchronisation
 * src_u8 uint8 [B,Hs,Ws,3] (RGB, 4-byte aligned, Ws % 4 == 0) -> out f32 [N,3,S,S], N = views * B, crop n from image n % B
 * (view-major).  table f32 [N,16] on the DEVICE, 16-byte aligned, one row per crop:
 *   0..3 y0 x0 h w (the box)   4 flags (1 flip | 2 colour jitter | 4 grayscale | 8 solarize)
 *   5..8 the jitter's operations in the order they run (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none)
 *   9..12 the factors (brightness, contrast, saturation, hue)   13 sigma of the blur (<= 0: none)   14, 15 unused
 * In fp32 on x = u8 / 255:  crop the box and resize it to S x S as F.interpolate(mode="bicubic", antialias=True,
 * align_corners=False) does (a = -0.5, support 2 max(box / S, 1), taps outside the box dropped and the rest renormalised), clamp
 * to [0, 1]; flip; the jitter with blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1), gray = 0.2989 r + 0.587 g + 0.114 b (brightness
 * blend(x, 0, f); contrast blend(x, mean of gray over the crop as it stands, f); saturation blend(x, gray, f); hue by
 * torchvision's _rgb2hsv, h = (h + f) % 1, _hsv2rgb); grayscale; a 9 x 9 Gaussian blur (weights exp(-0.5 (t / sigma)^2) / sum,
 * reflect padding by 4, separable); solarize (x >= 128/255 ? 1 - x : x); (x - mean3[c]) / std3[c].  mean3 / std3: HOST float[3].
 * A box is clamped into the image and to 8 S per axis (the host refuses such a table).  S >= 5.  The contrast mean comes from
 * per-tile fp64 sums added in a fixed order: no float atomics, results repeat bit for bit.  Every output element is written once.
 * vtp_augment_scratch_floats returns the number of floats scratch must hold (the resampled crops and the tile sums), or -1. */
int vtp_augment_scratch_floats(long N, int S);
int vtp_augment_crops(const void* src_u8, long B, int Hs, int Ws, const float* table, long N, int S, const float* mean3,
                      const float* std3, float* out, float* scratch, long scratch_len, void* stream);

/* ---- Preprocessing (preprocess.hip): PIL's 8-bit Image.resize (BOX / BILINEAR / BICUBIC), crop, flip and ToTensor + Normalize over
 * a ragged batch of decoded byte images, bit for bit -- one launch per pass over the whole batch, no host synchronisation.
 * src_u8: the images' bytes (RGB, [H_i, W_i, 3] each) back to back, src_len bytes, on the device.  scratch: scratch_len bytes for
 * the uint8 intermediates (may be NULL when there is one launch).  jobs int64 [n, 16] on the DEVICE, 8-byte aligned, one row per
 * pass of one image:
 *   0 src byte offset (source buffer, or scratch with flag 1)   1 dst byte offset in scratch; last launch: the image's index
 *   2, 3 output height, width of the pass   4, 5 source bytes per output row, column   6 bytes between two taps
 *   7 index in tab of the pass's first (min, n) pair   8 index in tab of its first coefficient   9 coefficients per entry
 *   10 subtracted from min   11 flags (1 source in scratch | 2 the table runs along y | 4 flip)   12 first block in its launch
 *   13..15 unused
 * tab int32 on the DEVICE: (min, n) pairs and 22-bit fixed-point coefficients, formed on the host in float64 as PIL's Resample.c
 * does.  Per pixel and channel acc = 2^21 + sum_j K[j] src[min + j] in int32, dst = clamp(acc >> 22, 0, 255).
 * launches: HOST int [n_launches, 3] = (first job, jobs, blocks); a block is 256 consecutive output pixels of one job; the last
 * launch has one job per image, Ho x Wo each, and writes out f32 [B,3,Ho,Wo] = (float(u8) / 255 - mean3[c]) / std3[c] (the expression
 * of vtp_u8_to_images) and, unless NULL, out_u8 uint8 [B,Ho,Wo,3].  mean3 / std3: HOST float[3].
 * The job rows cannot be checked here: the caller guarantees that every offset lies inside its buffer (vtp_amd.preprocess.check_jobs).
 * Every output element is written exactly once, without atomics: results repeat bit for bit. */
int vtp_preprocess(const void* src_u8, long src_len, void* scratch, long scratch_len, const long* jobs, const int* tab,
                   const int* launches, int n_launches, long B, int Ho, int Wo, const float* mean3, const float* std3, float* out,
                   void* out_u8, void* stream);

/* ---- FID (fid.hip): Inception-v3 features in exact fp32 and the Frechet statistics in fp64.  No float atomics, no split sums: every
 * result repeats bit for bit and does not depend on the batch size.
 * vtp_conv2d_f32: y[b, oy, ox, c0 + n] = act(bias[n] + sum_{ky, kx, ci} x[b, oy s - ph + ky, ox s - pw + kx, ci] w[n, ky, kx, ci]).
 *   x f32 NHWC [B, H, W, Cin]; w f32 [Cout, kh, kw, Cin] (BatchNorm folded in); bias f32 [Cout] or NULL; y f32 [B, Ho, Wo, Ctot], of
 *   which only the channels [c0, c0 + Cout) are written; Ho = (H + 2 ph - kh) / s + 1.  kh, kw in {1, 3, 5, 7}, stride 1 or 2, zero
 *   padding (ph, pw), relu != 0: max(., 0).  An implicit GEMM on v_mfma_f32_32x32x2_f32: every output element is ONE fmaf chain
 *   that starts at the bias and runs over k in the order (ky, kx, ci).  x and w 16-byte aligned when Cin % 4 == 0 (16-byte loads
 *   along Cin); any other Cin (the first layer's 3) takes scalar loads.
 * vtp_conv2d_f32_blocked: the same convolution with the sum over k taken in blocks of 32: every 32 consecutive k form a chain that
 *   starts at 0, and the block sums are added to the accumulator (which starts at the bias) in k order.  Rounding errors then grow
 *   with K / 32 + 32 rather than K (the fp32 LPIPS: K up to 4608); an output is still a fixed sequence of operations on its own
 *   row of x and of w, so it does not depend on the batch and repeats bit for bit.
 * vtp_pool3x3_f32: 3 x 3 pooling of x f32 NHWC [B, H, W, C] into the channels [c0, c0 + C) of y [B, Ho, Wo, Ctot].  stride 1 pads by
 *   1, stride 2 by 0.  mode 0 max (a NaN tap gives NaN, as F.max_pool2d), 1 average / 9 (the padding counts), 2 average over the taps inside.  C, c0, Ctot % 4 == 0.
 * vtp_global_avgpool_f32: x f32 [B, HW, C] -> y f32 [B, C], the pixels summed in order.
 * vtp_resize_bilinear_nhwc: y[b, oy, ox, c] = scale * bilinear(x[b, c])(oy, ox) + shift with F.interpolate's align_corners=False
 *   geometry; x f32 NCHW [B, C, H, W], y f32 NHWC [B, Ho, Wo, C].  Weights are exact rationals, the arithmetic fp64, one rounding.
 *   With Ho == H, Wo == W it is the NCHW -> NHWC repack.
 * vtp_fid_accum: sum[i] += feats[r, i] and outer[i, j] = fma(feats[r, i], feats[r, j], outer[i, j]) for r = 0 .. n - 1 in order, in
 *   fp64; feats f32 [n, D] with row stride ldf, sum f64 [D], outer f64 [D, D].  One thread owns each element: any split of the rows
 *   over calls leaves the same bits. */
int vtp_conv2d_f32(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, int kh,
                   int kw, int stride, int ph, int pw, int relu, int c0, int Ctot, void* stream);
int vtp_conv2d_f32_blocked(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, int kh,
                           int kw, int stride, int ph, int pw, int relu, int c0, int Ctot, void* stream);
int vtp_pool3x3_f32(const float* x, float* y, int B, int H, int W, int C, int stride, int mode, int c0, int Ctot, void* stream);
int vtp_global_avgpool_f32(const float* x, float* y, int B, int HW, int C, void* stream);
int vtp_resize_bilinear_nhwc(const float* x, float* y, int B, int C, int H, int W, int Ho, int Wo, float scale, float shift,
                             void* stream);
int vtp_fid_accum(const float* feats, int ldf, double* sum, double* outer, int n, int D, void* stream);

/* ---- fp32 inference forward (fp32.hip and fp32 variants of the row kernels): what the reference computes with fp32 weights and no
 * autocast.  Every tensor is f32; the products run on v_mfma_f32_32x32x2_f32.
 * vtp_gemm_nt_f32: C[M, N] = epi(A[M, K] W[N, K]^T).  Every output element is ONE fmaf chain over k = 0 .. K - 1 (no split of K, no
 *   atomics): its bits depend on its row of A and its row of W alone -- not on M or the batch the row came with -- and repeat from run
 *   to run.  Any M >= 1; N and K multiples of 8; lda, ldw multiples of 4; A, W, W2 16-byte aligned.  epi:
 *     0  C = acc + bias                                   (bias NULL: none)
 *     1  C = resid + gamma (.) (acc + bias)               (LayerScale gamma [N] or NULL; resid f32 [M, N], row stride ldr; may alias C)
 *     2  C[M, N] = silu(A W^T + bias) * (A W2^T + bias2)  (SwiGLU; W and W2 are [N, K], N = the hidden width)
 *     3  C = gelu_erf(acc + bias)        4  C = quick_gelu(acc + bias) = y / (1 + exp(-1.702 y))
 *   W2 / bias2 belong to epi 2 alone, gamma / resid to epi 1.
 * vtp_attn_fwd_f32: o = softmax(scale q k^T) v per (batch, head), head dimension 64; element strides as vtp_attn_fwd (batch sb, token
 *   sn, head h at + 64 h; o: sbo, sno), all multiples of 4, pointers 16-byte aligned.  Any N >= 1: keys past N (and key > query when
 *   causal != 0) are masked out of the softmax.  Online softmax in fp32; a sequence's result does not depend on the batch around it.
 * vtp_norm_fwd_f32: vtp_norm_fwd with the un-rounded f32 output.  vtp_rope_qk_f32: apply_rope (attention.py:70-89) in place on the q and
 *   k thirds of an f32 [B*N, 3*D] buffer: round to bf16, the arithmetic of vtp_rope_qk, widen back; v untouched.
 * vtp_im2col16_rows_f32 / vtp_pixel_shuffle16_f32 / vtp_pool_patch_rows_f32: the bf16 entry points' data movement on f32 rows. */
int vtp_gemm_nt_f32(const float* A, int lda, const float* W, int ldw, const float* W2, float* C, int ldc, const float* bias,
                    const float* bias2, const float* gamma, const float* resid, int ldr, int M, int N, int K, int epilogue, void* stream);
int vtp_attn_fwd_f32(const float* q, const float* k, const float* v, float* o, int B, int N, int heads, long sb, long sn, long sbo,
                     long sno, float scale, int causal, void* stream);
int vtp_norm_fwd_f32(const float* x, const float* w, const float* b, float* y, float* stats, int M, int D, float eps, int kind,
                     void* stream);
int vtp_rope_qk_f32(float* qkv, const void* sin, const void* cos, int B, int N, int heads, int prefix, void* stream);
int vtp_im2col16_rows_f32(const float* img, float* rows, int B, int H, int W, int prefix, void* stream);
int vtp_pixel_shuffle16_f32(const float* t, float* img, int B, int h, int w, void* stream);
int vtp_pool_patch_rows_f32(const float* x, float* out, int B, int N, int D, float scale, void* stream);

/* ---- LPIPS in exact fp32 for evaluation (lpips_f32.hip): what vtp/utils/lpips.py computes on fp32 tensors outside autocast (the
 * reconstruction tool's LPIPS_VTP).  Activations are f32 NHWC without borders; the 13 convolutions are vtp_conv2d_f32_blocked.  No float
 * atomics, nothing depends on the grid or the batch: a pair's value repeats bit for bit whatever it is batched with.
 * vtp_lpips_scale_nhwc_f32: ScalingLayer (lpips.py:103-114) and the repack: x f32 NCHW [B, 3, H, W] -> y f32 NHWC [B, H, W, Cout],
 *   y_c = (x_c - shift_c) / scale_c, one fp32 subtraction and one fp32 division.  Cout = 3, or 4: channel 3 is zero (16-byte stores,
 *   and the first convolution takes 16-byte loads on weights zero-padded to Cin = 4).  shift / scale: host float[3].
 * vtp_maxpool2_f32: nn.MaxPool2d(2, 2), x f32 NHWC [B, H, W, C] -> y [B, H / 2, W / 2, C]; H, W even, C % 4 == 0, 16-byte aligned.
 * vtp_lpips_head_f32: one tap.  f f32 [2 n, HW, C]: the ReLU features of image b and of image n + b; w f32 [C] (NetLinLayer).  Per
 *   pixel in fp32: a = f0 / (sqrt(sum_c f0^2) + 1e-10), b likewise from f1, s = sum_c w_c (a_c - b_c)^2 (an all-zero pixel gives 0).
 *   part f64 [n, ceil(HW / 256)]: part[b, j] = the sum of s over the pixels [256 j, 256 j + 256) of pair b, in a fixed order.
 *   C in {64, 128, 256, 512}.
 * vtp_lpips_finalize_f32: part f64 = the five taps' partial sums back to back, tap k as [n, ceil(HW_k / 256)] with HW_k =
 *   (H >> k) (W >> k); val[b] = (((r_0 + r_1) + r_2) + r_3) + r_4 in fp32, r_k = float(sum_j part_k[b, j] / HW_k), the segments
 *   summed in fp64 in a fixed order (lpips.py:90-100: spatial_average, val = res[0]; val += res[l]). */
int vtp_lpips_scale_nhwc_f32(const float* x, float* y, int B, int H, int W, int Cout, const float* shift, const float* scale,
                             void* stream);
int vtp_maxpool2_f32(const float* x, float* y, int B, int H, int W, int C, void* stream);
int vtp_lpips_head_f32(const float* f, const float* w, double* part, int n, int HW, int C, void* stream);
int vtp_lpips_finalize_f32(const double* part, float* val, int n, int H, int W, void* stream);

/* ---- weighted k-NN classification on frozen features (knn.hip): the DINO / DINOv2 evaluation protocol (k = 10, 20, 100, 200,
 * temperature 0.07, top-1 / top-5), restated from the papers' description; neither code base is a reference of this project, so
 * parity with those programs is unpinned.  Everything in exact fp32, no float atomics, no host synchronisation.
 *
 * vtp_knn_topk merges the chunk X f32 [N, D] (row stride ldx) of the bank, whose row 0 has the global index index_base, into the
 * running neighbour lists of the queries Q f32 [B, D] (row stride ldq).  Replaces torch.matmul over bank chunks + topk + cat +
 * topk; the [B, N] similarities are never written (except to sims_out).
 *   s[b, n] = the fmaf chain over k = 0 .. D-1 ascending, the bits of element [b, n] of vtp_gemm_nt_f32(Q, X) with the plain
 *   epilogue, whatever B, N, the chunk or the grid (no split of k).
 *   State, in and out: sims f32 [B, K] and idx int64 [B, K], contiguous: per query the first K bank rows seen so far under
 *   (similarity descending, global index ascending), in that order.  An empty entry is (-inf, -1) and empties come last: start
 *   from all-empty lists; there is no separate count.  The result is identical bit for bit whatever the chunking of the bank,
 *   the number of splits, B or the launch geometry.  Inputs are finite by contract; a NaN similarity is never selected.
 *   splits: the bank chunk is cut into that many slices, one workgroup per (slice, 128 queries); 0 picks a count that fills the
 *   chip.  workspace holds the slices' partial lists: vtp_knn_workspace_bytes(B, K, splits) bytes (for splits = 0: enough for
 *   whatever the heuristic picks at this B), 16-byte aligned; contents need not be kept between calls.
 *   sims_out (may be NULL): f32 [B, N], row stride lds: the chunk's similarities, for tests.
 *   Limits (those of vtp_gemm_nt_f32): D a positive multiple of 8, ldq and ldx multiples of 4, Q and X 16-byte aligned;
 *   1 <= K <= 256, 0 <= splits <= 1024.
 * vtp_knn_workspace_bytes returns the bytes, or -1 (bad argument, or more than 2 GiB: pass fewer queries per call).
 *
 * vtp_knn_vote turns the lists into statistics in one launch.  Replaces softmax + one_hot + mul + cumsum + topk(5) + eq + sum.
 *   labels int32 [n_total]: the class of every bank row; a neighbour whose index or label is out of range votes for nothing.
 *   targets int64 [B]; ks: HOST int[nk], ascending, 1 <= ks[m] <= K, nk <= 8; inv_T = 1 / temperature; num_classes >= 5.
 *   w_j = expf((s_j - s_0) * inv_T) (the protocol's softmax over the list without its common denominator: the same ranking);
 *   the score of class c at k = the sum of w_j over the first k neighbours with label c, added in neighbour order; a class without
 *   a neighbour has score 0.  Classes are ranked by (score descending, class index ascending), so a target with score 0 comes
 *   behind every positive class and every score-0 class of lower index.
 *   counts    int64 [nk, 3] += (top-1 hits, top-5 hits, rows), integer atomics only                       -- may be NULL
 *   rank_out  int32 [B, nk]   the number of classes ranked before the target; num_classes for a target outside
 *                             [0, num_classes), which is a miss at every k and still a row                 -- may be NULL
 *   pred_out  int32 [B, nk, 5] the five best classes                                                      -- may be NULL */
int vtp_knn_workspace_bytes(int B, int K, int splits);
int vtp_knn_topk(const float* Q, int ldq, const float* X, int ldx, long index_base, int B, int N, int D, int K, float* sims,
                 long* idx, void* workspace, long workspace_bytes, int splits, float* sims_out, int lds, void* stream);
int vtp_knn_vote(const float* sims, const long* idx, const int* labels, long n_total, const long* targets, const int* ks, int nk,
                 float inv_T, int num_classes, int B, int K, long* counts, int* rank_out, int* pred_out, void* stream);

/* ---- k-NN manifold precision / recall of two feature sets (precision_recall.hip): the estimate of Kynkaanniemi et al. 2019 that
 * the ADM evaluation suite reports with k = 3, restated from the paper's description; neither ADM's evaluator nor the authors' code
 * is a reference of this project, so parity with those programs is unpinned.  Everything in exact fp32, no float atomics, no host
 * synchronisation.
 *   s(a, b)  = the fmaf chain over k = 0 .. D-1 ascending, the bits of vtp_gemm_nt_f32 with the plain epilogue; n(a) = s(a, a).
 *   d2(a, b) = max((n(a) + n(b)) - 2 s(a, b), 0): symmetric bit for bit, exactly 0 for two identical rows.  A NaN stays a NaN, is
 *   never selected and never a hit; inputs are finite by contract.
 *
 * vtp_pr_sqnorm: out[i] = n(row i of X f32 [N, D], row stride ldx).
 *
 * vtp_pr_knn_dist merges the chunk X f32 [N, D] (row stride ldx, norms xn f32 [N]) of a bank into dist f32 [B, 8], contiguous and
 * 16-byte aligned: per query of Q f32 [B, D] (row stride ldq, norms qn f32 [B]) the 8 smallest d2 seen so far, ascending, +inf for
 * an empty entry.  dist is in/out: fill it with +inf before the first chunk.  The radius of a row for neighbourhood size k <= 8 is
 * column k - 1 of its list against its own set.  Only values are kept: the result is identical bit for bit whatever the chunking
 * of the bank, the number of splits, B or the launch geometry.
 *   query_base >= 0 turns self-exclusion on: the pair with query_base + b == index_base + n is skipped (by index, not by value: a
 *   duplicate row elsewhere counts, at distance 0); query_base = -1 turns it off (two different sets).  index_base >= 0.
 *   splits: the chunk is cut into that many slices, one workgroup per (slice, 128 queries); 0 picks a count that fills the chip.
 *   workspace holds the slices' partial lists: vtp_pr_workspace_bytes(B, splits) = splits * B * 32 bytes (for splits = 0: enough
 *   for whatever the heuristic picks at this B), 16-byte aligned; contents need not be kept between calls.
 *   d2_out (may be NULL): f32 [B, N], row stride ldo: the chunk's distances (the excluded pair included), for tests.
 *   Limits: D a positive multiple of 8, ldq and ldx multiples of 4 and >= D, Q and X 16-byte aligned; 0 <= splits <= 1024.
 * vtp_pr_workspace_bytes returns the bytes, or -1 (bad argument, or more than 2 GiB: pass fewer queries per call).
 *
 * vtp_pr_cover: hits int32 [B]: hits[b] += the number of rows n of the chunk with d2(q_b, x_n) <= r2[n] (r2 f32 [N]: the squared
 * radii of the bank rows).  One integer atomic per query and workgroup: exact and order-free.  Limits as vtp_pr_knn_dist. */
int vtp_pr_workspace_bytes(int B, int splits);
int vtp_pr_sqnorm(const float* X, int ldx, int N, int D, float* out, void* stream);
int vtp_pr_knn_dist(const float* Q, int ldq, const float* qn, const float* X, int ldx, const float* xn, long query_base,
                    long index_base, int B, int N, int D, float* dist, void* workspace, long workspace_bytes, int splits,
                    float* d2_out, int ldo, void* stream);
int vtp_pr_cover(const float* Q, int ldq, const float* qn, const float* X, int ldx, const float* xn, const float* r2, int B, int N,
                 int D, int* hits, int splits, void* stream);

/* ---- Cross-modal retrieval on the CLIP heads (retrieval.hip): image -> text and text -> image recall@K on a captioned set, the
 * evaluation the CLIP paper reports on Flickr30k and MSCOCO-5k, restated from the papers' description; neither CLIP_benchmark nor
 * OpenCLIP is a reference of this project, so parity with those programs is unpinned.  Everything in exact fp32, integer atomics
 * only, no host synchronisation.
 *   s(i, j) = the fmaf chain over k = 0 .. D-1 ascending, the bits of element [i, j] of vtp_gemm_nt_f32(Q, X) with the plain
 *   epilogue (no split of k).  Gallery rows are ordered by (similarity descending, gallery index ascending), a total order.
 *   (s*, j*) = the first ground-truth row of a query under that order; rank = #{j : s(i, j) > s*} + #{j < j* : s(i, j) == s*}.  No
 *   ground-truth row is ever counted.  A query without ground truth has (s*, j*) = (-inf, -1) and rank = the gallery size: a miss
 *   at every K and still a row.  Inputs are finite by contract; a NaN similarity never beats anything and is never chosen as s*.
 *
 * vtp_retr_best: per query of Q f32 [B, D] (row stride ldq) the best of its ground-truth rows in the WHOLE gallery X f32
 * [n_total, D] (row stride ldx): best_s f32 [B], best_j int64 [B].  The lists are a CSR: gt_ptr int32 [B + 1], ascending, values in
 * [0, nnz], the list of query b being gt_idx[gt_ptr[b] .. gt_ptr[b + 1]); gt_idx int64 [nnz] holds gallery rows in any order; an
 * index outside [0, n_total) is ignored; an empty list gives (-inf, -1).  Among equal similarities the lower row wins.  Work is cut
 * over (query, list entry) pairs.  Limits: D a positive multiple of 8, ldq and ldx multiples of 4 and >= D, Q and X 16-byte
 * aligned, n_total <= 2^31 - 1 (a rank is an int32).
 *
 * vtp_retr_rank: one sweep of the chunk X f32 [N, D] of the gallery, whose row 0 has the global index index_base, over the queries:
 * beats int32 [B] += the number of chunk rows strictly before (best_s[b], best_j[b]) under the order above; best_j[b] == -1 counts
 * every row of the chunk.  beats is in/out: zero it before the first chunk; after the last one it is the rank.  One integer atomic
 * per query and workgroup: the result is identical whatever the chunking of the gallery, the number of splits, B or the grid.
 *   splits: the chunk is cut into that many slices, one workgroup per (slice, 128 queries); 0 picks a count that fills the chip.
 *   sims_out (may be NULL): f32 [B, N], row stride lds: the chunk's similarities, for tests.
 *   Limits (those of vtp_knn_topk): D a positive multiple of 8, ldq and ldx multiples of 4 and >= D, Q and X 16-byte aligned,
 *   0 <= splits <= 1024; index_base + N <= 2^31 - 1.
 *
 * vtp_retr_count: counts int64 [nk + 1]: counts[m] += #{b : beats[b] < ks[m]}, counts[nk] += B.  ks: HOST int[nk], positive and
 * ascending, nk <= 8.  rank (may be NULL): int32, rank[rank_offset + b] = beats[b]: the ranks of a whole evaluation stay on the
 * device. */
int vtp_retr_best(const float* Q, int ldq, const float* X, int ldx, long n_total, const int* gt_ptr, const long* gt_idx, int nnz, int B,
                  int D, float* best_s, long* best_j, void* stream);
int vtp_retr_rank(const float* Q, int ldq, const float* X, int ldx, long index_base, int B, int N, int D, const float* best_s,
                  const long* best_j, int* beats, int splits, float* sims_out, int lds, void* stream);
int vtp_retr_count(const int* beats, int B, const int* ks, int nk, long* counts, int* rank, long rank_offset, void* stream);

/* ---- Inception Score (inception_score.hip): Salimans et al. 2016, the figure the ADM evaluation suite reports beside FID, restated
 * from the papers' definition; neither ADM's evaluator nor its TF graph is a reference of this project, so parity with that program
 * is unpinned.  With p_i = softmax(logits_i) and the rows cut in order into splits of split_size rows:
 *   KL_s = (1 / n_s) sum_i sum_c p_ic (log p_ic - log m_c), m_c = (1 / n_s) sum_i p_ic, IS = mean_s exp(KL_s), accumulated as
 *   H_s = sum_i h_i with h_i = sum_c p_ic (l_ic - lse_i) and S_sc = sum_i p_ic:  KL_s = (H_s - sum_c S_sc log(S_sc / n_s)) / n_s.
 * Everything in fp64, no float atomics, no host synchronisation.
 *
 * vtp_is_rows: logits f32 [B, ldl], of which the columns c < C count (the buffer may be wider: the padded columns of a GEMM) ->
 *   p f64 [B, ldp] (columns c < C written) and h f64 [B].  Per row: m = max_c l_c, j the first column that holds it, d_c = l_c - m
 *   (exact), z = sum_{c != j} exp(d_c), Z = 1 + z, log Z = log1p(z) (a row certain of one class keeps its log Z), p_c = exp(d_c) / Z,
 *   h = sum_c p_c (d_c - log Z) (= sum_c p_c (l_c - lse) with lse = m + log Z; never p log p: a p_c that underflows to 0 contributes
 *   0).  One wave per row, lanes stride over c, lane sums in column order, a fixed butterfly: the bits of a row depend on that row
 *   alone, not on B or on its place in the batch.  Logits are finite by contract.
 * vtp_is_accum: row i of the update (p f64 [B, ldp], h f64 [B]) is global row row_base + i and belongs to slot
 *   (row_base + i) / split_size of state f64 [n_slots, 1 + C], a slot being [H_s | S_s0 .. S_s,C-1].  The thread that owns an
 *   element of a slot adds its rows in ascending order (the scheme of vtp_fid_accum): any split of the same rows over updates
 *   leaves the same bits, an update that straddles a split boundary included.  The row counts n_s are the caller's to keep.
 *   split_size >= 1 (LONG_MAX: one split), row_base >= 0, the last row's slot < n_slots, at most 65535 slots per update. */
int vtp_is_rows(const float* logits, int ldl, int B, int C, double* p, int ldp, double* h, void* stream);
int vtp_is_accum(const double* p, int ldp, const double* h, long row_base, long split_size, int B, int C, double* state, int n_slots,
                 void* stream);

/* ---- Kernel Inception Distance (mmd.hip): the pair sums of the unbiased MMD^2 of two feature sets under the polynomial kernel
 * k(x, y) = (gamma x.y + coef0)^degree (Binkowski et al. 2018), restated from the paper's definition; neither torch-fidelity nor the
 * authors' TF code is a reference of this project, so parity with those programs is unpinned.  No atomics, no host synchronisation.
 *   s(a, b) = the fmaf chain over k = 0 .. D-1 ascending, the bits of vtp_gemm_nt_f32 with the plain epilogue; then in fp64, every
 *   operation rounded on its own: t = (double)s * gamma + coef0, k = t multiplied by t a further degree - 1 times, left to right.
 *
 * vtp_mmd_poly_part: part f64 [P, tiles, B], tiles = ceil(N / 128): part[p][t][b] = the sum of k(q_b, x_n) over the rows n of tile t
 * of problem p's bank.  Q f32 [., D] (row stride ldq) holds the queries, X f32 [., D] (row stride ldx) the bank rows.
 *   qi / xi (may be NULL: identity, Q is [B, D] / X is [N, D]): DEVICE int32 [P, B] / [P, N]: query b of problem p is row qi[p][b] of
 *   Q [q_rows, D], bank row n is row xi[p][n] of X [x_rows, D]; an index outside its matrix is read as a row of zeros.  q_rows /
 *   x_rows are read only with a list.
 *   Left out (skipped, not added as zero): the pair with query_base + b == index_base + n when query_base >= 0 (positions in the
 *   lists, not gathered rows; query_base = -1: nothing is excluded), rows past N, queries past B.
 *   kparams: HOST double[2] = {gamma, coef0}, read before the launch.  degree: 1 .. 8.
 *   The order of every sum is fixed (written once in mmd.hip) and depends on a row's position in its tile alone; index_base must be
 *   a multiple of 128, so a tile covers the same absolute rows whatever the chunking of the bank.
 *   Limits: D a positive multiple of 8, ldq and ldx multiples of 4 and >= D, Q and X 16-byte aligned, B <= 65535 * 128, P <= 65535,
 *   part_bytes >= vtp_mmd_workspace_bytes(B, N, P) = P * tiles * B * 8.
 * vtp_mmd_workspace_bytes returns the bytes of part, or -1 (bad argument, or more than 2 GiB: pass fewer rows per call).
 * vtp_mmd_fold: rowsum f64 [P, B] (in/out: zero it before the first chunk; chunks in ascending order): rowsum[p][b] += part[p][t][b]
 *   for t = 0 .. tiles - 1 ascending, one owner thread per element.
 * vtp_mmd_total: total f64 [P]: total[p] = the sum of rowsum[p][0 .. B) by the tree that pairs neighbours level by level (an odd last
 *   element moves up unchanged): its shape depends on B alone.  B <= 2097152.
 * Row sums and totals repeat bit for bit whatever the chunk size, the queries per call or the card. */
int vtp_mmd_workspace_bytes(int B, int N, int P);
int vtp_mmd_poly_part(const float* Q, int ldq, int q_rows, const int* qi, const float* X, int ldx, int x_rows, const int* xi,
                      long query_base, long index_base, int B, int N, int D, int P, const double* kparams, int degree, double* part,
                      long part_bytes, void* stream);
int vtp_mmd_fold(const double* part, double* rowsum, int B, int tiles, int P, void* stream);
int vtp_mmd_total(const double* rowsum, int B, int P, double* total, void* stream);

#ifdef __cplusplus
}
#endif
#endif
