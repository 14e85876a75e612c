// Linear monocular-depth probe (the DINOv2 "lin." depth protocol, restated from the papers): a linear layer on frozen patch tokens
// whose C outputs are bins of depth, its low-resolution logit map upsampled bilinearly to the label map, the AdaBins "linear
// normalisation" a_c = max(z_c, 0) + 0.1, dhat = sum_c a_c e_c / sum_c a_c over uniform bin centres, the scale-invariant log loss of
// Eigen et al.  The low-resolution logits Z[M = B h w, H C] come from vtp_probe_logits; nothing of size [B, C, Hl, Wl] is stored:
//   vtp_depth_pix     : per pixel and head the interpolated logits from LDS-staged cells -> dhat, g = log dhat - log gt, fp64 partials
//                       of g and g^2 per workgroup, folded in workgroup order into n, m1, m2, L; the evaluation sums per image
//   vtp_depth_dlogits : G = d L / d Z as a GATHER shaped like vtp_seg_dlogits: one wave per (cell, head, 64 bins)
//   vtp_depth_sgd     : vtp_seg_sgd's two kernels through seg_sgd_launch (seg_bilinear.h), for up to 1024 bins
// The taps, the blend and the tiling are seg_bilinear.h's, the bin centres depth_bin's: forward and gradient agree on every pixel.
// No float atomics and no integer ones either: every number has one writer and one summation order.
#include "common.h"
#include "seg_bilinear.h"
#include "vtp_hip.h"

namespace vtp {

constexpr int DEPTH_MAX_BINS = 1024;
constexpr int DEPTH_SUMS = 6;  // fp64 partials per workgroup and head: g, g^2, |d - gt| / gt, (d - gt)^2 / gt, (d - gt)^2, |g| / ln 10
constexpr int DEPTH_CNTS = 3;  // i32 partials per workgroup and head: max(d / gt, gt / d) < 1.25, 1.25^2, 1.25^3
constexpr int DEPTH_AUX = 3;   // f32 planes [H, B, Hl, Wl] of the cell pass: dhat, g, 1 / (dhat S) (0 marks an invalid pixel)

// centre of bin c of C uniform bins over [lo, hi]: 4 roundings, the same in every kernel
__device__ __forceinline__ float depth_bin(int c, int C, float lo, float hi) {
#pragma clang fp contract(off)
  return lo + ((hi - lo) * (float)c) / (float)(C - 1);
}

__device__ __forceinline__ bool depth_valid(float gt, float hi) { return gt > 0.f && gt <= hi; }  // false for NaN and inf

// fixed order: the xor tree of a wave, then the four waves ascending
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------------------------- pixel pass
// grid (tiles, B), workgroup blk = b * tiles + tile.  part_sum f64 [H, DEPTH_SUMS, nblocks], part_cnt i32 [H, DEPTH_CNTS, nblocks] and
// part_n i32 [nblocks] get one entry per workgroup; without `eval` only the first two sums are written (and read by the fold).
__global__ __launch_bounds__(SEG_THREADS) void depth_pix_kernel(const float* __restrict__ Z, int ldz, const float* __restrict__ gt, int h,
                                                               int w, int Hl, int Wl, int H, int C, float lo, float hi, int th, int tw,
                                                               int tiles_x, float* __restrict__ dhat, float* __restrict__ aux, int eval,
                                                               double* __restrict__ part_sum, int* __restrict__ part_cnt,
                                                               int* __restrict__ part_n) {
  __shared__ float cells[SEG_CELL_FLOATS];
  __shared__ float bins[DEPTH_MAX_BINS];
  __shared__ double redd[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, b = blockIdx.y, B = gridDim.y, tile = blockIdx.x;
  const long nblocks = (long)gridDim.x * gridDim.y, blk = (long)b * gridDim.x + tile;
  const SegTile geo(tile, tiles_x, th, tw, h, w, Hl, Wl, C);
  const int y0 = geo.y0, x0 = geo.x0, y1 = geo.y1, x1 = geo.x1, npix = th * tw;
  const long plane = (long)Hl * Wl;
  const float* gt_b = gt ? gt + b * plane : nullptr;
  const double inv_ln10 = 0.43429448190325182765;

  for (int c = tid; c < C; c += SEG_THREADS) bins[c] = depth_bin(c, C, lo, hi);
  if (gt_b) {
    int nv = 0;
    for (int p = tid; p < npix; p += SEG_THREADS) {
      const int py = y0 + p / tw, px = x0 + p % tw;
      if (py > y1 || px > x1) continue;
      nv += depth_valid(gt_b[(long)py * Wl + px], hi) ? 1 : 0;
    }
    nv = block_sum_int(nv, redi);
    if (tid == 0) part_n[blk] = nv;
  }

  for (int hh = 0; hh < H; ++hh) {
    __syncthreads();
    geo.stage(cells, Z, ldz, b, hh, h, w, C);
    __syncthreads();
    double s[DEPTH_SUMS] = {0., 0., 0., 0., 0., 0.};
    int k[DEPTH_CNTS] = {0, 0, 0};
    for (int p = tid; p < npix; p += SEG_THREADS) {
      const int py = y0 + p / tw, px = x0 + p % tw;
      if (py > y1 || px > x1) continue;
      const long at = ((long)hh * B + b) * plane + (long)py * Wl + px;
      const float t = gt_b ? gt_b[(long)py * Wl + px] : 0.f;
      const bool ok = gt_b && depth_valid(t, hi);
      if (!ok && aux)
#pragma unroll
        for (int a = 0; a < DEPTH_AUX; ++a) aux[(long)a * H * B * plane + at] = 0.f;
      if (!ok && !dhat) continue;
      const SegTap ty = seg_tap(py, h, Hl), tx = seg_tap(px, w, Wl);
      const SegCorners q = geo.corners(cells, ty, tx);
      float S = 0.f, T = 0.f;
      for (int c = 0; c < C; ++c) {
        const float v = seg_blend(q.c00[c], q.c01[c], q.c10[c], q.c11[c], ty, tx);
        const float a = (v > 0.f ? v : 0.f) + 0.1f;
        S += a;
        T = fmaf(a, bins[c], T);
      }
      const float d = T / S;
      if (dhat) dhat[at] = d;
      if (!ok) continue;
      const float g = logf(d) - logf(t);
      s[0] += (double)g;
      s[1] += (double)g * (double)g;
      if (aux) {
        aux[at] = d;
        aux[(long)H * B * plane + at] = g;
        aux[2L * H * B * plane + at] = 1.f / (d * S);
      }
      if (eval) {
        const double dd = (double)d, tt = (double)t, diff = dd - tt, ratio = fmax(dd / tt, tt / dd);
        s[2] += fabs(diff) / tt;
        s[3] += diff * diff / tt;
        s[4] += diff * diff;
        s[5] += fabs((double)g) * inv_ln10;
        k[0] += ratio < 1.25 ? 1 : 0;
        k[1] += ratio < 1.5625 ? 1 : 0;
        k[2] += ratio < 1.953125 ? 1 : 0;
      }
    }
    if (!gt_b) continue;
    const int nsum = eval ? DEPTH_SUMS : 2;
    for (int q = 0; q < nsum; ++q) {
      const double v = block_sum_f64(s[q], redd);
      if (tid == 0) part_sum[((long)hh * DEPTH_SUMS + q) * nblocks + blk] = v;
    }
    if (eval)
      for (int q = 0; q < DEPTH_CNTS; ++q) {
        const int v = block_sum_int(k[q], redi);
        if (tid == 0) part_cnt[((long)hh * DEPTH_CNTS + q) * nblocks + blk] = v;
      }
  }
}

// One workgroup, one owner thread per number.  Per head: n, sum g and sum g^2 over the workgroups in ascending order -> stats (n, m1,
// m2, L) and loss.  The evaluation sums: per image the partials of its tiles in tile order, then the images added to the running
// accumulators in batch order, so any split of an image sequence into batches leaves the same bits.
__global__ __launch_bounds__(SEG_THREADS) void depth_fold_kernel(const double* __restrict__ part_sum, const int* __restrict__ part_cnt,
                                                                const int* __restrict__ part_n, int tiles, int B, int H, float lam,
                                                                float* __restrict__ loss, double* __restrict__ stats,
                                                                long* __restrict__ ecnt, double* __restrict__ esum) {
  const long nblocks = (long)tiles * B;
  const int ntask = H + (ecnt ? H * (DEPTH_SUMS + 1 + DEPTH_CNTS) : 0);
  for (int t = threadIdx.x; t < ntask; t += SEG_THREADS) {
    if (t < H) {
      const double* p = part_sum + (long)t * DEPTH_SUMS * nblocks;
      long n = 0;
      double s1 = 0., s2 = 0.;
      for (long i = 0; i < nblocks; ++i) n += part_n[i], s1 += p[i], s2 += p[nblocks + i];
      const double m1 = n > 0 ? s1 / (double)n : 0., m2 = n > 0 ? s2 / (double)n : 0.;
      const double L = sqrt(fmax(m2 - (double)lam * m1 * m1, 0.));
      stats[4 * t] = (double)n, stats[4 * t + 1] = m1, stats[4 * t + 2] = m2, stats[4 * t + 3] = L;
      loss[t] = (float)L;
      continue;
    }
    const int e = t - H, hh = e / (DEPTH_SUMS + 1 + DEPTH_CNTS), q = e % (DEPTH_SUMS + 1 + DEPTH_CNTS);
    if (q < DEPTH_SUMS) {
      const double* p = part_sum + ((long)hh * DEPTH_SUMS + q) * nblocks;
      double acc = esum[hh * DEPTH_SUMS + q];
      for (int b = 0; b < B; ++b) {
        double img = 0.;
        for (int i = 0; i < tiles; ++i) img += p[(long)b * tiles + i];
        acc += img;
      }
      esum[hh * DEPTH_SUMS + q] = acc;
    } else {
      const int* p = q == DEPTH_SUMS ? part_n : part_cnt + ((long)hh * DEPTH_CNTS + (q - DEPTH_SUMS - 1)) * nblocks;
      long n = 0;
      for (long i = 0; i < nblocks; ++i) n += p[i];
      ecnt[hh * (1 + DEPTH_CNTS) + (q - DEPTH_SUMS)] += n;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- cell pass
// seg_cell_walk (seg_bilinear.h) with one wave per (cell, head, chunk of 64 bins), lane = bin: the walk reads only the three aux
// numbers of each pixel.
//   q_p = ((g_p - fl(lam m1)) * r_p) * fl(1 / (n L)),  G += (wy wx) * [z_p[c] > 0] * (q_p * (e_c - dhat_p))
__global__ __launch_bounds__(SEG_THREADS) void depth_dlogits_kernel(const float* __restrict__ Z, int ldz, const float* __restrict__ aux,
                                                                   const double* __restrict__ stats, float* __restrict__ G, int ldg, int B,
                                                                   int h, int w, int Hl, int Wl, int H, int C, float lo, float hi, float lam,
                                                                   int chunks, long tasks) {
  const long task = seg_cell_task();
  if (task >= tasks) return;
  const SegCell t(task, h, w, H, C, chunks);
  const int c = t.c, hh = t.hh;
  const double n = stats[4 * hh], m1 = stats[4 * hh + 1], L = stats[4 * hh + 3];
  if (!(n > 0. && L > 0.)) {  // wave-uniform
    if (c < C) G[t.cell * ldg + (long)hh * C + c] = 0.f;
    return;
  }
  const float lm1 = (float)((double)lam * m1), inv_nl = (float)(1. / (n * L));
  const float e = depth_bin(t.cl, C, lo, hi);
  const long plane = (long)Hl * Wl, planes = (long)H * B * plane;
  const float* aux_d = aux + ((long)hh * B + t.b) * plane;
  const float* aux_g = aux_d + planes;
  const float* aux_r = aux_g + planes;
  float r;
  const float acc = seg_cell_walk(
      t, Z, ldz, h, w, Hl, Wl, C,
      [&](int py, int px) {
        r = aux_r[(long)py * Wl + px];
        return r != 0.f;  // 0 marks an invalid pixel
      },
      [&](int py, int px, float z) {
        const float q = ((aux_g[(long)py * Wl + px] - lm1) * r) * inv_nl;
        const float d = q * (e - aux_d[(long)py * Wl + px]);
        return z > 0.f ? d : 0.f;
      });
  if (c < C) G[t.cell * ldg + (long)hh * C + c] = acc;
}

static long depth_pix_bytes(const SegPlan& p, int B, int H) {
  return (long)p.tiles_y * p.tiles_x * B * ((long)H * (DEPTH_SUMS * 8 + DEPTH_CNTS * 4) + 4);
}

static bool depth_range_ok(float lo, float hi) { return lo > 0.f && lo < hi && hi < INFINITY; }

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_depth_pix_workspace_bytes(int B, int h, int w, int Hl, int Wl, int H, int C, int aux_plane) {
  if (seg_check("vtp_depth_pix_workspace_bytes", B, h, w, Hl, Wl, H, C, 2, DEPTH_MAX_BINS, 0, nullptr, 0, nullptr, nullptr))
    return VTP_ERR_ARG;
  const long n = aux_plane ? (long)DEPTH_AUX * H * B * Hl * Wl * 4 : depth_pix_bytes(seg_plan(h, w, Hl, Wl, C), B, H);
  VTP_REQUIRE(n <= INT_MAX, "vtp_depth_pix_workspace_bytes: more than 2 GiB (pass fewer heads per call)");
  return (int)n;
}

extern "C" int vtp_depth_pix(const float* Z, int ldz, const float* gt, int B, int h, int w, int Hl, int Wl, int H, int C, float min_depth,
                             float max_depth, float lam, float* dhat, float* aux, float* loss, double* stats, long* eval_counts,
                             double* eval_sums, void* workspace, long workspace_bytes, void* stream) {
  VTP_REQUIRE(Z && (dhat || gt), "vtp_depth_pix: null pointer (Z; dhat or gt)");
  VTP_REQUIRE(!gt || (loss && stats && workspace), "vtp_depth_pix: null pointer (labels need loss, stats and a workspace)");
  VTP_REQUIRE(gt || (!aux && !eval_counts && !eval_sums), "vtp_depth_pix: aux and the evaluation counters need labels");
  VTP_REQUIRE(!eval_counts == !eval_sums, "vtp_depth_pix: eval_counts and eval_sums go together");
  SegPlan p;
  if (seg_check("vtp_depth_pix", B, h, w, Hl, Wl, H, C, 2, DEPTH_MAX_BINS, C, "ldz", ldz, &p, nullptr)) return VTP_ERR_ARG;
  VTP_REQUIRE(depth_range_ok(min_depth, max_depth), "vtp_depth_pix: bad depth range (0 < min_depth < max_depth)");
  const long tiles = (long)p.tiles_y * p.tiles_x, nblocks = tiles * B;
  VTP_REQUIRE(!gt || (workspace_bytes >= depth_pix_bytes(p, B, H) && ((uintptr_t)workspace & 7) == 0),
              "vtp_depth_pix: workspace too small (vtp_depth_pix_workspace_bytes) or not 8-byte aligned");
  double* part_sum = (double*)workspace;
  int* part_cnt = (int*)(part_sum + (long)H * DEPTH_SUMS * nblocks);
  int* part_n = part_cnt + (long)H * DEPTH_CNTS * nblocks;
  hipLaunchKernelGGL(depth_pix_kernel, dim3((unsigned)tiles, B), dim3(SEG_THREADS), 0, (hipStream_t)stream, Z, ldz, gt, h, w, Hl, Wl, H, C,
                     min_depth, max_depth, p.th, p.tw, p.tiles_x, dhat, aux, eval_counts ? 1 : 0, part_sum, part_cnt, part_n);
  if (gt)
    hipLaunchKernelGGL(depth_fold_kernel, dim3(1), dim3(SEG_THREADS), 0, (hipStream_t)stream, part_sum, part_cnt, part_n, (int)tiles, B, H,
                       lam, loss, stats, eval_counts, eval_sums);
  return check_launch("depth_pix");
}

extern "C" int vtp_depth_dlogits(const float* Z, int ldz, const float* aux, const double* stats, float* G, int ldg, int B, int h, int w,
                                 int Hl, int Wl, int H, int C, float min_depth, float max_depth, float lam, void* stream) {
  VTP_REQUIRE(Z && aux && stats && G, "vtp_depth_dlogits: null pointer");
  long tasks;
  if (seg_check("vtp_depth_dlogits", B, h, w, Hl, Wl, H, C, 2, DEPTH_MAX_BINS, C, "ldz, ldg", min(ldz, ldg), nullptr, &tasks))
    return VTP_ERR_ARG;
  VTP_REQUIRE(depth_range_ok(min_depth, max_depth), "vtp_depth_dlogits: bad depth range (0 < min_depth < max_depth)");
  const int chunks = cdiv(C, 64);
  hipLaunchKernelGGL(depth_dlogits_kernel, dim3(cdiv(tasks, 4)), dim3(SEG_THREADS), 0, (hipStream_t)stream, Z, ldz, aux, stats, G, ldg, B, h,
                     w, Hl, Wl, H, C, min_depth, max_depth, lam, chunks, tasks);
  return check_launch("depth_dlogits");
}

extern "C" int vtp_depth_sgd_workspace_bytes(int M, int N, int K) { return seg_sgd_workspace("vtp_depth_sgd_workspace_bytes", M, N, K); }

extern "C" int vtp_depth_sgd(float* W, float* bias, float* mW, float* mb, const float* G, int ldg, const float* X, int ldx, const float* lr,
                             int M, int H, int C, int K, float momentum, void* workspace, long workspace_bytes, void* stream) {
  VTP_REQUIRE(C >= 1 && C <= DEPTH_MAX_BINS, "vtp_depth_sgd: bad shape (1 <= C <= 1024)");
  return seg_sgd_launch("vtp_depth_sgd", W, bias, mW, mb, G, ldg, X, ldx, lr, M, H, C, K, momentum, workspace, workspace_bytes, stream);
}
