// Linear segmentation probe (the DINOv2 / iBOT dense evaluation protocol, restated from the papers): a linear layer on frozen patch
// tokens, its low-resolution logit map upsampled bilinearly to the label map, per-pixel cross-entropy, mIoU.  The low-resolution
// logits Z[M = B h w, H C] come from vtp_probe_logits; nothing of size [B, C, Hl, Wl] is ever stored:
//   vtp_seg_ce      : per pixel and head the interpolated logits from LDS-staged cells -> lse, argmax, loss partials, confusion counts
//   vtp_seg_dlogits : G = d loss / d Z as a GATHER: one wave per (cell, head, 64 classes) walks the pixels of the cell's support
//   vtp_seg_sgd     : dW = G^T X on the f32-input MFMA in fixed slices of the token rows, folded in slice order into the SGD step
// ATen's upsample_bilinear2d (align_corners=False, no antialias) per axis is seg_tap (seg_bilinear.h, shared with depthprobe.hip); every
// kernel takes the taps and weights of a pixel from that one function, and the blend from seg_blend, so the forward and the gradient
// agree on every pixel.  The weight step's launcher, seg_sgd_launch, also serves vtp_depth_sgd: its two kernels exist once, here.
// No float atomics anywhere: every float has one writer and one summation order; the confusion counts are integer atomics.
#include "common.h"
#include "seg_bilinear.h"
#include "vtp_hip.h"
#include "wave_f32.h"

namespace vtp {

constexpr int SEG_HASH = 2048;   // slots of the workgroup's (target, prediction) table: twice the pixels of the largest tile
constexpr int SEG_SLICE = 512;   // token rows per weight-gradient slice: a constant, never derived from the device

__device__ __forceinline__ bool seg_valid(int lab, int C, int ignore) { return lab != ignore && lab < C; }

// ---------------------------------------------------------------------------------------------------------------- pixel pass
// (the tiling of the label map, seg_plan, and a tile's geometry and cells, SegTile, are seg_bilinear.h's)
// grid (tiles, B).  part_loss f32 [H, nblocks] and part_cnt i32 [2, nblocks] (valid, out of range) get one entry per workgroup;
// seg_ce_fold_kernel adds them in workgroup order.
__global__ __launch_bounds__(SEG_THREADS) void seg_ce_kernel(const float* __restrict__ Z, int ldz, const uint8_t* __restrict__ labels,
                                                            int h, int w, int Hl, int Wl, int H, int C, int ignore, int th, int tw,
                                                            int tiles_x, float* __restrict__ lse, unsigned long long* __restrict__ conf,
                                                            float* __restrict__ part_loss, int* __restrict__ part_cnt) {
  __shared__ float cells[SEG_CELL_FLOATS];
  __shared__ int hkey[SEG_HASH], hcnt[SEG_HASH];
  __shared__ float red[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, b = blockIdx.y, B = gridDim.y, tile = blockIdx.x;
  const int nblocks = gridDim.x * gridDim.y, blk = b * gridDim.x + tile;
  const SegTile geo(tile, tiles_x, th, tw, h, w, Hl, Wl, C);
  const int y0 = geo.y0, x0 = geo.x0, y1 = geo.y1, x1 = geo.x1, npix = th * tw;
  const long plane = (long)Hl * Wl;
  const uint8_t* lab_b = labels + b * plane;

  int nv = 0, no = 0;
  for (int p = tid; p < npix; p += SEG_THREADS) {
    const int py = y0 + p / tw, px = x0 + p % tw;
    if (py > y1 || px > x1) continue;
    const int lab = lab_b[(long)py * Wl + px];
    if (lab == ignore) continue;
    if (lab < C) ++nv;
    else ++no;
  }
  nv = block_sum_int(nv, redi);
  no = block_sum_int(no, redi);
  if (tid == 0) part_cnt[blk] = nv, part_cnt[nblocks + blk] = no;

  for (int hh = 0; hh < H; ++hh) {
    __syncthreads();
    geo.stage(cells, Z, ldz, b, hh, h, w, C);
    if (conf)
      for (int i = tid; i < SEG_HASH; i += SEG_THREADS) hkey[i] = -1, hcnt[i] = 0;
    __syncthreads();
    float loss = 0.f;
    for (int p = tid; p < npix; p += SEG_THREADS) {
      const int py = y0 + p / tw, px = x0 + p % tw;
      if (py > y1 || px > x1) continue;
      const int lab = lab_b[(long)py * Wl + px];
      const bool ok = seg_valid(lab, C, ignore);
      if (!ok && !lse) continue;
      const SegTap ty = seg_tap(py, h, Hl), tx = seg_tap(px, w, Wl);
      const SegCorners q = geo.corners(cells, ty, tx);
      float m = -INFINITY;
      int mi = 0;
      for (int c = 0; c < C; ++c) {
        const float v = seg_blend(q.c00[c], q.c01[c], q.c10[c], q.c11[c], ty, tx);
        if (v > m) m = v, mi = c;  // strict >: the lowest index of the maximum stays
      }
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += expf(seg_blend(q.c00[c], q.c01[c], q.c10[c], q.c11[c], ty, tx) - m);
      const float l = m + logf(s);
      if (lse) lse[((long)hh * B + b) * plane + (long)py * Wl + px] = l;
      if (!ok) continue;
      loss += l - seg_blend(q.c00[lab], q.c01[lab], q.c10[lab], q.c11[lab], ty, tx);
      if (conf) {  // integer counts in an LDS table first: one global atomic per (target, prediction) pair the tile holds
        const int key = lab * C + mi;
        unsigned slot = ((unsigned)key * 2654435761u) >> 21;
        for (;;) {
          const int prev = atomicCAS(&hkey[slot], -1, key);
          if (prev == -1 || prev == key) break;
          slot = (slot + 1) & (SEG_HASH - 1);  // at most npix <= SEG_HASH / 2 keys: a free slot exists
        }
        atomicAdd(&hcnt[slot], 1);
      }
    }
    loss = block_sum<4>(loss, red);  // fixed order; its barriers also close the table
    if (tid == 0) part_loss[(long)hh * nblocks + blk] = loss;
    if (conf)
      for (int i = tid; i < SEG_HASH; i += SEG_THREADS)
        if (hkey[i] >= 0) atomicAdd(conf + (long)hh * C * C + hkey[i], (unsigned long long)hcnt[i]);
  }
}

// one workgroup; one owner thread per sum, partials added in ascending workgroup order
__global__ __launch_bounds__(SEG_THREADS) void seg_ce_fold_kernel(const float* __restrict__ part_loss, const int* __restrict__ part_cnt,
                                                                 int nblocks, int H, float* __restrict__ loss, int* __restrict__ call_counts,
                                                                 long* __restrict__ totals) {
  __shared__ int cnt[2];
  const int tid = threadIdx.x;
  if (tid < 2) {
    int s = 0;
    for (int i = 0; i < nblocks; ++i) s += part_cnt[(long)tid * nblocks + i];
    cnt[tid] = s;
    call_counts[tid] = s;
    if (totals) totals[tid] += s;
  }
  __syncthreads();
  const int n = cnt[0];
  for (int hh = tid; hh < H; hh += SEG_THREADS) {
    float s = 0.f;
    for (int i = 0; i < nblocks; ++i) s += part_loss[(long)hh * nblocks + i];
    loss[hh] = n > 0 ? s / (float)n : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------- cell pass
// seg_cell_walk (seg_bilinear.h) with one wave per (cell, head, chunk of 64 classes), lane = class: the walk reads only the label and
// lse of each pixel, its term is softmax minus one-hot.
__global__ __launch_bounds__(SEG_THREADS) void seg_dlogits_kernel(const float* __restrict__ Z, int ldz, const uint8_t* __restrict__ labels,
                                                                 const float* __restrict__ lse, const int* __restrict__ call_counts,
                                                                 float* __restrict__ G, int ldg, int B, int h, int w, int Hl, int Wl, int H,
                                                                 int C, int ignore, int chunks, long tasks) {
  const long task = seg_cell_task();
  if (task >= tasks) return;
  const SegCell t(task, h, w, H, C, chunks);
  const int c = t.c;
  const long plane = (long)Hl * Wl;
  const uint8_t* lab_b = labels + t.b * plane;
  const float* lse_b = lse + ((long)t.hh * B + t.b) * plane;
  int lab;
  const float acc = seg_cell_walk(
      t, Z, ldz, h, w, Hl, Wl, C,
      [&](int py, int px) {
        lab = lab_b[(long)py * Wl + px];
        return seg_valid(lab, C, ignore);
      },
      [&](int py, int px, float z) { return expf(z - lse_b[(long)py * Wl + px]) - (lab == c ? 1.f : 0.f); });
  const int nv = call_counts[0];
  const float inv = nv > 0 ? 1.f / (float)nv : 0.f;
  if (c < C) G[t.cell * ldg + (long)t.hh * C + c] = acc * inv;
}

// ---------------------------------------------------------------------------------------------------------------- weight step
// The G^T X tile of wave_f32.h (one wave = 64 rows n x 64 columns k, the tile of probe_sgd_kernel) over ONE slice of SEG_SLICE token
// rows; the partial tile goes to wsW [S, N, K], the partial column sums of G to wsb [S, N].
__global__ __launch_bounds__(SEG_THREADS) void seg_wgrad_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ X, int ldx,
                                                               int M, int N, int K, int k_tiles, int n_tiles, long tasks,
                                                               float* __restrict__ wsW, float* __restrict__ wsb) {
  const int lane = threadIdx.x & 63, r = lane & 31, half = lane >> 5;
  const long task = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (task >= tasks) return;
  const int kt = (int)(task % k_tiles);
  const long t2 = task / k_tiles;
  const int nt = (int)(t2 % n_tiles), s = (int)(t2 / n_tiles);
  const int n0 = nt * 64, k0 = kt * 64, m0 = s * SEG_SLICE, m1 = min(M, m0 + SEG_SLICE);
  const int na = n0 + r, nb = n0 + 32 + r, ka = k0 + r, kb = k0 + 32 + r;
  f32x16 acc[2][2];
  wave_gtx_tile<4>(acc, G + (na < N ? na : N - 1), G + (nb < N ? nb : N - 1), ldg, X + (ka < K ? ka : K - 1), X + (kb < K ? kb : K - 1), ldx,
                na >= N, nb >= N, ka >= K, kb >= K, m0, m1, half);
  float* out = wsW + (long)s * N * K;
  wave_gtx_visit(
      acc, n0, k0, N, K, r, half, [&](int n) { return out + (long)n * K; }, [](int, int k, float d, float* out_row) { out_row[k] = d; });
  if (k0 == 0) {
    const int n = n0 + lane;
    if (n < N) wsb[(long)s * N + n] = wave_gtx_colsum(G + n, ldg, m0, m1);
  }
}

// one owner per four weights (or one bias): the S partials added in slice order, then vtp_probe_sgd's step (sgd_momentum_step)
__global__ __launch_bounds__(SEG_THREADS) void seg_sgd_fold_kernel(float* __restrict__ W, float* __restrict__ bias, float* __restrict__ mW,
                                                                  float* __restrict__ mb, const float* __restrict__ wsW,
                                                                  const float* __restrict__ wsb, const float* __restrict__ lr, int S, int N,
                                                                  int C, int K, float momentum) {
  const long nk4 = (long)N * K / 4, i = (long)blockIdx.x * SEG_THREADS + threadIdx.x;
  if (i < nk4) {
    const f32x4* p = (const f32x4*)wsW + i;
    f32x4 d = p[0];
    for (int s = 1; s < S; ++s) d += p[(long)s * nk4];
    const float nlr = -lr[(int)(i * 4 / K) / C];  // K % 4 == 0: the four weights share a row
    f32x4 m = ((f32x4*)mW)[i], x = ((f32x4*)W)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float we = x[e], me = m[e];
      sgd_momentum_step(we, me, d[e], momentum, nlr);
      x[e] = we, m[e] = me;
    }
    ((f32x4*)mW)[i] = m;
    ((f32x4*)W)[i] = x;
  } else if (i - nk4 < N) {
    const int n = (int)(i - nk4);
    float d = wsb[n];
    for (int s = 1; s < S; ++s) d += wsb[(long)s * N + n];
    float w = bias[n], m = mb[n];
    sgd_momentum_step(w, m, d, momentum, -lr[n / C]);
    mb[n] = m;
    bias[n] = w;
  }
}

static long seg_ce_bytes(const SegPlan& p, int B, int H) { return ((long)H + 2) * p.tiles_y * p.tiles_x * B * 4; }
static long seg_sgd_bytes(int M, int N, int K) { return (long)cdiv(M, SEG_SLICE) * N * ((long)K + 1) * 4; }

int seg_sgd_workspace(const char* who, int M, int N, int K) {
  VTP_REQUIRE(M >= 1 && N >= 1 && K >= 4 && K % 4 == 0, "%s: bad shape (M, N >= 1, K %% 4 == 0)", who);
  const long n = seg_sgd_bytes(M, N, K);
  VTP_REQUIRE(n <= INT_MAX, "%s: more than 2 GiB (pass fewer heads per call)", who);
  return (int)n;
}

int seg_sgd_launch(const char* who, float* W, float* bias, float* mW, float* mb, const float* G, int ldg, const float* X, int ldx,
                   const float* lr, int M, int H, int C, int K, float momentum, void* workspace, long workspace_bytes, void* stream) {
  VTP_REQUIRE(W && bias && mW && mb && G && X && lr && workspace, "%s: null pointer", who);
  VTP_REQUIRE(M >= 1 && H >= 1 && C >= 1 && (long)H * C <= INT_MAX && K >= 4 && K % 4 == 0, "%s: bad shape (M, H, C >= 1, K %% 4 == 0)", who);
  VTP_REQUIRE(ldx >= K && ldx % 4 == 0 && ldg >= (long)H * C, "%s: bad leading dimension (ldx >= K, ldx %% 4 == 0, ldg >= H * C)", who);
  VTP_REQUIRE(aligned16(X) && aligned16(W) && aligned16(mW) && aligned16(workspace),
              "%s: X, W, mW and workspace must be 16-byte aligned", who);
  const int N = H * C, S = cdiv(M, SEG_SLICE);
  VTP_REQUIRE(workspace_bytes >= seg_sgd_bytes(M, N, K), "%s: workspace too small (%s_workspace_bytes)", who, who);
  const int k_tiles = cdiv(K, 64), n_tiles = cdiv(N, 64);
  const long tasks = (long)k_tiles * n_tiles * S, nk4 = (long)N * K / 4;
  VTP_REQUIRE((tasks + 3) / 4 <= INT_MAX && (nk4 + N) / SEG_THREADS < INT_MAX, "%s: too many tiles", who);
  float* wsW = (float*)workspace;
  float* wsb = wsW + (long)S * N * K;
  hipLaunchKernelGGL(seg_wgrad_kernel, dim3(cdiv(tasks, 4)), dim3(SEG_THREADS), 0, (hipStream_t)stream, G, ldg, X, ldx, M, N, K, k_tiles,
                     n_tiles, tasks, wsW, wsb);
  hipLaunchKernelGGL(seg_sgd_fold_kernel, dim3(cdiv(nk4 + N, SEG_THREADS)), dim3(SEG_THREADS), 0, (hipStream_t)stream, W, bias, mW, mb, wsW,
                     wsb, lr, S, N, C, K, momentum);
  return check_launch(who + 4);  // without the "vtp_"
}

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_seg_ce_workspace_bytes(int B, int h, int w, int Hl, int Wl, int H, int C) {
  if (seg_check("vtp_seg_ce_workspace_bytes", B, h, w, Hl, Wl, H, C, 1, 255, 0, nullptr, 0, nullptr, nullptr)) return VTP_ERR_ARG;
  const long n = seg_ce_bytes(seg_plan(h, w, Hl, Wl, C), B, H);
  VTP_REQUIRE(n <= INT_MAX, "vtp_seg_ce_workspace_bytes: more than 2 GiB (pass fewer heads per call)");
  return (int)n;
}

extern "C" int vtp_seg_ce(const float* Z, int ldz, const unsigned char* labels, int B, int h, int w, int Hl, int Wl, int H, int C,
                          int ignore_index, float* lse, long* conf, float* loss, int* call_counts, long* totals, void* workspace,
                          long workspace_bytes, void* stream) {
  VTP_REQUIRE(Z && labels && loss && call_counts && workspace, "vtp_seg_ce: null pointer");
  SegPlan p;
  if (seg_check("vtp_seg_ce", B, h, w, Hl, Wl, H, C, 1, 255, (long)C * C, "ldz", ldz, &p, nullptr)) return VTP_ERR_ARG;
  const long tiles = (long)p.tiles_y * p.tiles_x, nblocks = tiles * B;
  VTP_REQUIRE(workspace_bytes >= seg_ce_bytes(p, B, H) && ((uintptr_t)workspace & 3) == 0,
              "vtp_seg_ce: workspace too small (vtp_seg_ce_workspace_bytes) or not 4-byte aligned");
  float* part_loss = (float*)workspace;
  int* part_cnt = (int*)(part_loss + (long)H * nblocks);
  hipLaunchKernelGGL(seg_ce_kernel, dim3((unsigned)tiles, B), dim3(SEG_THREADS), 0, (hipStream_t)stream, Z, ldz, labels, h, w, Hl, Wl, H,
                     C, ignore_index, p.th, p.tw, p.tiles_x, lse, (unsigned long long*)conf, part_loss, part_cnt);
  hipLaunchKernelGGL(seg_ce_fold_kernel, dim3(1), dim3(SEG_THREADS), 0, (hipStream_t)stream, part_loss, part_cnt, (int)nblocks, H, loss,
                     call_counts, totals);
  return check_launch("seg_ce");
}

extern "C" int vtp_seg_dlogits(const float* Z, int ldz, const unsigned char* labels, const float* lse, const int* call_counts, float* G,
                               int ldg, int B, int h, int w, int Hl, int Wl, int H, int C, int ignore_index, void* stream) {
  VTP_REQUIRE(Z && labels && lse && call_counts && G, "vtp_seg_dlogits: null pointer");
  long tasks;
  if (seg_check("vtp_seg_dlogits", B, h, w, Hl, Wl, H, C, 1, 255, C, "ldz, ldg", min(ldz, ldg), nullptr, &tasks)) return VTP_ERR_ARG;
  const int chunks = cdiv(C, 64);
  hipLaunchKernelGGL(seg_dlogits_kernel, dim3(cdiv(tasks, 4)), dim3(SEG_THREADS), 0, (hipStream_t)stream, Z, ldz, labels, lse, call_counts,
                     G, ldg, B, h, w, Hl, Wl, H, C, ignore_index, chunks, tasks);
  return check_launch("seg_dlogits");
}

extern "C" int vtp_seg_sgd_slice(void) { return SEG_SLICE; }

extern "C" int vtp_seg_sgd_workspace_bytes(int M, int N, int K) {
  return seg_sgd_workspace("vtp_seg_sgd_workspace_bytes", M, N, K);
}

extern "C" int vtp_seg_sgd(float* W, float* bias, float* mW, float* mb, const float* G, int ldg, const float* X, int ldx, const float* lr,
                           int M, int H, int C, int K, float momentum, void* workspace, long workspace_bytes, void* stream) {
  VTP_REQUIRE(W && bias && mW && mb && G && X && lr && workspace, "vtp_seg_sgd: null pointer");
  VTP_REQUIRE(C >= 1 && C <= 255, "vtp_seg_sgd: bad shape (1 <= C <= 255)");
  return seg_sgd_launch("vtp_seg_sgd", W, bias, mW, mb, G, ldg, X, ldx, lr, M, H, C, K, momentum, workspace, workspace_bytes, stream);
}
