// What the dense probes (segprobe.hip, depthprobe.hip) share: ATen's upsample_bilinear2d (align_corners=False, no antialias) per
// axis as seg_tap, the blend of a pixel's four cells as seg_blend, the tiling of the label map whose cell footprint fits the LDS
// budget, the shape limits, and the launcher of the sliced weight step (its two kernels live in segprobe.hip, once).
#pragma once
#include "common.h"

#include <limits.h>

namespace vtp {

constexpr int SEG_THREADS = 256;
constexpr int SEG_CELL_FLOATS = 10240;  // LDS floats for the staged cells of one head (40 KB)
constexpr int SEG_TILE = 32;            // label pixels per tile edge where the footprint allows it
constexpr int SEG_MAX_EDGE = 32768;     // h, w, Hl, Wl: keeps the integer inverse map and B Hl Wl checks simple

struct SegTap {
  int i0, i1;
  float l0, l1;
};

// taps and weights of output index dst on an axis resampled from `in` to `out` entries.  No contraction: the host plans the LDS
// footprint with the same function and has to get the same integers.
__host__ __device__ inline SegTap seg_tap(int dst, int in, int out) {
#pragma clang fp contract(off)
  const float scale = (float)in / (float)out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  SegTap t;
  t.i0 = (int)src;
  if (t.i0 > in - 1) t.i0 = in - 1;  // cannot happen for dst < out; keeps every index inside the map whatever the rounding
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// 7 roundings, the same in every kernel
__device__ __forceinline__ float seg_blend(float v00, float v01, float v10, float v11, const SegTap& ty, const SegTap& tx) {
#pragma clang fp contract(off)
  return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

__device__ __forceinline__ float seg_pick(float a, float b, float c, int k) { return k == 0 ? a : (k == 1 ? b : c); }

// The tiling of the label map: tiles of th x tw pixels whose cell footprint (fy x fx cells of C | 1 floats) fits the LDS budget.
struct SegPlan {
  int th, tw, tiles_y, tiles_x;
};

static inline int seg_footprint(int tile, int in, int out) {
  int worst = 1;
  for (int p0 = 0; p0 < out; p0 += tile) {
    const int p1 = (p0 + tile < out ? p0 + tile : out) - 1;
    const int n = seg_tap(p1, in, out).i1 - seg_tap(p0, in, out).i0 + 1;
    worst = n > worst ? n : worst;
  }
  return worst;
}

static inline SegPlan seg_plan(int h, int w, int Hl, int Wl, int C) {
  SegPlan p;
  p.th = p.tw = SEG_TILE;
  const int Cs = C | 1;
  for (;;) {
    const int fy = seg_footprint(p.th, h, Hl), fx = seg_footprint(p.tw, w, Wl);
    if ((long)fy * fx * Cs <= SEG_CELL_FLOATS || (p.th == 1 && p.tw == 1)) break;  // 1 x 1 pixel: at most 2 x 2 cells of C | 1 floats
    if ((fy >= fx && p.th > 1) || p.tw == 1) p.th /= 2;
    else p.tw /= 2;
  }
  p.tiles_y = cdiv(Hl, p.th);
  p.tiles_x = cdiv(Wl, p.tw);
  return p;
}

static inline bool seg_shape_ok(int B, int h, int w, int Hl, int Wl) {
  return B >= 1 && B <= 65535 && h >= 1 && w >= 1 && h <= SEG_MAX_EDGE && w <= SEG_MAX_EDGE && Hl <= SEG_MAX_EDGE && Wl <= SEG_MAX_EDGE &&
         (long)B * h * w <= INT_MAX && (long)B * Hl * Wl <= INT_MAX;
}

// The sliced weight step behind vtp_seg_sgd and vtp_depth_sgd (segprobe.hip): every argument check but the caller's own bound on C,
// then seg_wgrad_kernel and seg_sgd_fold_kernel.  `who` names the entry point in the messages.
int seg_sgd_workspace(const char* who, int M, int N, int K);
int seg_sgd_launch(const char* who, float* W, float* bias, float* mW, float* mb, const float* G, int ldg, const float* X, int ldx,
                   const float* lr, int M, int H, int C, int K, float momentum, void* workspace, long workspace_bytes, void* stream);

}  // namespace vtp
