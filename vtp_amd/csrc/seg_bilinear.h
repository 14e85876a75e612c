// What the dense probes (segprobe.hip, depthprobe.hip) share: ATen's upsample_bilinear2d (align_corners=False, no antialias) per
// axis as seg_tap, the blend of a pixel's four cells as seg_blend, the tiling of the label map whose cell footprint fits the LDS
// budget, a tile's geometry and cell staging in the pixel passes (SegTile), the gather walk of the cell passes (SegCell,
// seg_cell_walk), the checks the entry points have in common (seg_check), and the launcher of the sliced weight step (its two
// kernels live in segprobe.hip, once).
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

// What the entry points of both probes check alike, under the caller's name and its bounds on C: the label size, the bounds on H and
// C (`per_head` = entries per head of the largest array the call indexes, 0 for none: H * per_head has to fit an int), the map sizes,
// the leading dimensions `ld_names` names (ld_min = the smallest of them; nullptr: the call has none) and the launch size -- of a
// pixel pass when `plan` is given (filled in), of a cell pass when `tasks` is.
static int seg_check(const char* who, int B, int h, int w, int Hl, int Wl, int H, int C, int c_lo, int c_hi, long per_head,
                     const char* ld_names, long ld_min, SegPlan* plan, long* tasks) {
  VTP_REQUIRE(Hl >= 1 && Wl >= 1, "%s: bad label size (Hl, Wl >= 1)", who);
  VTP_REQUIRE(C >= c_lo && C <= c_hi && H >= 1 && (long)H * per_head <= INT_MAX, "%s: bad shape (H >= 1, %d <= C <= %d)", who, c_lo, c_hi);
  VTP_REQUIRE(seg_shape_ok(B, h, w, Hl, Wl), "%s: bad shape (B, h, w >= 1; edges <= 32768; B Hl Wl < 2^31)", who);
  VTP_REQUIRE(!ld_names || ld_min >= (long)H * C, "%s: bad leading dimension (%s >= H * C)", who, ld_names);
  if (plan) {
    *plan = seg_plan(h, w, Hl, Wl, C);
    VTP_REQUIRE((long)plan->tiles_y * plan->tiles_x * B <= INT_MAX / 4, "%s: too many tiles", who);
  }
  if (tasks) {
    *tasks = (long)B * h * w * H * cdiv(C, 64);
    VTP_REQUIRE((*tasks + 3) / 4 <= INT_MAX, "%s: too many tiles", who);
  }
  return 0;
}

// fixed order: the xor tree of a wave, then the four waves ascending
__device__ __forceinline__ int block_sum_int(int v, int* red) {
  v = wave_sum_int(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// ---------------------------------------------------------------------------------------------------------------- pixel passes
// The tile of label pixels (y0..y1, x0..x1) a workgroup owns and its footprint of ncy x ncx cells from (fy0, fx0), staged in LDS one
// head at a time as rows of Cs floats.
struct SegCorners {
  const float *c00, *c01, *c10, *c11;
};

struct SegTile {
  int y0, x0, y1, x1, fy0, fx0, ncy, ncx, Cs, ncell;

  __device__ __forceinline__ SegTile(int tile, int tiles_x, int th, int tw, int h, int w, int Hl, int Wl, int C) {
    y0 = (tile / tiles_x) * th, x0 = (tile % tiles_x) * tw;
    y1 = min(y0 + th, Hl) - 1, x1 = min(x0 + tw, Wl) - 1;
    fy0 = seg_tap(y0, h, Hl).i0, fx0 = seg_tap(x0, w, Wl).i0;
    ncy = seg_tap(y1, h, Hl).i1 - fy0 + 1, ncx = seg_tap(x1, w, Wl).i1 - fx0 + 1;
    Cs = C | 1;  // odd row length: the cells of neighbouring pixels land on different LDS banks
    ncell = min(ncy * ncx, SEG_CELL_FLOATS / Cs);  // the host planned the tile so that the footprint fits
  }

  // the cells of head hh of image b from Z into `cells`, by the whole workgroup; the caller's barriers stand around it
  __device__ __forceinline__ void stage(float* cells, const float* __restrict__ Z, int ldz, int b, int hh, int h, int w, int C) const {
    for (int i = threadIdx.x; i < ncell * C; i += SEG_THREADS) {
      const int cell = i / C, c = i - cell * C;
      const long row = ((long)b * h + fy0 + cell / ncx) * w + fx0 + cell % ncx;
      cells[cell * Cs + c] = Z[row * ldz + (long)hh * C + c];
    }
  }

  // the staged rows of the four cells a pixel with taps (ty, tx) blends
  __device__ __forceinline__ SegCorners corners(const float* cells, const SegTap& ty, const SegTap& tx) const {
    return {cells + ((ty.i0 - fy0) * ncx + (tx.i0 - fx0)) * Cs, cells + ((ty.i0 - fy0) * ncx + (tx.i1 - fx0)) * Cs,
            cells + ((ty.i1 - fy0) * ncx + (tx.i0 - fx0)) * Cs, cells + ((ty.i1 - fy0) * ncx + (tx.i1 - fx0)) * Cs};
  }
};

// ---------------------------------------------------------------------------------------------------------------- cell passes
// One wave per (cell, head, chunk of 64 outputs), lane = output c (cl = c clamped into the head: a lane past C loads, computes and
// does not store).  Four waves per workgroup, the wave's number made wave-uniform for the compiler.
__device__ __forceinline__ long seg_cell_task() { return (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

struct SegCell {
  long cell;
  int cc, hh, b, iy, ix, c, cl;

  __device__ __forceinline__ SegCell(long task, int h, int w, int H, int C, int chunks) {
    cc = (int)(task % chunks);
    const long t2 = task / chunks;
    hh = (int)(t2 % H);
    cell = t2 / H;
    const int hw = h * w;
    b = (int)(cell / hw), iy = (int)(cell % hw) / w, ix = (int)(cell % w);
    c = cc * 64 + (threadIdx.x & 63), cl = c < C ? c : C - 1;
  }
};

// The gather of a cell pass: sum over the label pixels p that have cell (iy, ix) among their taps of (wy wx) * term(py, px, z_p), z_p
// the pixel's interpolated logit of the lane's output.  A pixel that has the cell among its taps has its other taps in the cell's
// 3 x 3 neighbourhood, whatever the scale: the nine logits sit in registers and the walk over the candidate pixels (raster order,
// wave-uniform) reads only what keep and term read.  keep(py, px) is the wave-uniform skip of a pixel that does not count; term
// follows it for the same pixel.
template <class Keep, class Term>
__device__ __forceinline__ float seg_cell_walk(const SegCell& t, const float* __restrict__ Z, int ldz, int h, int w, int Hl, int Wl, int C,
                                               Keep keep, Term term) {
  const int iy = t.iy, ix = t.ix;
  float nb[3][3];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int yy = min(max(iy + dy - 1, 0), h - 1), xx = min(max(ix + dx - 1, 0), w - 1);  // a clamped neighbour is never a tap
      nb[dy][dx] = Z[((long)t.b * (h * w) + (long)yy * w + xx) * ldz + (long)t.hh * C + t.cl];
    }
  // candidate pixels from the inverse map in integers, two pixels wider than src in [i - 1, i + 1) asks for; membership and weight
  // are the tap function's
  const int ylo = (int)max(0L, (2L * iy - 1) * Hl / (2L * h) - 2), yhi = (int)min((long)Hl - 1, ((2L * iy + 3) * Hl + 2L * h - 1) / (2L * h) + 1);
  const int xlo = (int)max(0L, (2L * ix - 1) * Wl / (2L * w) - 2), xhi = (int)min((long)Wl - 1, ((2L * ix + 3) * Wl + 2L * w - 1) / (2L * w) + 1);
  float acc = 0.f;
  for (int py = ylo; py <= yhi; ++py) {
    const SegTap ty = seg_tap(py, h, Hl);
    if (ty.i0 != iy && ty.i1 != iy) continue;
    const float wy = (ty.i0 == iy ? ty.l0 : 0.f) + (ty.i1 == iy ? ty.l1 : 0.f);
    const int ka = ty.i0 - iy + 1, kb = ty.i1 - iy + 1;
    float ra[3], rb[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) ra[j] = seg_pick(nb[0][j], nb[1][j], nb[2][j], ka), rb[j] = seg_pick(nb[0][j], nb[1][j], nb[2][j], kb);
    for (int px = xlo; px <= xhi; ++px) {
      const SegTap tx = seg_tap(px, w, Wl);
      if (tx.i0 != ix && tx.i1 != ix) continue;
      if (!keep(py, px)) continue;
      const float wx = (tx.i0 == ix ? tx.l0 : 0.f) + (tx.i1 == ix ? tx.l1 : 0.f);
      const int ja = tx.i0 - ix + 1, jb = tx.i1 - ix + 1;
      const float z = seg_blend(seg_pick(ra[0], ra[1], ra[2], ja), seg_pick(ra[0], ra[1], ra[2], jb), seg_pick(rb[0], rb[1], rb[2], ja),
                                seg_pick(rb[0], rb[1], rb[2], jb), ty, tx);
      const float g = term(py, px, z);
      acc = fmaf(wy * wx, g, acc);
    }
  }
  return acc;
}
// The sliced weight step behind vtp_seg_sgd and vtp_depth_sgd (segprobe.hip): every argument check but the caller's own bound on C,
// then seg_wgrad_kernel and seg_sgd_fold_kernel.  `who` names the entry point in the messages.
int seg_sgd_workspace(const char* who, int M, int N, int K);
int seg_sgd_launch(const char* who, float* W, float* bias, float* mW, float* mb, const float* G, int ldg, const float* X, int ldx,
                   const float* lr, int M, int H, int C, int K, float momentum, void* workspace, long workspace_bytes, void* stream);

}  // namespace vtp
