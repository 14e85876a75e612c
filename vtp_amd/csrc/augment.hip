// The DINO multi-crop augmentation (the recipe of DINOv2's DataAugmentationDINO, the arithmetic of torchvision's float-tensor
// path) from decoded byte images to the normalised fp32 crops the trainer takes, as two launches with no host synchronisation --
//   augment_resample : box -> S x S antialiased bicubic resampling (+ flip), the gray sum of each tile at the point of the colour
//                      chain where the contrast stands, and -- for a crop that needs neither a contrast mean nor a blur -- the
//                      rest of the chain and the output itself
//   augment_finish   : for every other crop, the colour chain with the crop's mean, the 9 x 9 blur over LDS tiles with a 4-pixel
//                      halo of fully colour-processed pixels, solarize, normalise
//
// One row of the table f32 [N, 16] drives one crop n = v * B + b of image b:
//   0..3  y0 x0 h w   the box, in source pixels
//   4     flags       1 flip | 2 colour jitter | 4 grayscale | 8 solarize
//   5..8  order       the jitter's operations in the order they run: 0 brightness 1 contrast 2 saturation 3 hue, -1 none
//   9..12 factors     brightness contrast saturation hue
//   13    sigma       of the blur; <= 0: no blur
//   14,15 unused
//
// Resampling is F.interpolate(crop, (S, S), mode="bicubic", antialias=True, align_corners=False): per axis scale = box / S, support
// 2 max(scale, 1), cubic a = -0.5, the taps outside the crop dropped and the rest renormalised; rows first (along x), then columns.
// A workgroup owns one 32 x 32 output tile.  It walks the source rows under the tile 16 at a time: the bytes under the tile's
// columns go to LDS by 4-byte loads (row starts are 4-byte aligned: Ws % 4 == 0), the row filter writes 16 x 32 fp32 values per
// channel to LDS, and each thread adds the rows of that chunk to its four pixels' column sums -- in ascending row order whichever
// chunk holds them.  u8 -> float is a 256-entry table of (float)i / 255.0f, the IEEE quotient ToTensor forms.
//
// The table lives on the device, so nothing here can refuse a bad row; the box is clamped into the image and to 8 S per axis
// instead (the host checks both and raises).  The tile sums are fp64, one slot per workgroup, and augment_finish adds them in a
// fixed order: no float atomics, a run repeats bit for bit.
#include "common.h"
#include "vtp_hip.h"

#include <limits.h>
#include <math.h>

namespace vtp {

constexpr int AG_T = 32;                                    // output pixels per tile side
constexpr int AG_MAXR = 8;                                  // largest box / S per axis
constexpr int AG_TAPS = 2 * 2 * AG_MAXR + 1;                // taps per output pixel at that ratio
constexpr int AG_CH = 16;                                   // source rows per chunk
constexpr int AG_FOOT = (AG_T - 1) * AG_MAXR + AG_TAPS + 9; // source pixels under one tile, per axis, with room to spare
constexpr int AG_ROWW = (AG_FOOT * 3 + 6 + 3) / 4;          // 4-byte words per staged row (both ends rounded to a word)
constexpr int AG_HALO = 4;
constexpr int AG_P = AG_T + 2 * AG_HALO;                    // 40: tile plus halo

struct AgRow {
  int y0, x0, h, w;
  int flip, jitter, gray, solarize;
  int op[4];
  float fb, fc, fs, fh;
  float sigma;
  int contrast;  // the jitter runs and holds a contrast: the crop needs its mean
};

__device__ __forceinline__ int ag_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ AgRow ag_row(const float* __restrict__ table, long n, int Hs, int Ws, int S) {
  const f32x4* t = (const f32x4*)(table + n * 16);
  const f32x4 a = t[0], b = t[1], c = t[2], d = t[3];
  AgRow r;
  const int lim = AG_MAXR * S;
  r.h = ag_clampi((int)a[2], 1, Hs < lim ? Hs : lim);
  r.w = ag_clampi((int)a[3], 1, Ws < lim ? Ws : lim);
  r.y0 = ag_clampi((int)a[0], 0, Hs - r.h);
  r.x0 = ag_clampi((int)a[1], 0, Ws - r.w);
  const int f = (int)b[0];
  r.flip = f & 1, r.jitter = (f >> 1) & 1, r.gray = (f >> 2) & 1, r.solarize = (f >> 3) & 1;
  r.op[0] = (int)b[1], r.op[1] = (int)b[2], r.op[2] = (int)b[3], r.op[3] = (int)c[0];
  r.fb = c[1], r.fc = c[2], r.fs = c[3], r.fh = d[0];
  r.sigma = d[1];
  r.contrast = r.jitter && (r.op[0] == 1 || r.op[1] == 1 || r.op[2] == 1 || r.op[3] == 1);
  return r;
}

__device__ __forceinline__ float ag_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float ag_gray(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
__device__ __forceinline__ float ag_blend(float a, float b, float f) { return ag_clamp01(f * a + (1.0f - f) * b); }

// torchvision's _rgb2hsv, h = (h + f) % 1, _hsv2rgb
__device__ __forceinline__ void ag_hue(float& r, float& g, float& b, float f) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.0f : maxc);
  const float dv = eqc ? 1.0f : cr;
  const float rc = (maxc - r) / dv, gc = (maxc - g) / dv, bc = (maxc - b) / dv;
  float h;
  if (maxc == r) h = bc - gc;
  else if (maxc == g) h = 2.0f + rc - bc;
  else h = 4.0f + gc - rc;
  h = fmodf(h / 6.0f + 1.0f, 1.0f);
  h = h + f;
  h = h - floorf(h);  // python's % 1 of a value in (-1, 2)
  if (h >= 1.0f) h = 0.0f;
  const float h6 = h * 6.0f;
  const float fl = floorf(h6);
  const float fr = h6 - fl;
  const int i = ((int)fl) % 6;
  const float v = maxc;
  const float p = ag_clamp01(v * (1.0f - s));
  const float q = ag_clamp01(v * (1.0f - fr * s));
  const float t = ag_clamp01(v * (1.0f - s * (1.0f - fr)));
  switch (i) {
    case 0: r = v, g = t, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = t; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = t, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
  }
}

// the jitter's operations in the row's order; with `prefix` it stops in front of the contrast (what its mean is taken of)
__device__ __forceinline__ void ag_jitter(float& r, float& g, float& b, const AgRow& p, float mean, bool prefix) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = p.op[k];
    if (op == 0) {
      r = ag_blend(r, 0.0f, p.fb), g = ag_blend(g, 0.0f, p.fb), b = ag_blend(b, 0.0f, p.fb);
    } else if (op == 1) {
      if (prefix) return;
      r = ag_blend(r, mean, p.fc), g = ag_blend(g, mean, p.fc), b = ag_blend(b, mean, p.fc);
    } else if (op == 2) {
      const float y = ag_gray(r, g, b);
      r = ag_blend(r, y, p.fs), g = ag_blend(g, y, p.fs), b = ag_blend(b, y, p.fs);
    } else if (op == 3) {
      ag_hue(r, g, b, p.fh);
    }
  }
}

// jitter and grayscale: what the blur reads
__device__ __forceinline__ void ag_colour(float& r, float& g, float& b, const AgRow& p, float mean) {
  if (p.jitter) ag_jitter(r, g, b, p, mean, false);
  if (p.gray) {
    const float y = ag_gray(r, g, b);
    r = y, g = y, b = y;
  }
}

// solarize and normalise: a comparison, a subtraction and an IEEE division per statement, nothing to contract
__device__ __forceinline__ float ag_tail(float v, int solarize, float mean, float stdv) {
  if (solarize && v >= 128.0f / 255.0f) v = 1.0f - v;
  const float a = v - mean;
  return a / stdv;
}

__device__ __forceinline__ double ag_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float ag_cubic(float x) {
  const float A = -0.5f;
  x = fabsf(x);
  if (x < 1.0f) return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  if (x < 2.0f) return ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
  return 0.0f;
}

// the taps of output index u along an axis of `box` source pixels: first tap mn, count sz (<= AG_TAPS), weights w[0..sz)
__device__ __forceinline__ void ag_axis(int u, int box, int S, float* w, int& mn, int& sz) {
  const float scale = (float)box / (float)S;
  const float support = scale >= 1.0f ? 2.0f * scale : 2.0f;
  const float inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
  const float center = scale * ((float)u + 0.5f);
  mn = max((int)(center - support + 0.5f), 0);
  sz = ag_clampi(min((int)(center + support + 0.5f), box) - mn, 0, AG_TAPS);
  float tot = 0.0f;
  for (int k = 0; k < sz; ++k) {
    const float v = ag_cubic(((float)(k + mn) - center + 0.5f) * inv);
    w[k] = v;
    tot += v;
  }
  if (tot != 0.0f)
    for (int k = 0; k < sz; ++k) w[k] = w[k] / tot;
}

// four pixels of one row: to `dst` planes (stride S * S) at offset o, as one 16-byte store per channel where the layout allows
__device__ __forceinline__ void ag_store4(float* __restrict__ dst, long plane, long o, int valid, bool vec, const float (&v)[3][4]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* d = dst + c * plane + o;
    if (vec) {
      *(f32x4*)d = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < valid) d[q] = v[c][q];
    }
  }
}

__global__ __launch_bounds__(256) void augment_resample_kernel(const uint8_t* __restrict__ src, int B, int Hs, int Ws,
                                                               const float* __restrict__ table, int S, int nt, f32x4 mean, f32x4 stdv,
                                                               float* __restrict__ inter, double* __restrict__ partial,
                                                               float* __restrict__ out) {
  __shared__ float lut[256];
  __shared__ float wx[AG_T][AG_TAPS], wy[AG_T][AG_TAPS];
  __shared__ int xmn[AG_T], xsz[AG_T], ymn[AG_T], ysz[AG_T];
  __shared__ uint32_t stage[AG_CH][AG_ROWW];
  __shared__ __attribute__((aligned(16))) float hbuf[AG_CH][3][AG_T];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int tiles = nt * nt;
  const long n = blockIdx.x / tiles;
  const int t = (int)(blockIdx.x - n * tiles), ty = t / nt, tx = t - ty * nt;
  const int oy0 = ty * AG_T, ox0 = tx * AG_T;
  const AgRow p = ag_row(table, n, Hs, Ws, S);
  const int b = (int)(n % B);
  const uint8_t* img = src + (long)b * Hs * Ws * 3;

  lut[tid] = (float)tid / 255.0f;
  if (tid < AG_T) {  // the tile's columns; a flipped crop takes the taps of the mirrored column
    const int x = ox0 + tid;
    int mn = 0, sz = 0;
    if (x < S) ag_axis(p.flip ? S - 1 - x : x, p.w, S, wx[tid], mn, sz);
    xmn[tid] = mn, xsz[tid] = sz;
  } else if (tid >= 64 && tid < 64 + AG_T) {
    const int i = tid - 64, y = oy0 + i;
    int mn = 0, sz = 0;
    if (y < S) ag_axis(y, p.h, S, wy[i], mn, sz);
    ymn[i] = mn, ysz[i] = sz;
  }
  __syncthreads();
  int xlo = INT_MAX, xhi = 0, ylo = INT_MAX, yhi = 0;  // the source pixels under the tile, relative to the box
  for (int i = 0; i < AG_T; ++i) {
    if (xsz[i] > 0) xlo = min(xlo, xmn[i]), xhi = max(xhi, xmn[i] + xsz[i]);
    if (ysz[i] > 0) ylo = min(ylo, ymn[i]), yhi = max(yhi, ymn[i] + ysz[i]);
  }
  if (xhi - xlo > AG_FOOT) xhi = xlo + AG_FOOT;  // cannot happen with box <= 8 S; keeps the staging inside its LDS rows
  const int bs = ((p.x0 + xlo) * 3) & ~3;              // first staged byte of a source row
  const int nd = xhi > xlo ? (((p.x0 + xhi) * 3 + 3) & ~3) / 4 - bs / 4 : 0;  // words per row: <= AG_ROWW, inside the row
  const uint8_t* sbytes = (const uint8_t*)&stage[0][0];

  const int j4 = (tid & 7) * 4, i = tid >> 3;  // this thread's four columns and its row of the tile
  const int my_mn = ymn[i], my_end = ymn[i] + ysz[i];
  float acc[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[c][q] = 0.0f;

  for (int c0 = ylo; c0 < yhi; c0 += AG_CH) {
    const int nrows = min(AG_CH, yhi - c0);
    for (int it = tid; it < nrows * nd; it += 256) {
      const int r = it / nd, d = it - r * nd;
      stage[r][d] = *(const uint32_t*)(img + ((long)(p.y0 + c0 + r) * Ws) * 3 + bs + 4 * d);
    }
    __syncthreads();
    for (int it = tid; it < nrows * AG_T; it += 256) {
      const int r = it >> 5, j = it & 31;
      const int sz = xsz[j];
      float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
      const uint8_t* px = sbytes + r * (AG_ROWW * 4) + ((p.x0 + xmn[j]) * 3 - bs);
      const int last = (xhi - xmn[j]);  // taps beyond the staged pixels (never, see above) are not read
      for (int k = 0; k < sz && k < last; ++k) {
        const float w = wx[j][k];
        a0 = fmaf(w, lut[px[3 * k]], a0);
        a1 = fmaf(w, lut[px[3 * k + 1]], a1);
        a2 = fmaf(w, lut[px[3 * k + 2]], a2);
      }
      hbuf[r][0][j] = a0, hbuf[r][1][j] = a1, hbuf[r][2][j] = a2;
    }
    __syncthreads();
    const int r0 = max(c0, my_mn), r1 = min(c0 + nrows, my_end);
    for (int r = r0; r < r1; ++r) {
      const float w = wy[i][r - my_mn];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 v = *(const f32x4*)&hbuf[r - c0][c][j4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[c][q] = fmaf(w, v[q], acc[c][q]);
      }
    }
    // the next chunk's row filter writes hbuf after the barrier that follows its staging: every column sum above is done by then
  }

  const int y = oy0 + i, x = ox0 + j4;
  const int valid = y < S ? ag_clampi(S - x, 0, 4) : 0;
  const long plane = (long)S * S;
  const long o = n * 3 * plane + (long)y * S + x;
  const bool vec = valid == 4 && (S & 3) == 0;
  const bool later = p.contrast || p.sigma > 0.0f;  // augment_finish writes this crop
  float v[3][4];
  double gsum = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float r = ag_clamp01(acc[0][q]), g = ag_clamp01(acc[1][q]), bl = ag_clamp01(acc[2][q]);
    if (later) {
      v[0][q] = r, v[1][q] = g, v[2][q] = bl;
      if (p.contrast) {
        ag_jitter(r, g, bl, p, 0.0f, true);
        if (q < valid) gsum += (double)ag_gray(r, g, bl);
      }
    } else {
      ag_colour(r, g, bl, p, 0.0f);
      v[0][q] = ag_tail(r, p.solarize, mean[0], stdv[0]);
      v[1][q] = ag_tail(g, p.solarize, mean[1], stdv[1]);
      v[2][q] = ag_tail(bl, p.solarize, mean[2], stdv[2]);
    }
  }
  if (valid > 0) ag_store4(later ? inter : out, plane, o, valid, vec, v);
  gsum = ag_wave_sum_f64(gsum);
  if ((tid & 63) == 0) red[tid >> 6] = gsum;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void augment_finish_kernel(const float* __restrict__ table, int Hs, int Ws, int S, int nt, f32x4 mean,
                                                             f32x4 stdv, const float* __restrict__ inter,
                                                             const double* __restrict__ partial, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float P[3][AG_P][AG_P];
  __shared__ __attribute__((aligned(16))) float Hb[3][AG_P][AG_T];
  __shared__ float mean_s;
  const int tid = threadIdx.x;
  const int tiles = nt * nt;
  const long n = blockIdx.x / tiles;
  const AgRow p = ag_row(table, n, Hs, Ws, S);
  const bool blur = p.sigma > 0.0f;
  if (!p.contrast && !blur) return;  // augment_resample has written this crop
  const int t = (int)(blockIdx.x - n * tiles), ty = t / nt, tx = t - ty * nt;
  const int oy0 = ty * AG_T, ox0 = tx * AG_T;
  const long plane = (long)S * S;
  const float* in = inter + n * 3 * plane;

  float gmean = 0.0f;
  if (p.contrast) {  // the crop's tiles in a fixed order: lane l takes tiles l, l + 64, ..., then the wave's tree
    if (tid < 64) {
      double s = 0.0;
      for (int k = tid; k < tiles; k += 64) s += partial[n * tiles + k];
      s = ag_wave_sum_f64(s);
      if (tid == 0) mean_s = (float)(s / (double)plane);
    }
    __syncthreads();
    gmean = mean_s;
  }

  const int j4 = (tid & 7) * 4, i = tid >> 3;
  const int y = oy0 + i, x = ox0 + j4;
  const int valid = y < S ? ag_clampi(S - x, 0, 4) : 0;
  const bool vec = valid == 4 && (S & 3) == 0;
  const long o = n * 3 * plane + (long)y * S + x;
  float v[3][4];

  if (!blur) {
    if (valid == 0) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long e = (long)y * S + min(x + q, S - 1);
      float r = in[e], g = in[plane + e], bl = in[2 * plane + e];
      ag_colour(r, g, bl, p, gmean);
      v[0][q] = ag_tail(r, p.solarize, mean[0], stdv[0]);
      v[1][q] = ag_tail(g, p.solarize, mean[1], stdv[1]);
      v[2][q] = ag_tail(bl, p.solarize, mean[2], stdv[2]);
    }
    ag_store4(out, plane, o, valid, vec, v);
    return;
  }

  float gw[9];
  {
    float tot = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float q = (float)(k - 4) / p.sigma;
      gw[k] = expf(-0.5f * (q * q));
      tot += gw[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) gw[k] = gw[k] / tot;
  }
  // tile plus halo, reflected at the crop's border (S >= 5: the mirror image lies inside the crop), through the colour chain
  for (int it = tid; it < AG_P * AG_P; it += 256) {
    const int ly = it / AG_P, lx = it - ly * AG_P;
    int gy = oy0 - AG_HALO + ly, gx = ox0 - AG_HALO + lx;
    gy = gy < 0 ? -gy : (gy >= S ? 2 * (S - 1) - gy : gy);
    gx = gx < 0 ? -gx : (gx >= S ? 2 * (S - 1) - gx : gx);
    gy = ag_clampi(gy, 0, S - 1), gx = ag_clampi(gx, 0, S - 1);  // beyond the halo of a partial tile: read, never used
    const long e = (long)gy * S + gx;
    float r = in[e], g = in[plane + e], bl = in[2 * plane + e];
    ag_colour(r, g, bl, p, gmean);
    P[0][ly][lx] = r, P[1][ly][lx] = g, P[2][ly][lx] = bl;
  }
  __syncthreads();
  for (int it = tid; it < 3 * AG_P * (AG_T / 4); it += 256) {  // along x: four outputs from twelve inputs
    const int c = it / (AG_P * (AG_T / 4)), rem = it - c * (AG_P * (AG_T / 4));
    const int ly = rem / (AG_T / 4), g4 = (rem - ly * (AG_T / 4)) * 4;
    float in12[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const f32x4 w4 = *(const f32x4*)&P[c][ly][g4 + 4 * k];
      in12[4 * k] = w4[0], in12[4 * k + 1] = w4[1], in12[4 * k + 2] = w4[2], in12[4 * k + 3] = w4[3];
    }
    f32x4 r4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float a = 0.0f;
#pragma unroll
      for (int k = 0; k < 9; ++k) a = fmaf(gw[k], in12[q + k], a);
      r4[q] = a;
    }
    *(f32x4*)&Hb[c][ly][g4] = r4;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {  // along y, then solarize and normalise
    f32x4 a = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const f32x4 h4 = *(const f32x4*)&Hb[c][i + k][j4];
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = fmaf(gw[k], h4[q], a[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) v[c][q] = ag_tail(a[q], p.solarize, mean[c], stdv[c]);
  }
  if (valid > 0) ag_store4(out, plane, o, valid, vec, v);
}

}  // namespace vtp

using namespace vtp;

static bool ag_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static int ag_tiles(int S) { return (S + AG_T - 1) / AG_T; }

// doubles of tile sums in front (an even count: the fp32 crops behind them stay 16-byte aligned), then f32 [N, 3, S, S]
static long ag_partial_floats(long N, int S) { return 2 * ((N * ag_tiles(S) * ag_tiles(S) + 1) / 2 * 2); }

static int augment_shape_ok(const char* who, long N, int S) {
  VTP_REQUIRE(N >= 1, "%s: N >= 1", who);
  VTP_REQUIRE(S >= 5, "%s: S >= 5 (the blur reflects by 4), got %d", who, S);
  VTP_REQUIRE(S <= 4096, "%s: S <= 4096, got %d", who, S);
  VTP_REQUIRE(N * ag_tiles(S) * ag_tiles(S) <= 0x7fffffffL, "%s: too many tiles for one launch", who);
  VTP_REQUIRE(ag_partial_floats(N, S) + N * 3 * S * S <= 0x7fffffffL, "%s: scratch does not fit 2^31 floats", who);
  return VTP_OK;
}

extern "C" int vtp_augment_scratch_floats(long N, int S) {
  if (augment_shape_ok("vtp_augment_scratch_floats", N, S) != VTP_OK) return VTP_ERR_ARG;
  return (int)(ag_partial_floats(N, S) + N * 3 * S * S);
}

extern "C" int vtp_augment_crops(const void* src_u8, long B, int Hs, int Ws, const float* table, long N, int S, const float* mean3,
                                 const float* std3, float* out, float* scratch, long scratch_len, void* stream) {
  VTP_REQUIRE(src_u8 && table && mean3 && std3 && out && scratch,
              "vtp_augment_crops: null pointer (src_u8, table, mean3, std3, out, scratch)");
  VTP_REQUIRE(B >= 1 && B <= 0x7fffffffL && Hs >= 1 && Ws >= 1, "vtp_augment_crops: B, Hs, Ws >= 1");
  VTP_REQUIRE(Ws % 4 == 0, "vtp_augment_crops: Ws %% 4 == 0, got %d", Ws);
  if (augment_shape_ok("vtp_augment_crops", N, S) != VTP_OK) return VTP_ERR_ARG;
  VTP_REQUIRE(N % B == 0, "vtp_augment_crops: N must be views * B (crop n reads image n %% B), got N = %ld, B = %ld", N, B);
  VTP_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "vtp_augment_crops: std3 must not be zero");
  const long pf = ag_partial_floats(N, S);
  VTP_REQUIRE(scratch_len >= pf + N * 3 * S * S, "vtp_augment_crops: scratch too small (%ld floats, needs %ld)", scratch_len,
              pf + N * 3 * S * S);
  VTP_REQUIRE(ag_aligned(src_u8, 4) && ag_aligned(table, 16) && ag_aligned(out, 16) && ag_aligned(scratch, 16),
              "vtp_augment_crops: src_u8 must be 4-byte aligned, table, out and scratch 16-byte aligned");
  const int nt = ag_tiles(S);
  const f32x4 m = {mean3[0], mean3[1], mean3[2], 0.f}, s = {std3[0], std3[1], std3[2], 1.f};
  double* partial = (double*)scratch;
  float* inter = scratch + pf;
  const dim3 grid((unsigned)(N * nt * nt));
  hipLaunchKernelGGL(augment_resample_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src_u8, (int)B, Hs, Ws, table, S,
                     nt, m, s, inter, partial, out);
  const int rc = check_launch("augment_resample");
  if (rc != VTP_OK) return rc;
  hipLaunchKernelGGL(augment_finish_kernel, grid, dim3(256), 0, (hipStream_t)stream, table, Hs, Ws, S, nt, m, s, (const float*)inter,
                     (const double*)partial, out);
  return check_launch("augment_finish");
}
