// Reconstruction evaluation (reference: tools/test_reconstruction_hf.py:360-409): what the tool does per batch around its model
// calls, as two launches with no host synchronisation --
//   vtp_recon_metrics  : transform_rev + clamp of both image tensors (:371-376), the LPIPS inputs (:381-382), the byte images of
//                        the PNG folders (:401-402), per-image squared error (:395-397) and per-image SSIM (:392) partials
//   vtp_recon_finalize : per-image PSNR and SSIM from the partials in a fixed order, and the running sums of the evaluation
//
// SSIM is what torchmetrics' StructuralSimilarityIndexMeasure(data_range=1.0) defines with its defaults: an 11x11 Gaussian window
// (sigma 1.5, normalised to sum 1), c1 = 1e-4, c2 = 9e-4, both variances clamped at zero, the covariance not, the mean over all
// channels and window positions.  The library reflect-pads by 5, convolves and crops 5 from every border of the map: that is
// exactly the VALID convolution of the unpadded image over (H-10) x (W-10) window positions (every kept position has its whole
// window inside the image), so there is no padding and no reflect logic here -- a separable filter, rows into LDS, then columns.
//
// The five windowed sums (p, t, p^2, t^2, p t) are formed in fp64: E[x^2] - mu^2 of a flat window cancels to the last bits, and in
// fp32 the rounding of that difference (about 1e-7) is not small against c2.  Each sum is one fma chain over the taps 0..10 in
// that order, whichever tile forms it.  The window is normalised so that this chain over a window of ones does not exceed 1: a
// saturated window then has E[x^2] - mu^2 >= 0, nothing is clamped, and a pair of identical images scores exactly 1.
//
// Geometry.  A workgroup owns one 32 x 32 tile of window positions of one image: it needs the 42 x 42 pixels under them.  It also
// owns the pixels of its tile for the squared error and the byte / LPIPS stores; the last tile row and tile column own the
// remainder up to H and W (at most 10 more: (H-10) <= tiles * 32), so every pixel has exactly one owner.  Partial sums go to the
// caller's scratch, one slot per workgroup; nothing is added across workgroups with float atomics, so results repeat bit for bit.
#include "common.h"
#include "vtp_hip.h"

#include <math.h>

namespace vtp {

constexpr int RC_TS = 32;           // window positions per tile side
constexpr int RC_R = RC_TS + 10;    // pixels under them
constexpr int RC_LD = 44;           // floats per LDS pixel row: 11 x 16 bytes
constexpr int RC_HITEMS = RC_R * (RC_TS / 4);

typedef __attribute__((ext_vector_type(2))) double f64x2;

struct ReconWindow {
  double w[11];
};

// transform_rev then torch.clamp (:265-268, :371-376): a subtraction, an IEEE division, the clamp -- separate statements, so
// nothing here can be contracted
__device__ __forceinline__ float rc_denorm(float v, float sub, float dv) {
  const float a = v - sub;
  const float q = a / dv;
  return fminf(fmaxf(q, 0.0f), 1.0f);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// four neighbouring outputs of the 11-tap filter from 14 inputs: out[o] = sum_j w[j] v[o + j], j = 0..10 in order
__device__ __forceinline__ void rc_filter4(const ReconWindow& win, const double (&v)[14], double (&out)[4]) {
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < 11; ++j) a = fma(win.w[j], v[o + j], a);
    out[o] = a;
  }
}

__device__ __forceinline__ void rc_store4(double* dst, const double (&out)[4]) {
  *(f64x2*)dst = f64x2{out[0], out[1]};
  *(f64x2*)(dst + 2) = f64x2{out[2], out[3]};
}

__global__ __launch_bounds__(256) void recon_metrics_kernel(const float* __restrict__ img, const float* __restrict__ rec, int H, int W,
                                                            int nty, int ntx, f32x4 sub, f32x4 dv, ReconWindow win,
                                                            uint8_t* __restrict__ ref_u8, uint8_t* __restrict__ rec_u8,
                                                            float* __restrict__ ref_lp, float* __restrict__ rec_lp,
                                                            double* __restrict__ scratch) {
  __shared__ __attribute__((aligned(16))) float Ps[RC_R][RC_LD];
  __shared__ __attribute__((aligned(16))) float Ts[RC_R][RC_LD];
  __shared__ __attribute__((aligned(16))) double hb[5][RC_R][RC_TS];
  __shared__ double red[2][4];
  const int tid = threadIdx.x;
  const int tiles = nty * ntx;
  const long b = blockIdx.x / tiles;
  const int t = (int)(blockIdx.x - b * tiles), ty = t / ntx, tx = t - ty * ntx;
  const int y0 = ty * RC_TS, x0 = tx * RC_TS;
  const long plane = (long)H * W;
  const float* ib = img + b * 3 * plane;
  const float* rb = rec + b * 3 * plane;

  // ---- the pixels this tile owns: squared error, byte images, LPIPS inputs (one thread per 4 pixels of a row, all 3 channels)
  const int y1 = ty == nty - 1 ? H : y0 + RC_TS, x1 = tx == ntx - 1 ? W : x0 + RC_TS;
  const int gw = (x1 - x0) / 4, groups = (y1 - y0) * gw;
  double sse = 0.0;
  for (int g = tid; g < groups; g += 256) {
    const int yy = g / gw, xg = g - yy * gw;
    const long p = (long)(y0 + yy) * W + x0 + 4 * xg;  // pixel offset inside the plane, a multiple of 4
    uint32_t wo[3] = {0, 0, 0}, wr[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 vo = *(const f32x4*)(ib + c * plane + p), vr = *(const f32x4*)(rb + c * plane + p);
      f32x4 lo, lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dor = rc_denorm(vo[j], sub[c], dv[c]), drc = rc_denorm(vr[j], sub[c], dv[c]);
        const float o255 = dor * 255.0f;  // orig_denorm[i] * 255.0 (:396) and the byte image's product (:401): one multiply
        const float r255 = drc * 255.0f;
        const float df = o255 - r255;
        sse += (double)df * (double)df;  // the square of an fp32 number is exact in fp64
        const int k = j * 3 + c;
        wo[k >> 2] |= (uint32_t)o255 << ((k & 3) * 8);  // astype(np.uint8) of a value in [0, 255]: truncation
        wr[k >> 2] |= (uint32_t)r255 << ((k & 3) * 8);
        lo[j] = dor * 2.0f - 1.0f;  // dor * 2 is exact: a contraction rounds the same number
        lr[j] = drc * 2.0f - 1.0f;
      }
      if (ref_lp) *(f32x4*)(ref_lp + (b * 3 + c) * plane + p) = lo;
      if (rec_lp) *(f32x4*)(rec_lp + (b * 3 + c) * plane + p) = lr;
    }
    if (ref_u8) {
      uint32_t* o = (uint32_t*)(ref_u8 + (b * plane + p) * 3);  // 12 bytes per 4 pixels, 4-byte aligned (p % 4 == 0)
      o[0] = wo[0], o[1] = wo[1], o[2] = wo[2];
    }
    if (rec_u8) {
      uint32_t* o = (uint32_t*)(rec_u8 + (b * plane + p) * 3);
      o[0] = wr[0], o[1] = wr[1], o[2] = wr[2];
    }
  }

  // ---- SSIM over the tile's window positions, channel by channel
  const int vx = tid & 31, vr0 = (tid >> 5) * 4;  // column pass: this thread's column and the first of its four rows
  double ssum = 0.0;
  for (int c = 0; c < 3; ++c) {
    const float* ic = ib + c * plane;
    const float* rc = rb + c * plane;
    for (int it = tid; it < RC_R * (RC_LD / 4); it += 256) {
      const int ry = it / (RC_LD / 4), q = it - ry * (RC_LD / 4);
      const int y = y0 + ry, x = x0 + 4 * q;
      f32x4 po = {0.f, 0.f, 0.f, 0.f}, pr = {0.f, 0.f, 0.f, 0.f};  // outside the image: only masked positions read it
      if (y < H && x < W) {                                        // W % 4 == 0: four pixels are inside or outside together
        const f32x4 vo = *(const f32x4*)(ic + (long)y * W + x), vr = *(const f32x4*)(rc + (long)y * W + x);
#pragma unroll
        for (int j = 0; j < 4; ++j) po[j] = rc_denorm(vo[j], sub[c], dv[c]), pr[j] = rc_denorm(vr[j], sub[c], dv[c]);
      }
      *(f32x4*)&Ps[ry][4 * q] = po;
      *(f32x4*)&Ts[ry][4 * q] = pr;
    }
    __syncthreads();
    // row pass: (pixel row, group of four window columns) -> the five windowed row sums
    for (int it = tid; it < RC_HITEMS; it += 256) {
      const int r = it / (RC_TS / 4), g4 = (it - r * (RC_TS / 4)) * 4;
      double p[14], q[14], v[14], out[4];
#pragma unroll
      for (int j = 0; j < 14; ++j) p[j] = (double)Ps[r][g4 + j], q[j] = (double)Ts[r][g4 + j];
      rc_filter4(win, p, out);
      rc_store4(&hb[0][r][g4], out);
      rc_filter4(win, q, out);
      rc_store4(&hb[1][r][g4], out);
#pragma unroll
      for (int j = 0; j < 14; ++j) v[j] = p[j] * p[j];
      rc_filter4(win, v, out);
      rc_store4(&hb[2][r][g4], out);
#pragma unroll
      for (int j = 0; j < 14; ++j) v[j] = q[j] * q[j];
      rc_filter4(win, v, out);
      rc_store4(&hb[3][r][g4], out);
#pragma unroll
      for (int j = 0; j < 14; ++j) v[j] = p[j] * q[j];
      rc_filter4(win, v, out);
      rc_store4(&hb[4][r][g4], out);
    }
    __syncthreads();
    // column pass: four window rows of one column per thread, then the SSIM of each position
    double s[5][4];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      double v[14];
#pragma unroll
      for (int i = 0; i < 14; ++i) v[i] = hb[m][vr0 + i][vx];
      rc_filter4(win, v, s[m]);
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      // one operation per statement: with p == t every pair of corresponding terms is the same sequence of roundings
      const double mp = s[0][o], mt = s[1][o];
      const double mpp = mp * mp;
      const double mtt = mt * mt;
      const double mpt = mp * mt;
      const double xp = s[2][o] - mpp;
      const double xt = s[3][o] - mtt;
      const double cov = s[4][o] - mpt;
      const double varp = fmax(xp, 0.0), vart = fmax(xt, 0.0);
      const double two_mpt = 2.0 * mpt;
      const double a1 = two_mpt + 1e-4;
      const double two_cov = 2.0 * cov;
      const double a2 = two_cov + 9e-4;
      const double msum = mpp + mtt;
      const double b1 = msum + 1e-4;
      const double vsum = varp + vart;
      const double b2 = vsum + 9e-4;
      const double num = a1 * a2;
      const double den = b1 * b2;
      const double val = num / den;
      if (y0 + vr0 + o < H - 10 && x0 + vx < W - 10) ssum += val;
    }
    // the next channel's loads write Ps / Ts, which the row pass has finished with; its row pass writes hb after the barrier
    // that follows those loads, so every column pass above is done by then
  }

  // ---- the workgroup's partials, summed in a fixed order, into its own scratch slot
  sse = wave_sum_f64(sse);
  ssum = wave_sum_f64(ssum);
  if ((tid & 63) == 0) red[0][tid >> 6] = sse, red[1][tid >> 6] = ssum;
  __syncthreads();
  if (tid == 0) {
    scratch[2 * (long)blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    scratch[2 * (long)blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// block-wide fp64 sum in a fixed order (256 threads); every thread gets the result
__device__ __forceinline__ double rc_block_sum(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup.  Thread t takes the images t, t + 256, ...; the tiles of an image are summed in tile order.
__global__ __launch_bounds__(256) void recon_finalize_kernel(const double* __restrict__ scratch, long B, int tiles, double n_pix,
                                                             double n_win, float* __restrict__ psnr, float* __restrict__ ssim,
                                                             double* __restrict__ sse_out, const float* __restrict__ lpips,
                                                             double* __restrict__ acc) {
  __shared__ double red[4];
  double s_psnr = 0.0, s_ident = 0.0, s_ssim = 0.0, s_lp = 0.0;
  for (long b = threadIdx.x; b < B; b += 256) {
    double sse = 0.0, ss = 0.0;
    for (int t = 0; t < tiles; ++t) {
      sse += scratch[2 * (b * tiles + t)];
      ss += scratch[2 * (b * tiles + t) + 1];
    }
    // calculate_psnr (:49-63): mse == 0 -> inf, else 20 log10(255 / sqrt(mse))
    const double ps = sse == 0.0 ? (double)INFINITY : 20.0 * log10(255.0 / sqrt(sse / n_pix));
    const double sm = ss / n_win;
    psnr[b] = (float)ps;
    ssim[b] = (float)sm;
    if (sse_out) sse_out[b] = sse;
    s_psnr += ps;
    s_ident += sse == 0.0 ? 1.0 : 0.0;
    s_ssim += sm;
    if (lpips) s_lp += (double)lpips[b];
  }
  s_psnr = rc_block_sum(s_psnr, red);
  s_ident = rc_block_sum(s_ident, red);
  s_ssim = rc_block_sum(s_ssim, red);
  s_lp = rc_block_sum(s_lp, red);
  if (threadIdx.x == 0) {
    acc[0] += s_psnr;             // PSNR is averaged over images (:395-397, :429)
    acc[1] += (double)B;
    acc[2] += s_ident;
    acc[3] += s_ssim;
    acc[4] += s_ssim / (double)B;  // SSIM and LPIPS are averaged over the batches' means (:386, :392, :428, :430)
    acc[5] += 1.0;
    if (lpips) {
      acc[6] += s_lp / (double)B;
      acc[7] += s_lp;
    }
  }
}

}  // namespace vtp

using namespace vtp;

static bool rc_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static int rc_tiles(int n) { return (n - 10 + RC_TS - 1) / RC_TS; }

// exp(-d^2 / (2 sigma^2)) / sum, d = -5..5, sigma = 1.5; then the centre tap is lowered by single ulps until the kernel's chain
// over a window of ones (fma, taps 0..10) does not exceed 1 (see the head of this file)
static ReconWindow recon_window() {
  ReconWindow win;
  double s = 0.0;
  for (int j = 0; j < 11; ++j) s += win.w[j] = exp(-(double)((j - 5) * (j - 5)) / (2.0 * 1.5 * 1.5));
  for (int j = 0; j < 11; ++j) win.w[j] /= s;
  for (;;) {
    double a = 0.0;
    for (int j = 0; j < 11; ++j) a = fma(win.w[j], 1.0, a);
    if (a <= 1.0) return win;
    win.w[5] = nextafter(win.w[5], 0.0);
  }
}

static int recon_shape_ok(const char* who, long B, int H, int W) {
  VTP_REQUIRE(B >= 1, "%s: B >= 1", who);
  VTP_REQUIRE(H >= 11 && W >= 11, "%s: H and W >= 11 (one 11 x 11 SSIM window), got %d x %d", who, H, W);
  VTP_REQUIRE(W % 4 == 0, "%s: W %% 4 == 0, got %d", who, W);
  VTP_REQUIRE(B * rc_tiles(H) * rc_tiles(W) <= 0x7fffffffL / 2, "%s: too many tiles for one launch", who);
  return VTP_OK;
}

extern "C" int vtp_recon_scratch_doubles(long B, int H, int W) {
  if (recon_shape_ok("vtp_recon_scratch_doubles", B, H, W) != VTP_OK) return VTP_ERR_ARG;
  return (int)(2 * B * rc_tiles(H) * rc_tiles(W));
}

extern "C" int vtp_recon_metrics(const float* images, const float* recon, long B, int H, int W, const float* sub3, const float* div3,
                                 void* ref_u8, void* rec_u8, float* ref_lp, float* rec_lp, double* scratch, long scratch_len,
                                 void* stream) {
  VTP_REQUIRE(images && recon && sub3 && div3 && scratch, "vtp_recon_metrics: null pointer (images, recon, sub3, div3, scratch)");
  if (recon_shape_ok("vtp_recon_metrics", B, H, W) != VTP_OK) return VTP_ERR_ARG;
  const int nty = rc_tiles(H), ntx = rc_tiles(W);
  VTP_REQUIRE(scratch_len >= 2 * B * nty * ntx, "vtp_recon_metrics: scratch too small (%ld doubles, needs %ld)", scratch_len,
              2 * B * nty * ntx);
  VTP_REQUIRE(rc_aligned(images, 16) && rc_aligned(recon, 16) && rc_aligned(ref_lp, 16) && rc_aligned(rec_lp, 16),
              "vtp_recon_metrics: images, recon, ref_lp and rec_lp must be 16-byte aligned");
  VTP_REQUIRE(rc_aligned(ref_u8, 4) && rc_aligned(rec_u8, 4) && rc_aligned(scratch, 8),
              "vtp_recon_metrics: ref_u8 / rec_u8 must be 4-byte aligned, scratch 8-byte aligned");
  static const ReconWindow win = recon_window();
  const f32x4 a = {sub3[0], sub3[1], sub3[2], 0.f}, d = {div3[0], div3[1], div3[2], 1.f};
  hipLaunchKernelGGL(recon_metrics_kernel, dim3((unsigned)(B * nty * ntx)), dim3(256), 0, (hipStream_t)stream, images, recon, H, W, nty,
                     ntx, a, d, win, (uint8_t*)ref_u8, (uint8_t*)rec_u8, ref_lp, rec_lp, scratch);
  return check_launch("recon_metrics");
}

extern "C" int vtp_recon_finalize(const double* scratch, long scratch_len, long B, int H, int W, float* psnr, float* ssim, double* sse,
                                  const float* lpips, double* acc, void* stream) {
  VTP_REQUIRE(scratch && psnr && ssim && acc, "vtp_recon_finalize: null pointer (scratch, psnr, ssim, acc)");
  if (recon_shape_ok("vtp_recon_finalize", B, H, W) != VTP_OK) return VTP_ERR_ARG;
  const int tiles = rc_tiles(H) * rc_tiles(W);
  VTP_REQUIRE(scratch_len >= 2 * B * tiles, "vtp_recon_finalize: scratch too small (%ld doubles, needs %ld)", scratch_len,
              2 * B * tiles);
  VTP_REQUIRE(rc_aligned(scratch, 8) && rc_aligned(acc, 8) && rc_aligned(sse, 8),
              "vtp_recon_finalize: scratch, acc and sse must be 8-byte aligned");
  hipLaunchKernelGGL(recon_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, B, tiles, 3.0 * H * W,
                     3.0 * (H - 10) * (double)(W - 10), psnr, ssim, sse, lpips, acc);
  return check_launch("recon_finalize");
}
