// FID on the device (reference: _calculate_fid_manual, tools/test_reconstruction_hf.py:121-176): Inception-v3 features in exact
// fp32 and the Frechet statistics in fp64.
//   vtp_conv2d_f32         : implicit-GEMM convolution on the f32-input MFMA (mfma_f32.h), NHWC, BatchNorm folded into (w, bias)
//   vtp_pool3x3_f32        : 3 x 3 max / average pooling (stride 1 pad 1, or stride 2 pad 0) into a channel slice
//   vtp_global_avgpool_f32 : [B, HW, C] -> [B, C]
//   vtp_resize_bilinear_nhwc : F.interpolate(bilinear, align_corners=False) + affine, NCHW -> NHWC (the repack at equal sizes)
//   vtp_fid_accum          : sum x and sum x x^T of feature rows into fp64 buffers, rows in order, every element owned by one thread
// Nothing here uses float atomics or splits a sum: every result is the same bits from run to run, whatever the batch size.
#include "common.h"
#include "mfma_f32.h"
#include "vtp_hip.h"

namespace vtp {

// ---------------------------------------------------------------------------------------------------------------- convolution
// GEMM view: M = B Ho Wo output pixels, N = Cout, K = kh kw Cin in the order (ky, kx, ci) -- the weight's own layout
// [Cout][kh][kw][Cin].  One workgroup of four waves computes 128 rows x (32 NT) columns: wave w owns rows 32 w .. 32 w + 31 and NT
// 32-column tiles, each ONE accumulator over the whole of K (the MFMA's dependent latency equals its issue interval).  The
// accumulator starts at the bias, so an output element is
//     fma(x_{K-1}, w_{K-1}, ... fma(x_1, w_1, fma(x_0, w_0, bias)))
// in k order, wherever it lands in a tile.  Zero padding of the image, the zero tail of the last K chunk and rows / columns past
// M / N contribute fma(0, ., acc) = acc or are never stored.
//
// Staging: K goes in chunks of 32.  Thread t stages the 16-byte quad kq = t & 7 of the chunk for rows (t >> 3) + 32 j: with
// Cin % 4 == 0 a quad lies inside one filter tap and is one 16-byte load along Cin (a wave's load covers eight rows x 128
// contiguous bytes); otherwise (the first layer, Cin = 3) it is four scalar loads.  The quads of chunk c + 1 are loaded into
// registers before chunk c is multiplied, and written to LDS after it.
// LDS image: [row][36] floats (rows padded by 16 bytes: 16 consecutive rows start in 16 different 16-byte slots of the bank row).
// Within each group of 8 k the even k sit in floats 0..3 and the odd k in floats 4..7, so that the 16 bytes lane half h reads at
// float 8 g + 4 h are k = 8 g + {h, 2 + h, 4 + h, 6 + h}: element e of both operands feeds MFMA e, whose two products are
// k = 8 g + 2 e (half 0) then 8 g + 2 e + 1 (half 1) -- ascending k.
constexpr int CV_BM = 128, CV_BK = 32, CV_LD = 36, CV_THREADS = 256;

struct ConvArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  int H, W, Cin, Cout, kh, kw, stride, ph, pw, Ho, Wo, M, K, relu, c0, Ctot;
};

// the tap (ky, kx) and channel ci of a k index
struct KPos {
  int ky, kx, ci;
};
__device__ __forceinline__ KPos kpos(int k, int Cin, int kw) {
  const int tap = k / Cin;
  return {tap / kw, tap % kw, k - tap * Cin};
}

template <bool VEC>
__device__ __forceinline__ f32x4 conv_load_x(const ConvArgs& a, long base, int iy0, int ix0, bool row_ok, int k, KPos p) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!row_ok) return v;
  if constexpr (VEC) {
    const int iy = iy0 + p.ky, ix = ix0 + p.kx;
    if (k < a.K && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = *(const f32x4*)(a.x + base + ((long)iy * a.W + ix) * a.Cin + p.ci);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (k + e < a.K) {
        const KPos q = kpos(k + e, a.Cin, a.kw);
        const int iy = iy0 + q.ky, ix = ix0 + q.kx;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v[e] = a.x[base + ((long)iy * a.W + ix) * a.Cin + q.ci];
      }
    }
  }
  return v;
}

template <bool VEC>
__device__ __forceinline__ f32x4 conv_load_w(const ConvArgs& a, int n, int k) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (n >= a.Cout) return v;
  const float* p = a.w + (long)n * a.K + k;
  if constexpr (VEC) {
    if (k < a.K) v = *(const f32x4*)p;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < a.K) v[e] = p[e];
  }
  return v;
}

// quad kq of a row: (k0, k2) to floats 8 g + 2 s, (k1, k3) to floats 8 g + 4 + 2 s, g = kq >> 1, s = kq & 1
__device__ __forceinline__ void conv_put(float* row, int kq, f32x4 v) {
  float* p = row + 8 * (kq >> 1) + 2 * (kq & 1);
  *(f32x2*)p = f32x2{v[0], v[2]};
  *(f32x2*)(p + 4) = f32x2{v[1], v[3]};
}

// BLK: the K sum in blocks.  Each chunk of 32 k is a chain of its own that starts at 0, and the chunk sums are added to the
// accumulator (which starts at the bias) in k order: a rounding error is then relative to a 32-term partial sum or to one of K / 32
// running sums, not to one of K -- what the long reductions of VGG16 (K = 576 .. 4608) need to stay as close to fp64 as torch's own
// fp32 convolutions do.  An output element is still a fixed sequence of operations on its own inputs.
template <int NT, bool VEC, bool BLK>
__global__ __launch_bounds__(CV_THREADS) void conv2d_f32_kernel(const ConvArgs a) {
  constexpr int BN = 32 * NT, XQ = CV_BM / 32, WQ = BN / 32;
  __shared__ __attribute__((aligned(16))) float lds[(CV_BM + BN) * CV_LD];
  float* xs = lds;
  float* wsm = lds + CV_BM * CV_LD;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, half = lane >> 5, wv = tid >> 6;
  const int m0 = blockIdx.x * CV_BM, n0 = blockIdx.y * BN;
  const int kq = tid & 7, srow = tid >> 3;

  // the thread's staging rows: image base, top-left input coordinate
  long xbase[XQ];
  int iy0[XQ], ix0[XQ];
  bool rok[XQ];
#pragma unroll
  for (int j = 0; j < XQ; ++j) {
    const int m = m0 + srow + 32 * j;
    rok[j] = m < a.M;
    const int mm = rok[j] ? m : 0;
    const int b = mm / (a.Ho * a.Wo), rem = mm - b * (a.Ho * a.Wo), oy = rem / a.Wo, ox = rem - oy * a.Wo;
    xbase[j] = (long)b * a.H * a.W * a.Cin;
    iy0[j] = oy * a.stride - a.ph;
    ix0[j] = ox * a.stride - a.pw;
  }

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 32 * t + r;
    const float bv = (a.bias && n < a.Cout) ? a.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = bv;
  }

  f32x4 xr[XQ], wr[WQ];
  KPos p = {0, 0, 0};
  if constexpr (VEC) p = kpos(4 * kq, a.Cin, a.kw);
  auto load_chunk = [&](int k0) {
    const int k = k0 + 4 * kq;
#pragma unroll
    for (int j = 0; j < XQ; ++j) xr[j] = conv_load_x<VEC>(a, xbase[j], iy0[j], ix0[j], rok[j], k, p);
#pragma unroll
    for (int j = 0; j < WQ; ++j) wr[j] = conv_load_w<VEC>(a, n0 + srow + 32 * j, k);
    if constexpr (VEC) {  // the quad of the next chunk: 32 channels on, across taps where Cin is short
      p.ci += CV_BK;
      while (p.ci >= a.Cin) {
        p.ci -= a.Cin;
        if (++p.kx == a.kw) p.kx = 0, ++p.ky;
      }
    }
  };

  load_chunk(0);
  for (int k0 = 0; k0 < a.K; k0 += CV_BK) {
    __syncthreads();  // the chunk before has been read
#pragma unroll
    for (int j = 0; j < XQ; ++j) conv_put(xs + (srow + 32 * j) * CV_LD, kq, xr[j]);
#pragma unroll
    for (int j = 0; j < WQ; ++j) conv_put(wsm + (srow + 32 * j) * CV_LD, kq, wr[j]);
    __syncthreads();
    if (k0 + CV_BK < a.K) load_chunk(k0 + CV_BK);
    const float* xrow = xs + (32 * wv + r) * CV_LD + 4 * half;
    if constexpr (BLK) {
      f32x16 part[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) part[t][i] = 0.f;
#pragma unroll
      for (int g = 0; g < CV_BK / 8; ++g) {
        const f32x4 av = *(const f32x4*)(xrow + 8 * g);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 bv = *(const f32x4*)(wsm + (32 * t + r) * CV_LD + 4 * half + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) part[t] = mfma32(av[e], bv[e], part[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] += part[t];
    } else {
#pragma unroll
      for (int g = 0; g < CV_BK / 8; ++g) {
        const f32x4 av = *(const f32x4*)(xrow + 8 * g);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 bv = *(const f32x4*)(wsm + (32 * t + r) * CV_LD + 4 * half + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t] = mfma32(av[e], bv[e], acc[t]);
        }
      }
    }
  }

#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 32 * t + r;
    if (n >= a.Cout) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int m = m0 + 32 * wv + acc_row(i, half);
      if (m < a.M) {
        const float v = acc[t][i];
        a.y[(long)m * a.Ctot + a.c0 + n] = a.relu ? fmaxf(v, 0.f) : v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- pooling
// One thread per output pixel and 16-byte channel group.  mode 0: max; 1: average, the divisor counts the padding (9, what
// F.avg_pool2d does by default); 2: average over the taps inside the image.  Taps are visited in the order (ky, kx).
__global__ __launch_bounds__(256) void pool3x3_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C, int Ho,
                                                      int Wo, int stride, int pad, int mode, int c0, int Ctot, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = C / 4;
  const int c = (int)(idx % c4) * 4;
  const long pix = idx / c4;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
  const long b = pix / ((long)Wo * Ho);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * stride - pad + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * stride - pad + kx;
      if (ix < 0 || ix >= W) continue;
      const f32x4 v = *(const f32x4*)(x + ((b * H + iy) * W + ix) * C + c);
      if (mode == 0) {
        if (cnt == 0) s = v;
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = (v[e] > s[e] || v[e] != v[e]) ? v[e] : s[e];  // a NaN wins, as in F.max_pool2d
      } else {
        s += v;
      }
      ++cnt;
    }
  }
  if (mode == 1) s /= 9.f;
  if (mode == 2) s /= (float)cnt;
  *(f32x4*)(y + pix * Ctot + c0 + c) = s;
}

// [B, HW, C] -> [B, C]: one thread per (image, channel), the pixels in order, one division
__global__ __launch_bounds__(256) void global_avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, int HW, int C, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long b = idx / C;
  const int c = (int)(idx - b * C);
  const float* p = x + b * HW * C + c;
  float s = 0.f;
  for (int i = 0; i < HW; ++i) s += p[(long)i * C];
  y[idx] = s / (float)HW;
}

// ---------------------------------------------------------------------------------------------------------------- resize
// F.interpolate(mode='bilinear', align_corners=False): the source coordinate of output o is (o + 0.5) in / out - 0.5, clamped at 0
// = num / (2 out) with the integer num = max((2 o + 1) in - out, 0), so the cell and the weight are exact rationals.  The four
// products, their sum and the affine a v + b are taken in fp64 and rounded to fp32 once.  At in == out every weight is 1 or 0: the
// kernel is then the NCHW -> NHWC repack (with a = 1, b = 0 a copy).
struct Lerp {
  int i0, i1;
  double w1;
};
__device__ __forceinline__ Lerp lerp_of(int o, int in, int out) {
  long num = (long)(2 * o + 1) * in - out;
  if (num < 0) num = 0;
  const int i0 = (int)(num / (2 * out));
  return {i0, i0 + 1 < in ? i0 + 1 : in - 1, (double)(num - (long)i0 * 2 * out) / (double)(2 * out)};
}

// One thread per output pixel, the channels in a loop: neighbouring lanes read neighbouring columns of one NCHW plane and write
// C consecutive floats each.
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int H, int W,
                                                              int Ho, int Wo, float sa, float sb, long total) {
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= total) return;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
  const long b = pix / ((long)Wo * Ho);
  const Lerp ly = lerp_of(oy, H, Ho), lx = lerp_of(ox, W, Wo);
  for (int c = 0; c < C; ++c) {
    const float* p = x + (b * C + c) * (long)H * W;
    const double v00 = p[(long)ly.i0 * W + lx.i0], v01 = p[(long)ly.i0 * W + lx.i1];
    const double v10 = p[(long)ly.i1 * W + lx.i0], v11 = p[(long)ly.i1 * W + lx.i1];
    const double top = (1.0 - lx.w1) * v00 + lx.w1 * v01, bot = (1.0 - lx.w1) * v10 + lx.w1 * v11;
    const double v = (1.0 - ly.w1) * top + ly.w1 * bot;
    y[pix * C + c] = (float)((double)sa * v + (double)sb);
  }
}

// ---------------------------------------------------------------------------------------------------------------- statistics
// outer[i][j] = fma(x_r[i], x_r[j], outer[i][j]) and sum[i] += x_r[i] for r = 0 .. n - 1 in order, in fp64.  A workgroup owns a
// 64 x 64 block of `outer` (thread (ty, tx): rows ty + 16 a, columns tx + 16 b), the workgroups of the first block column also the
// 64 entries of `sum` beside it.  Up to 32 feature rows at a time are staged in LDS.  Since every element is updated by one
// thread in row order, feeding the rows in one call or in several leaves the same bits.
constexpr int FA_T = 64, FA_R = 32;
__global__ __launch_bounds__(256) void fid_accum_kernel(const float* __restrict__ f, int ldf, double* __restrict__ sum,
                                                        double* __restrict__ outer, int n, int D) {
  __shared__ float xi[FA_R][FA_T], xj[FA_R][FA_T];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * FA_T, j0 = blockIdx.x * FA_T;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      acc[a][b] = (i < D && j < D) ? outer[(long)i * D + j] : 0.0;
    }
  const bool own_sum = blockIdx.x == 0 && tid < FA_T && i0 + tid < D;
  double s = own_sum ? sum[i0 + tid] : 0.0;
  for (int r0 = 0; r0 < n; r0 += FA_R) {
    const int nr = n - r0 < FA_R ? n - r0 : FA_R;
    __syncthreads();
    for (int e = tid; e < nr * FA_T; e += 256) {
      const int rr = e / FA_T, cc = e % FA_T;
      const float* row = f + (long)(r0 + rr) * ldf;
      xi[rr][cc] = i0 + cc < D ? row[i0 + cc] : 0.f;
      xj[rr][cc] = j0 + cc < D ? row[j0 + cc] : 0.f;
    }
    __syncthreads();
    for (int rr = 0; rr < nr; ++rr) {
      double vi[4], vj[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) vi[a] = (double)xi[rr][ty + 16 * a], vj[a] = (double)xj[rr][tx + 16 * a];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fma(vi[a], vj[b], acc[a][b]);
      if (own_sum) s += (double)xi[rr][tid];
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i < D && j < D) outer[(long)i * D + j] = acc[a][b];
    }
  if (own_sum) sum[i0 + tid] = s;
}

}  // namespace vtp

using namespace vtp;

static const long INT_LIMIT = 2147483647L;

static int conv2d_f32(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, int kh, int kw,
                      int stride, int ph, int pw, int relu, int c0, int Ctot, bool blocked, void* stream) {
  VTP_REQUIRE(x && w && y, "vtp_conv2d_f32: null pointer (x, w, y)");
  VTP_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "vtp_conv2d_f32: bad shape (B, H, W, Cin, Cout >= 1)");
  VTP_REQUIRE((kh == 1 || kh == 3 || kh == 5 || kh == 7) && (kw == 1 || kw == 3 || kw == 5 || kw == 7),
              "vtp_conv2d_f32: kh, kw must be 1, 3, 5 or 7");
  VTP_REQUIRE(stride == 1 || stride == 2, "vtp_conv2d_f32: stride must be 1 or 2");
  VTP_REQUIRE(ph >= 0 && ph < kh && pw >= 0 && pw < kw, "vtp_conv2d_f32: bad padding (0 <= ph < kh, 0 <= pw < kw)");
  VTP_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "vtp_conv2d_f32: the image is smaller than the filter");
  VTP_REQUIRE(c0 >= 0 && Ctot >= 1 && (long)c0 + Cout <= Ctot, "vtp_conv2d_f32: the channel slice [c0, c0 + Cout) must lie inside Ctot");
  const int Ho = (H + 2 * ph - kh) / stride + 1, Wo = (W + 2 * pw - kw) / stride + 1;
  const long M = (long)B * Ho * Wo, K = (long)kh * kw * Cin;
  VTP_REQUIRE(M <= INT_LIMIT - CV_BM && K <= INT_LIMIT - CV_BK && (long)B * H * W <= INT_LIMIT,
              "vtp_conv2d_f32: B Ho Wo, B H W and kh kw Cin must fit 31 bits");
  const bool vec = Cin % 4 == 0;
  VTP_REQUIRE(!vec || (aligned16(x) && aligned16(w)), "vtp_conv2d_f32: x and w must be 16-byte aligned when Cin %% 4 == 0");
  VTP_REQUIRE(cdiv(Cout, 32) <= 65535, "vtp_conv2d_f32: Cout too large");
  ConvArgs a{x, w, bias, y, H, W, Cin, Cout, kh, kw, stride, ph, pw, Ho, Wo, (int)M, (int)K, relu ? 1 : 0, c0, Ctot};
  const int nt32 = cdiv(Cout, 32);
  const bool two = nt32 % 2 == 0;  // an odd count of 32-column tiles runs one tile per wave: no half-empty workgroup column
  const dim3 grid(cdiv(M, CV_BM), two ? nt32 / 2 : nt32);
  hipStream_t s = (hipStream_t)stream;
#define VTP_CONV(NT, VEC)                                                                                                \
  do {                                                                                                                    \
    if (blocked) hipLaunchKernelGGL((conv2d_f32_kernel<NT, VEC, true>), grid, dim3(CV_THREADS), 0, s, a);                  \
    else hipLaunchKernelGGL((conv2d_f32_kernel<NT, VEC, false>), grid, dim3(CV_THREADS), 0, s, a);                         \
  } while (0)
  if (two && vec) VTP_CONV(2, true);
  else if (two) VTP_CONV(2, false);
  else if (vec) VTP_CONV(1, true);
  else VTP_CONV(1, false);
#undef VTP_CONV
  return check_launch("conv2d_f32");
}

extern "C" int vtp_conv2d_f32(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, int kh,
                              int kw, int stride, int ph, int pw, int relu, int c0, int Ctot, void* stream) {
  return conv2d_f32(x, w, bias, y, B, H, W, Cin, Cout, kh, kw, stride, ph, pw, relu, c0, Ctot, false, stream);
}

extern "C" int vtp_conv2d_f32_blocked(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout,
                                      int kh, int kw, int stride, int ph, int pw, int relu, int c0, int Ctot, void* stream) {
  return conv2d_f32(x, w, bias, y, B, H, W, Cin, Cout, kh, kw, stride, ph, pw, relu, c0, Ctot, true, stream);
}

extern "C" int vtp_pool3x3_f32(const float* x, float* y, int B, int H, int W, int C, int stride, int mode, int c0, int Ctot, void* stream) {
  VTP_REQUIRE(x && y, "vtp_pool3x3_f32: null pointer");
  VTP_REQUIRE(B >= 1 && C >= 4 && C % 4 == 0, "vtp_pool3x3_f32: bad shape (B >= 1, C %% 4 == 0)");
  VTP_REQUIRE(stride == 1 || stride == 2, "vtp_pool3x3_f32: stride 1 (pad 1) or stride 2 (pad 0)");
  VTP_REQUIRE(mode >= 0 && mode <= 2, "vtp_pool3x3_f32: mode 0 (max), 1 (average over 9), 2 (average over the taps inside)");
  VTP_REQUIRE(H >= (stride == 2 ? 3 : 1) && W >= (stride == 2 ? 3 : 1), "vtp_pool3x3_f32: the image is smaller than the window");
  VTP_REQUIRE(c0 >= 0 && c0 % 4 == 0 && Ctot % 4 == 0 && (long)c0 + C <= Ctot,
              "vtp_pool3x3_f32: the channel slice [c0, c0 + C) must lie inside Ctot, c0 %% 4 == 0, Ctot %% 4 == 0");
  VTP_REQUIRE(aligned16(x) && aligned16(y), "vtp_pool3x3_f32: x and y must be 16-byte aligned");
  const int pad = stride == 1 ? 1 : 0;
  const int Ho = (H + 2 * pad - 3) / stride + 1, Wo = (W + 2 * pad - 3) / stride + 1;
  const long total = (long)B * Ho * Wo * (C / 4);
  VTP_REQUIRE((long)B * H * W <= INT_LIMIT && total / 256 < INT_LIMIT, "vtp_pool3x3_f32: too large");
  hipLaunchKernelGGL(pool3x3_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, C, Ho, Wo, stride, pad, mode, c0,
                     Ctot, total);
  return check_launch("pool3x3_f32");
}

extern "C" int vtp_global_avgpool_f32(const float* x, float* y, int B, int HW, int C, void* stream) {
  VTP_REQUIRE(x && y, "vtp_global_avgpool_f32: null pointer");
  VTP_REQUIRE(B >= 1 && HW >= 1 && C >= 1, "vtp_global_avgpool_f32: bad shape (B, HW, C >= 1)");
  const long total = (long)B * C;
  VTP_REQUIRE(total / 256 < INT_LIMIT, "vtp_global_avgpool_f32: too large");
  hipLaunchKernelGGL(global_avgpool_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, HW, C, total);
  return check_launch("global_avgpool_f32");
}

extern "C" int vtp_resize_bilinear_nhwc(const float* x, float* y, int B, int C, int H, int W, int Ho, int Wo, float scale, float shift,
                                        void* stream) {
  VTP_REQUIRE(x && y, "vtp_resize_bilinear_nhwc: null pointer");
  VTP_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "vtp_resize_bilinear_nhwc: bad shape (all >= 1)");
  VTP_REQUIRE(H <= (1 << 20) && W <= (1 << 20) && Ho <= (1 << 20) && Wo <= (1 << 20), "vtp_resize_bilinear_nhwc: sides up to 2^20");
  const long total = (long)B * Ho * Wo;  // output pixels, one thread each
  VTP_REQUIRE(total / 256 < INT_LIMIT, "vtp_resize_bilinear_nhwc: too large");
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, C, H, W, Ho, Wo, scale, shift,
                     total);
  return check_launch("resize_bilinear_nhwc");
}

extern "C" int vtp_fid_accum(const float* feats, int ldf, double* sum, double* outer, int n, int D, void* stream) {
  VTP_REQUIRE(feats && sum && outer, "vtp_fid_accum: null pointer");
  VTP_REQUIRE(n >= 1 && D >= 1 && ldf >= D, "vtp_fid_accum: bad shape (n, D >= 1, ldf >= D)");
  VTP_REQUIRE(cdiv(D, FA_T) <= 65535, "vtp_fid_accum: D too large");
  const int t = cdiv(D, FA_T);
  hipLaunchKernelGGL(fid_accum_kernel, dim3(t, t), dim3(256), 0, (hipStream_t)stream, feats, ldf, sum, outer, n, D);
  return check_launch("fid_accum");
}
