// LPIPS in exact fp32 for evaluation (reference: vtp/utils/lpips.py:61-175 called outside autocast, as
// tools/test_reconstruction_hf.py:344,378-383 does).  The 13 VGG16 convolutions are vtp_conv2d_f32_blocked (fid.hip); here are the pieces
// around them, all on f32 NHWC activations WITHOUT borders:
//   vtp_lpips_scale_nhwc_f32 : ScalingLayer + NCHW -> NHWC repack, optionally with a fourth zero channel
//   vtp_maxpool2_f32         : nn.MaxPool2d(2, 2)
//   vtp_lpips_head_f32       : normalize_tensor, difference, NetLinLayer of one tap; fp64 sums over fixed 256-pixel segments
//   vtp_lpips_finalize_f32   : segment sums -> spatial averages -> val = (((r0 + r1) + r2) + r3) + r4
// No float atomics and no split that depends on the grid or the batch: an image pair's value is the same bits whatever it is
// batched with, and repeats from run to run.
#include "common.h"
#include "vtp_hip.h"

namespace vtp {

// ---------------------------------------------------------------------------------------------------------------- ScalingLayer
// One thread per pixel: three coalesced plane reads, y_c = (x_c - shift_c) / scale_c with an IEEE division (what torch computes;
// a product with 1 / scale_c rounds differently), one 16-byte store (Co = 4, channel 3 = 0) or three 4-byte stores (Co = 3).
template <int Co>
__global__ __launch_bounds__(256) void lpips_scale_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, long HW, long total,
                                                               float sh0, float sh1, float sh2, float sc0, float sc1, float sc2) {
  const long pix = blockIdx.x * 256L + threadIdx.x;
  if (pix >= total) return;
  const long b = pix / HW, r = pix - b * HW;
  const float* p = x + b * 3 * HW + r;
  const float v0 = (p[0] - sh0) / sc0, v1 = (p[HW] - sh1) / sc1, v2 = (p[2 * HW] - sh2) / sc2;
  if constexpr (Co == 4) {
    *(f32x4*)(y + pix * 4) = f32x4{v0, v1, v2, 0.f};
  } else {
    y[pix * 3] = v0;
    y[pix * 3 + 1] = v1;
    y[pix * 3 + 2] = v2;
  }
}

// ---------------------------------------------------------------------------------------------------------------- 2x2 max-pool
// One thread per output pixel and 16-byte channel group.  The window is visited in row-major order and a later tap replaces the
// maximum only when it is greater or NaN: ATen's max_pool2d.
__global__ __launch_bounds__(256) void maxpool2_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C,
                                                           long total) {
  const long idx = blockIdx.x * 256L + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H >> 1, Wo = W >> 1, c4 = C >> 2;
  const int c = (int)(idx % c4) * 4;
  const long pix = idx / c4;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
  const long b = pix / ((long)Wo * Ho);
  const float* p = x + ((b * H + 2 * oy) * W + 2 * ox) * C + c;
  f32x4 s = *(const f32x4*)p;
  const f32x4 t[3] = {*(const f32x4*)(p + C), *(const f32x4*)(p + (long)W * C), *(const f32x4*)(p + (long)W * C + C)};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = (t[i][e] > s[e] || t[i][e] != t[i][e]) ? t[i][e] : s[e];
  *(f32x4*)(y + pix * C + c) = s;
}

// ---------------------------------------------------------------------------------------------------------------- head of one tap
// f f32 [2 n, HW, C]: the ReLU features of image b and of image n + b.  Per pixel, in fp32 as lpips.py:169-171, 90-94 write it:
//   n0 = sqrt(sum_c f0_c^2),  a_c = f0_c / (n0 + 1e-10);  the same for f1 giving b_c;  s = sum_c w_c (a_c - b_c)^2
// (an all-zero pixel gives a = 0 / 1e-10 = 0).  LPP = min(C / 4, 64) lanes share a pixel, each holding V = C / (4 LPP) 16-byte
// quads; the channel sums are xor butterflies over those lanes, so every lane of the group ends with the same bits.
// Work split: workgroup (seg, b) owns the pixels [256 seg, 256 seg + 256) of pair b; in round t, lane group g of wave w takes pixel
// 256 seg + (4 t + w) PPW + g.  Every group adds its s values to an fp64 sum in round order; a wave adds its groups' sums in
// group order, thread 0 the four waves' in wave order: part[b * nseg + seg].  All of it is a function of the pixel index alone.
constexpr int HEAD_SEG = 256;

template <int LPP, int V>
__global__ __launch_bounds__(256) void lpips_head_f32_kernel(const float* __restrict__ f, const float* __restrict__ w,
                                                             double* __restrict__ part, int n, int HW) {
  constexpr int C = 4 * LPP * V, PPW = 64 / LPP;
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane % LPP, grp = lane / LPP;
  const int seg = blockIdx.x, b = blockIdx.y;
  f32x4 ww[V];
#pragma unroll
  for (int v = 0; v < V; ++v) ww[v] = *(const f32x4*)(w + 4 * (sub + LPP * v));
  const float* f0 = f + (long)b * HW * C;
  const float* f1 = f + (long)(n + b) * HW * C;
  double acc = 0.0;
  for (int t = 0; t < HEAD_SEG / (4 * PPW); ++t) {
    const int pix = seg * HEAD_SEG + (4 * t + wv) * PPW + grp;
    const bool ok = pix < HW;  // past the image: pixel 0 is read and replaced by zero features, s = +0
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 a[V], c[V];
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const long off = (long)(ok ? pix : 0) * C + 4 * (sub + LPP * v);
      a[v] = ok ? *(const f32x4*)(f0 + off) : zero;
      c[v] = ok ? *(const f32x4*)(f1 + off) : zero;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s0 = fmaf(a[v][e], a[v][e], s0);
        s1 = fmaf(c[v][e], c[v][e], s1);
      }
    }
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) {
      s0 += __shfl_xor(s0, o, 64);
      s1 += __shfl_xor(s1, o, 64);
    }
    const float d0 = sqrtf(s0) + 1e-10f, d1 = sqrtf(s1) + 1e-10f;
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float df = a[v][e] / d0 - c[v][e] / d1;
        s = fmaf(ww[v][e], df * df, s);
      }
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) s += __shfl_xor(s, o, 64);
    acc += (double)s;
  }
  double tot = 0.0;
#pragma unroll
  for (int g = 0; g < PPW; ++g) tot += __shfl(acc, g * LPP, 64);
  if (lane == 0) red[wv] = tot;
  __syncthreads();
  if (threadIdx.x == 0) part[(long)b * gridDim.x + seg] = ((red[0] + red[1]) + red[2]) + red[3];
}

// part f64 [5 taps][n][nseg_k] (tap k at offset n * sum_{j<k} nseg_j, nseg_k = ceil(HW_k / 256), HW_k = (H >> k) (W >> k)).
// One wave per pair: lane l adds the segments l, l + 64, ... of a tap in order, an xor butterfly adds the lanes (the same tree for
// every pair: the segment count is a function of H and W), r_k = float(S_k / HW_k), val = (((r0 + r1) + r2) + r3) + r4 in fp32.
__global__ __launch_bounds__(64) void lpips_finalize_f32_kernel(const double* __restrict__ part, float* __restrict__ val, int n, int H,
                                                                int W) {
  const int lane = threadIdx.x, b = blockIdx.x;
  long off = 0;
  float v = 0.f;
  for (int k = 0; k < 5; ++k) {
    const long hw = (long)(H >> k) * (W >> k);
    const int nseg = (int)((hw + HEAD_SEG - 1) / HEAD_SEG);
    const double* p = part + off + (long)b * nseg;
    double s = 0.0;
    for (int i = lane; i < nseg; i += 64) s += p[i];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    const float r = (float)(s / (double)hw);
    v = k == 0 ? r : v + r;
    off += (long)n * nseg;
  }
  if (lane == 0) val[b] = v;
}

}  // namespace vtp

using namespace vtp;

static const long INT_LIMIT = 2147483647L;

extern "C" int vtp_lpips_scale_nhwc_f32(const float* x, float* y, int B, int H, int W, int Cout, const float* shift, const float* scale,
                                        void* stream) {
  VTP_REQUIRE(x && y && shift && scale, "vtp_lpips_scale_nhwc_f32: null pointer");
  VTP_REQUIRE(B >= 1 && H >= 1 && W >= 1, "vtp_lpips_scale_nhwc_f32: bad shape (B, H, W >= 1)");
  VTP_REQUIRE(Cout == 3 || Cout == 4, "vtp_lpips_scale_nhwc_f32: Cout must be 3, or 4 (a fourth channel of zeros)");
  VTP_REQUIRE(Cout == 3 || aligned16(y), "vtp_lpips_scale_nhwc_f32: y must be 16-byte aligned when Cout == 4");
  const long HW = (long)H * W, total = (long)B * HW;
  VTP_REQUIRE(total <= INT_LIMIT, "vtp_lpips_scale_nhwc_f32: B H W must fit 31 bits");
  const dim3 grid(cdiv(total, 256));
  hipStream_t s = (hipStream_t)stream;
  if (Cout == 4)
    hipLaunchKernelGGL(lpips_scale_nhwc_kernel<4>, grid, dim3(256), 0, s, x, y, HW, total, shift[0], shift[1], shift[2], scale[0], scale[1],
                       scale[2]);
  else
    hipLaunchKernelGGL(lpips_scale_nhwc_kernel<3>, grid, dim3(256), 0, s, x, y, HW, total, shift[0], shift[1], shift[2], scale[0], scale[1],
                       scale[2]);
  return check_launch("lpips_scale_nhwc_f32");
}

extern "C" int vtp_maxpool2_f32(const float* x, float* y, int B, int H, int W, int C, void* stream) {
  VTP_REQUIRE(x && y, "vtp_maxpool2_f32: null pointer");
  VTP_REQUIRE(B >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "vtp_maxpool2_f32: bad shape (B >= 1; H, W even and >= 2)");
  VTP_REQUIRE(C >= 4 && C % 4 == 0, "vtp_maxpool2_f32: C must be a multiple of 4");
  VTP_REQUIRE(aligned16(x) && aligned16(y), "vtp_maxpool2_f32: x and y must be 16-byte aligned");
  const long total = (long)B * (H / 2) * (W / 2) * (C / 4);
  VTP_REQUIRE((long)B * H * W <= INT_LIMIT && total / 256 < INT_LIMIT, "vtp_maxpool2_f32: too large");
  hipLaunchKernelGGL(maxpool2_f32_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, C, total);
  return check_launch("maxpool2_f32");
}

extern "C" int vtp_lpips_head_f32(const float* f, const float* w, double* part, int n, int HW, int C, void* stream) {
  VTP_REQUIRE(f && w && part, "vtp_lpips_head_f32: null pointer");
  VTP_REQUIRE(n >= 1 && n <= 65535 && HW >= 1, "vtp_lpips_head_f32: bad shape (1 <= n <= 65535, HW >= 1)");
  VTP_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512, "vtp_lpips_head_f32: C must be 64, 128, 256 or 512 (VGG16 taps)");
  VTP_REQUIRE(aligned16(f) && aligned16(w), "vtp_lpips_head_f32: f and w must be 16-byte aligned");
  VTP_REQUIRE(2L * n * HW <= INT_LIMIT, "vtp_lpips_head_f32: 2 n HW must fit 31 bits");
  const dim3 grid(cdiv(HW, HEAD_SEG), n);
  hipStream_t s = (hipStream_t)stream;
#define VTP_HEAD(L, V) hipLaunchKernelGGL((lpips_head_f32_kernel<L, V>), grid, dim3(256), 0, s, f, w, part, n, HW)
  switch (C) {
    case 64: VTP_HEAD(16, 1); break;
    case 128: VTP_HEAD(32, 1); break;
    case 256: VTP_HEAD(64, 1); break;
    default: VTP_HEAD(64, 2); break;
  }
#undef VTP_HEAD
  return check_launch("lpips_head_f32");
}

extern "C" int vtp_lpips_finalize_f32(const double* part, float* val, int n, int H, int W, void* stream) {
  VTP_REQUIRE(part && val, "vtp_lpips_finalize_f32: null pointer");
  VTP_REQUIRE(n >= 1 && H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0,
              "vtp_lpips_finalize_f32: bad shape (n >= 1; H, W multiples of 16)");
  hipLaunchKernelGGL(lpips_finalize_f32_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, part, val, n, H, W);
  return check_launch("lpips_finalize_f32");
}
