// Global gradient-norm clipping of the training step (torch.nn.utils.clip_grad_norm_, norm_type 2) without float atomics: every
// workgroup of the partials kernel stores ONE fp64 sum of squares of its chunk, and one workgroup adds the partials in a fixed tree
// order (the store-and-sum form).  The result depends on the gradient values and the partials layout only -- not on the CU count, the
// dispatch order or the timing -- so eager steps, graph replays and data-parallel ranks that see the same gradients agree bit for bit.
#include "common.h"
#include "vtp_hip.h"

namespace vtp {

constexpr int GN_THREADS = 256;
constexpr int GN_UNROLL = 8;                                      // float4 loads per thread, all issued before the first use
constexpr long GN_CHUNK = (long)GN_THREADS * GN_UNROLL * 4;       // elements per workgroup = per partial (8192)
constexpr int GN_FIN_THREADS = 1024;
constexpr int GN_FIN_UNROLL = 8;

// partials[blockIdx.x] = sum of g[i]^2 over the block's chunk, in fp64 (the square of an fp32 value is exact in fp64).  Short-lived
// blocks like adamw_ema_kernel: this runs on the optimizer lane beside the persistent GEMMs, so a block takes a free CU slot for one
// round of loads and gives it back (no grid-stride loop).
__global__ __launch_bounds__(GN_THREADS) void sumsq_partials_kernel(const float* __restrict__ g, long n4, double* __restrict__ partials) {
  const long base = blockIdx.x * (GN_CHUNK / 4) + threadIdx.x;
  f32x4 gv[GN_UNROLL];
#pragma unroll
  for (int u = 0; u < GN_UNROLL; ++u) {
    const long i = base + (long)u * GN_THREADS;
    gv[u] = i < n4 ? *(const f32x4*)(g + 4 * i) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < GN_UNROLL; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) s = fma((double)gv[u][e], (double)gv[u][e], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ double ws[GN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) ws[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// b^t by plain fp64 multiplications (square and multiply): exact wherever the power is representable
__device__ __forceinline__ double pow_by_squaring(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

// One workgroup: sum = partials[0, count) added in a fixed order (thread t: t, t + 1024, ... in sequence; then an LDS tree).
// hyper == nullptr: *sum_out = sum.  Otherwise the clip_grad_norm_ tail, with gs = hyper[7] (the gradient multiplier AdamW applies)
// and max_norm = hyper[10]:  total_norm = gs * sqrt(sum);  coef = clamp(max_norm / (total_norm + 1e-6), max=1);  hyper[7] = gs * coef.
// state != nullptr (VTPTrainer(skip_nonfinite=True)): the guarded tail.  state = int32 {applied_steps, skipped_steps, skip_now, pad}.
// skip = !isfinite(total_norm), tested on the REPORTED f32 norm (a finite fp64 sum whose scaled root overflows f32 skips too; a NaN
// or inf gradient element reaches the sum through the fp64 fma chain of sumsq_partials_kernel, and squares cannot cancel).  A skipped
// step leaves hyper[7] alone and counts in skipped_steps; an applied one folds coef in and counts in applied_steps.  Adam's step count
// is the DEVICE counter: hyper[5] = 1 - b1^t and hyper[6] = sqrt(1 - b2^t) with t = applied_steps after the increment (applied_steps
// + 1 on a skipped step: unused), in fp64 with the power by squaring (exact wherever b^t is representable).  One thread, plain stores.
__global__ __launch_bounds__(GN_FIN_THREADS) void sum_partials_kernel(const double* __restrict__ partials, int count,
                                                                      double* __restrict__ sum_out, float* __restrict__ hyper,
                                                                      float* __restrict__ norm_out, float* __restrict__ coef_out,
                                                                      int* __restrict__ state, double b1, double b2) {
  __shared__ double sh[GN_FIN_THREADS];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i0 = t; i0 < count; i0 += GN_FIN_THREADS * GN_FIN_UNROLL) {
    double v[GN_FIN_UNROLL];
#pragma unroll
    for (int u = 0; u < GN_FIN_UNROLL; ++u) {
      const int i = i0 + u * GN_FIN_THREADS;
      v[u] = i < count ? partials[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < GN_FIN_UNROLL; ++u) s += v[u];
  }
  sh[t] = s;
  __syncthreads();
#pragma unroll
  for (int w = GN_FIN_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  if (t != 0) return;
  const double sum = sh[0];
  if (!hyper) {
    *sum_out = sum;
    return;
  }
  const float gs = hyper[7], max_norm = hyper[10];
  const float total = (float)((double)gs * sqrt(sum));
  const float c = max_norm / (total + 1e-6f);
  const float coef = c > 1.f ? 1.f : c;  // torch.clamp(max=1): NaN stays NaN (fminf(NaN, 1) would return 1)
  norm_out[0] = total;
  coef_out[0] = coef;
  if (!state) {
    hyper[7] = gs * coef;
    return;
  }
  const bool skip = (__float_as_uint(total) & 0x7f800000u) == 0x7f800000u;  // inf or NaN
  int applied = state[0];
  if (skip) {
    state[1] += 1;
  } else {
    hyper[7] = gs * coef;
    state[0] = ++applied;
  }
  state[2] = skip ? 1 : 0;
  const int adam_t = skip ? applied + 1 : applied;
  hyper[5] = (float)(1.0 - pow_by_squaring(b1, adam_t));
  hyper[6] = (float)sqrt(1.0 - pow_by_squaring(b2, adam_t));
}

}  // namespace vtp
using namespace vtp;

extern "C" int vtp_sumsq_partials_count(long n) { return n > 0 ? (int)((n + GN_CHUNK - 1) / GN_CHUNK) : 0; }

extern "C" int vtp_sumsq_partials(const float* g, long n, double* partials, void* stream) {
  VTP_REQUIRE(g && partials && n > 0 && n % 4 == 0, "vtp_sumsq_partials: bad argument (n > 0, n %% 4 == 0)");
  VTP_REQUIRE(n / GN_CHUNK < 0x7fffffffL, "vtp_sumsq_partials: range too long for one launch");
  hipLaunchKernelGGL(sumsq_partials_kernel, dim3((unsigned)vtp_sumsq_partials_count(n)), dim3(GN_THREADS), 0, (hipStream_t)stream, g,
                     n / 4, partials);
  return check_launch("sumsq_partials");
}

extern "C" int vtp_sum_partials(const double* partials, int count, double* sum, void* stream) {
  VTP_REQUIRE(partials && sum && count >= 1, "vtp_sum_partials: bad argument (count >= 1)");
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(GN_FIN_THREADS), 0, (hipStream_t)stream, partials, count, sum,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, (int*)nullptr, 0.0, 0.0);
  return check_launch("sum_partials");
}

extern "C" int vtp_grad_clip_finalize(const double* partials, int count, float* hyper, float* total_norm, float* coef, void* stream) {
  VTP_REQUIRE(partials && hyper && total_norm && coef && count >= 1, "vtp_grad_clip_finalize: bad argument (count >= 1)");
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(GN_FIN_THREADS), 0, (hipStream_t)stream, partials, count, (double*)nullptr,
                     hyper, total_norm, coef, (int*)nullptr, 0.0, 0.0);
  return check_launch("grad_clip_finalize");
}

extern "C" int vtp_grad_clip_finalize_guarded(const double* partials, int count, float* hyper, float* total_norm, float* coef,
                                              int* state, const double* betas, void* stream) {
  VTP_REQUIRE(partials && hyper && total_norm && coef && state && betas && count >= 1,
              "vtp_grad_clip_finalize_guarded: bad argument (count >= 1)");
  const double b1 = betas[0], b2 = betas[1];  // HOST memory: read here, passed as launch arguments
  VTP_REQUIRE(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, "vtp_grad_clip_finalize_guarded: betas must lie in [0, 1)");
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(GN_FIN_THREADS), 0, (hipStream_t)stream, partials, count, (double*)nullptr,
                     hyper, total_norm, coef, state, b1, b2);
  return check_launch("grad_clip_finalize_guarded");
}
