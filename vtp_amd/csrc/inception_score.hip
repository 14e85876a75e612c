// Inception Score (Salimans et al. 2016; the figure the ADM evaluation suite reports beside FID), restated from the papers'
// definition: with p_i = softmax(logits_i), rows cut in order into splits of split_size rows,
//   KL_s = (1 / n_s) sum_i sum_c p_ic (log p_ic - log m_c),  m_c = (1 / n_s) sum_i p_ic,   IS = mean_s exp(KL_s).
// As sums that can be accumulated update by update:  H_s = sum_i h_i with h_i = sum_c p_ic (l_ic - lse_i),  S_sc = sum_i p_ic,
//   KL_s = (H_s - sum_c S_sc log(S_sc / n_s)) / n_s  (the host: vtp_amd/inception_score.py).
//   vtp_is_rows  : per row of fp32 logits the softmax p and the entropy term h, in fp64
//   vtp_is_accum : adds the rows' (h | p) to the slots [H_s | S_s0 .. S_s,C-1] of their splits, rows in order, every element owned by
//                  one thread
// No float atomics, no split sums, no host synchronisation: every result repeats bit for bit.
//
// Arithmetic of a row (is_rows_kernel), in fp64 from the fp32 logits.  m = max_c l_c and j = the first column that attains it;
//   d_c = l_c - m is exact (two fp32 values); z = sum_{c != j} exp(d_c), so that Z = sum_c exp(d_c) = 1 + z and
//   log Z = log1p(z): a row that is all but certain of one class (z ~ 1e-35) keeps log Z, which log(1 + z) would round to 0 and
//   with it the largest term of h.  p_c = exp(d_c) / Z (column j: exactly 1 / Z) and l_c - lse = d_c - log Z.  p_c is formed as a
//   quotient and not as exp(d_c - log Z): the rounding of that difference is an ABSOLUTE error of the exponent, up to 2^-53 |d_c|,
//   and so a relative error of p_c that grows with the spread of the row (700 u at the edge of the fp64 range) where the quotient
//   stays at a few u plus the C adds of z.  h = sum_c p_c (d_c - log Z): a p_c that underflowed to 0 contributes 0 x finite = 0.
// One wave per row: lanes stride over c, IS_U columns of a lane in flight (fp64 exp is some forty dependent instructions), the
//   lane sums added in column order and folded by a fixed xor butterfly: the bits of a row depend on that row alone.
#include "common.h"
#include "vtp_hip.h"

#include <limits.h>
#include <math.h>

namespace vtp {

constexpr int IS_WAVES = 4;  // rows per workgroup of is_rows_kernel
constexpr int IS_U = 4;      // columns of a lane in flight
constexpr int IS_R = 8;      // rows of an element in flight in is_accum_kernel

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64 * IS_WAVES) void is_rows_kernel(const float* __restrict__ logits, int ldl, int B, int C,
                                                                 double* __restrict__ p, int ldp, double* __restrict__ h) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * IS_WAVES + (threadIdx.x >> 6);
  if (row >= B) return;  // a whole wave: nothing below synchronises the workgroup
  const float* l = logits + (size_t)row * ldl;
  double* pr = p + (size_t)row * ldp;

  // the maximum and the first column that holds it: a lane keeps its first (strict >), the butterfly the smaller index of a tie
  float m = -INFINITY;
  int jm = INT_MAX;
  for (int c = lane; c < C; c += 64) {
    const float v = l[c];
    if (v > m) m = v, jm = c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oj = __shfl_xor(jm, o, 64);
    if (om > m || (om == m && oj < jm)) m = om, jm = oj;
  }
  const double md = (double)m;

  double z = 0.0;
  for (int c0 = lane; c0 < C; c0 += 64 * IS_U) {
    double e[IS_U];
#pragma unroll
    for (int u = 0; u < IS_U; ++u) {
      const int c = c0 + 64 * u;
      e[u] = (c < C && c != jm) ? exp((double)l[c] - md) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < IS_U; ++u) z += e[u];
  }
  z = wave_sum_f64(z);
  const double Z = 1.0 + z, logZ = log1p(z);

  double hs = 0.0;
  for (int c0 = lane; c0 < C; c0 += 64 * IS_U) {
    double t[IS_U];
#pragma unroll
    for (int u = 0; u < IS_U; ++u) {
      const int c = c0 + 64 * u;
      t[u] = 0.0;
      if (c < C) {
        const double d = (double)l[c] - md;
        const double pc = exp(d) / Z;
        pr[c] = pc;
        t[u] = pc * (d - logZ);
      }
    }
#pragma unroll
    for (int u = 0; u < IS_U; ++u) hs += t[u];
  }
  hs = wave_sum_f64(hs);
  if (lane == 0) h[row] = hs;
}

// Thread e of a slot's workgroups owns element e of the slot (0: H, 1 + c: S_c) and adds the update's rows that fall into the
// slot in ascending order, IS_R loads in flight: the scheme of fid_accum_kernel.  blockIdx.y counts the slots the update touches.
__global__ __launch_bounds__(256) void is_accum_kernel(const double* __restrict__ p, int ldp, const double* __restrict__ h, long row_base,
                                                        long split_size, int B, int C, double* __restrict__ state) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e > C) return;
  const long slot = row_base / split_size + blockIdx.y;
  const long first = slot * split_size;  // global row the slot starts at: <= row_base + B - 1
  const long lo = first > row_base ? first - row_base : 0;
  const long room = split_size - (row_base + lo - first);  // rows of the slot from row lo on
  const long hi = room < B - lo ? lo + room : B;
  const double* src = e == 0 ? h : p + (e - 1);
  const long stride = e == 0 ? 1 : ldp;
  double* dst = state + slot * (1 + (long)C) + e;
  double acc = *dst;
  for (long i = lo; i < hi; i += IS_R) {
    double v[IS_R];
#pragma unroll
    for (int u = 0; u < IS_R; ++u) v[u] = i + u < hi ? src[(i + u) * stride] : 0.0;
#pragma unroll
    for (int u = 0; u < IS_R; ++u)
      if (i + u < hi) acc += v[u];
  }
  *dst = acc;
}

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_is_rows(const float* logits, int ldl, int B, int C, double* p, int ldp, double* h, void* stream) {
  VTP_REQUIRE(logits && p && h, "vtp_is_rows: null pointer (logits, p, h)");
  VTP_REQUIRE(B >= 1 && C >= 1, "vtp_is_rows: need B, C >= 1 (B=%d C=%d)", B, C);
  VTP_REQUIRE(ldl >= C && ldp >= C, "vtp_is_rows: the leading dimensions must cover the rows (ldl=%d ldp=%d C=%d)", ldl, ldp, C);
  hipLaunchKernelGGL(is_rows_kernel, dim3(cdiv(B, IS_WAVES)), dim3(64 * IS_WAVES), 0, (hipStream_t)stream, logits, ldl, B, C, p, ldp, h);
  return check_launch("is_rows");
}

extern "C" int vtp_is_accum(const double* p, int ldp, const double* h, long row_base, long split_size, int B, int C, double* state,
                            int n_slots, void* stream) {
  VTP_REQUIRE(p && h && state, "vtp_is_accum: null pointer (p, h, state)");
  VTP_REQUIRE(B >= 1 && C >= 1 && ldp >= C, "vtp_is_accum: need B, C >= 1 and ldp >= C (B=%d C=%d ldp=%d)", B, C, ldp);
  VTP_REQUIRE(split_size >= 1, "vtp_is_accum: split_size must be positive (split_size=%ld)", split_size);
  VTP_REQUIRE(row_base >= 0 && row_base <= LONG_MAX - B, "vtp_is_accum: row_base must be a row index (row_base=%ld)", row_base);
  const long s_lo = row_base / split_size, s_hi = (row_base + B - 1) / split_size;
  VTP_REQUIRE(n_slots >= 1 && s_hi < n_slots, "vtp_is_accum: the rows reach slot %ld, the state holds n_slots=%d", s_hi, n_slots);
  VTP_REQUIRE(s_hi - s_lo < 65535, "vtp_is_accum: one update may touch at most 65535 slots (split_size=%ld B=%d)", split_size, B);
  hipLaunchKernelGGL(is_accum_kernel, dim3(cdiv(1 + (long)C, 256), (unsigned)(s_hi - s_lo + 1)), dim3(256), 0, (hipStream_t)stream, p, ldp,
                     h, row_base, split_size, B, C, state);
  return check_launch("is_accum");
}
