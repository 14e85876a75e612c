// The one-wave exact-fp32 tiles on v_mfma_f32_32x32x2_f32 that read their operands straight from memory (no LDS, no barrier), written
// once: the row-major k unit of probe_logits_kernel (probe.hip) and zs_tile (zeroshot.hip), the transposed 64 x 64 tile dW = G^T X of
// probe_sgd_kernel (probe.hip) and seg_wgrad_kernel (segprobe.hip), and the SGD-momentum step behind it.  Device-inline functions
// only: the kernels, their loops around a unit and their prefetch depths (measured per kernel) stay in their own files.
#pragma once
#include "common.h"
#include "mfma_f32.h"

namespace vtp {

// ---------------------------------------------------------------------------------------------------------------- the k unit
// A unit is 32 wide in k.  The lane (r = l & 31, half h = l >> 5) holds one row of W (the B operand) and ROWS rows of X (the A
// operands of ROWS independent 32 x 32 accumulators).  Per 8-wide chunk c the lane half h loads the 16 bytes at k0 + 8 c + 4 h of its
// rows, and element e of both operands feeds MFMA (c, e), whose two k values are (k0 + 8 c + e, k0 + 8 c + 4 + e).  A and B use the
// same (h, e) -> k map, so the product only permutes the order of the sum; the chain of an output element is this map and nothing
// else, which is why every kernel that runs a unit produces the same bits for the same rows.
// Chunks past K load zeros from the clamped address K - 4 (K % 4 == 0 keeps a 16-byte load inside its row).
// SCALED: X is multiplied by `scale` as it is loaded -- (scale * x) rounded once, then the product chain.
template <int ROWS>
struct WaveUnit {
  f32x4 w[4], x[ROWS][4];
};

template <int ROWS, bool SCALED>
__device__ __forceinline__ void wave_load_unit(WaveUnit<ROWS>& u, const float* __restrict__ wp, const float* const (&xp)[ROWS], int k0,
                                               int half, int K, float scale = 1.f) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = k0 + 8 * c + 4 * half;
    const int kc = k < K ? k : K - 4;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 w = *(const f32x4*)(wp + kc);
    f32x4 x[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) x[i] = *(const f32x4*)(xp[i] + kc);
    u.w[c] = k < K ? w : z;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      if constexpr (SCALED) u.x[i][c] = k < K ? x[i] * scale : z;
      else u.x[i][c] = k < K ? x[i] : z;
    }
  }
}

template <int ROWS>
__device__ __forceinline__ void wave_mma_unit(const WaveUnit<ROWS>& u, f32x16 (&acc)[ROWS]) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < ROWS; ++i) acc[i] = mfma32(u.x[i][c][e], u.w[c][e], acc[i]);
}

// ---------------------------------------------------------------------------------------------------------------- the G^T X tile
// One wave = 64 rows n x 64 columns k of dW = G^T X over the token rows [m0, m1) in four independent 32 x 32 accumulators:
// A = G^T (lane l reads G[b + (l >> 5)][n0 + (l & 31)] and the column 32 further), B = X[b + (l >> 5)][k0 + (l & 31)] likewise, both
// 128-byte rows from L2; one MFMA k step per two token rows.  The chain of an element runs over the rows ascending, two per MFMA, with
// zeros behind m1 (exact no-ops at the chain's end): that order does not depend on DEPTH, the number of k steps whose loads are issued
// before their MFMAs -- 4 in seg_wgrad_kernel, 1 in probe_sgd_kernel, each measured for its kernel (profiles/probe_tiles_ab.txt).
// The caller clamps the column pointers into the matrices (ga / gb: G + min(n, N - 1), xa / xb: X + min(k, K - 1)) and says which of
// them are outside (*_out): such a lane multiplies zeros.
template <int DEPTH>
__device__ __forceinline__ void wave_gtx_tile(f32x16 (&acc)[2][2], const float* __restrict__ ga, const float* __restrict__ gb, int ldg,
                                              const float* __restrict__ xa, const float* __restrict__ xb, int ldx, bool na_out,
                                              bool nb_out, bool ka_out, bool kb_out, int m0, int m1, int half) {
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[0][0][i] = acc[0][1][i] = acc[1][0][i] = acc[1][1][i] = 0.f;
  for (int b0 = m0; b0 < m1; b0 += 2 * DEPTH) {
    float a0[DEPTH], a1[DEPTH], x0[DEPTH], x1[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      const int b = b0 + 2 * u + half;
      const long bc = b < m1 ? b : m1 - 1;
      a0[u] = ga[bc * ldg], a1[u] = gb[bc * ldg], x0[u] = xa[bc * ldx], x1[u] = xb[bc * ldx];
      a0[u] = (b >= m1 || na_out) ? 0.f : a0[u];
      a1[u] = (b >= m1 || nb_out) ? 0.f : a1[u];
      x0[u] = (b >= m1 || ka_out) ? 0.f : x0[u];
      x1[u] = (b >= m1 || kb_out) ? 0.f : x1[u];
    }
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      acc[0][0] = mfma32(a0[u], x0[u], acc[0][0]);
      acc[0][1] = mfma32(a0[u], x1[u], acc[0][1]);
      acc[1][0] = mfma32(a1[u], x0[u], acc[1][0]);
      acc[1][1] = mfma32(a1[u], x1[u], acc[1][1]);
    }
  }
}

// f(n, k, value, row(n)) for the lane's elements of the tile at (n0, k0) that lie inside N x K, rows n outermost; row(n) is what
// the caller needs once per row (its learning rate, its output row) and is evaluated once per row
template <class R, class F>
__device__ __forceinline__ void wave_gtx_visit(const f32x16 (&acc)[2][2], int n0, int k0, int N, int K, int r, int half, R&& row, F&& f) {
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int n = n0 + 32 * ti + acc_row(i, half);
      if (n >= N) continue;
      const auto of_row = row(n);
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const int k = k0 + 32 * tj + r;
        if (k < K) f(n, k, acc[ti][tj][i], of_row);
      }
    }
}

// the bias gradient of one output: column n of G (g = G + n) summed serially over the token rows [m0, m1)
__device__ __forceinline__ float wave_gtx_colsum(const float* __restrict__ g, int ldg, int m0, int m1) {
  float s = 0.f;
  for (int b = m0; b < m1; ++b) s += g[(long)b * ldg];
  return s;
}

// ---------------------------------------------------------------------------------------------------------------- the SGD step
// torch.optim.SGD(momentum) on one parameter w with momentum buffer m and gradient d; nlr = -lr.  Two roundings.
__device__ __forceinline__ void sgd_momentum_step(float& w, float& m, float d, float momentum, float nlr) {
  m = fmaf(momentum, m, d);
  w = fmaf(nlr, m, w);
}

}  // namespace vtp
