// Linear probing (reference: tools/test_linear_probing_hf.py): every classifier of a feature group as ONE fused fp32 step --
//   vtp_probe_logits : logits = X W_all^T + bias          (LinearClassifier.forward :164-170 for all heads of the group)
//   vtp_probe_ce     : CrossEntropyLoss(mean) per head, top-1 counts, dlogits                             (:285, :327-328)
//   vtp_probe_sgd    : torch.optim.SGD(momentum) step of every head; dW lives in the MFMA accumulators only     (:487, :288-290)
// The reference does this arithmetic in fp32 outside its autocast context, so all three kernels are fp32 in and out on the
// f32-input MFMA v_mfma_f32_32x32x2_f32: bit-for-bit a k-ordered fmaf chain per output element (one rounding per product).
//   operand maps (one f32 VGPR each): lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31];
//   C/D: column j = l & 31, row i = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5), reg in [0, 16).
// Every output element has exactly one writer and a reduction order that depends on neither its tile nor its position in it: two
// heads with equal parameters stay bit-identical, and so do data-parallel replicas that run the same full-batch step.
#include "common.h"
#include "vtp_hip.h"
#include "wave_f32.h"

#include <limits.h>

namespace vtp {

// ---------------------------------------------------------------------------------------------------------------- logits
// One wave = 64 rows x 32 columns of the output over the whole of K; no LDS, no barrier.  Waves that share a column strip sit
// next to each other (the row pair is the fast task index), so a W strip comes from HBM once and X (<= 2 MB) from L2.
// The k unit (32 wide, wave_f32.h) holds both rows.  The next unit is loaded before the current one's 32 MFMAs (2048 cycles) are
// issued: one wave per SIMD has to cover the HBM latency by itself.
__global__ __launch_bounds__(256) void probe_logits_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ W,
                                                          const float* __restrict__ bias, float* __restrict__ logits, int ldl, int B,
                                                          int N, int K, int row_pairs, int tasks) {
  const int lane = threadIdx.x & 63, r = lane & 31, half = lane >> 5;
  const int task = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (task >= tasks) return;
  const int n0 = (task / row_pairs) * 32, b0 = (task % row_pairs) * 64;
  const int n = n0 + r, nc = n < N ? n : N - 1;
  const int ba = b0 + r, bb = b0 + 32 + r;
  const float* wp = W + (long)nc * K;
  // rows past B: a valid row, results never stored
  const float* const xp[2] = {X + (long)(ba < B ? ba : B - 1) * ldx, X + (long)(bb < B ? bb : B - 1) * ldx};
  const float bn = bias[nc];
  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[0][i] = acc[1][i] = bn;  // the bias opens the chain: K + 1 roundings per element
  WaveUnit<2> cur, nxt;
  wave_load_unit<2, false>(cur, wp, xp, 0, half, K);
  for (int k0 = 0; k0 < K; k0 += 32) {
    wave_load_unit<2, false>(nxt, wp, xp, k0 + 32, half, K);  // past K: clamped addresses, zeros (never used after the last unit)
    wave_mma_unit(cur, acc);
    cur = nxt;
  }
  if (n >= N) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int b = b0 + acc_row(i, half);
    if (b < B) logits[(long)b * ldl + n] = acc[0][i];
    if (b + 32 < B) logits[(long)(b + 32) * ldl + n] = acc[1][i];
  }
}

// ---------------------------------------------------------------------------------------------------------------- cross-entropy
// One workgroup per (row b, head h).  Three passes over the C logits of the row (L2-resident): maximum with its lowest index,
// sum of exponentials, gradient.  Reductions run in a fixed order, so dlogits does not depend on the launch.
__global__ __launch_bounds__(256) void probe_ce_kernel(const float* __restrict__ logits, int ldl, const long* __restrict__ labels,
                                                      int C, float inv_rows, float* __restrict__ loss, int* __restrict__ correct,
                                                      float* __restrict__ dlogits) {
  __shared__ float red_v[4];
  __shared__ int red_i[4];
  __shared__ float red_s[4];
  const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* z = logits + (long)b * ldl + (long)h * C;
  float m = -INFINITY;
  int mi = INT_MAX;
  for (int c = tid; c < C; c += 256) {
    const float v = z[c];
    if (v > m || mi == INT_MAX) m = v, mi = c;  // strict >: the first (lowest) index of a thread's maximum stays
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (oi != INT_MAX && (mi == INT_MAX || before(om, oi, m, mi))) m = om, mi = oi;
  }
  if (lane == 0) red_v[w] = m, red_i[w] = mi;
  __syncthreads();
  m = red_v[0], mi = red_i[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const float om = red_v[i];
    const int oi = red_i[i];
    if (oi != INT_MAX && (mi == INT_MAX || before(om, oi, m, mi))) m = om, mi = oi;
  }
  float s = 0.f;
  for (int c = tid; c < C; c += 256) s += expf(z[c] - m);
  s = block_sum<4>(s, red_s);
  const long lab = labels[b];
  const bool lab_ok = lab >= 0 && lab < C;  // labels are class indices in [0, C); anything else contributes no target term
  if (tid == 0) {
    const float zl = lab_ok ? z[lab] : m;
    atomicAdd(loss + h, (logf(s) - (zl - m)) * inv_rows);
    if (correct && lab_ok && mi == (int)lab) atomicAdd(correct + h, 1);
  }
  if (!dlogits) return;
  float* d = dlogits + (long)b * ldl + (long)h * C;
  const float inv_s = 1.f / s;
  for (int c = tid; c < C; c += 256) {
    const float p = expf(z[c] - m) * inv_s;
    d[c] = ((lab_ok && c == (int)lab) ? p - 1.f : p) * inv_rows;
  }
}

// ---------------------------------------------------------------------------------------------------------------- SGD step
// One wave = a 64 (rows n) x 64 (columns k) tile of W: dW = dlogits^T X over the whole batch (the G^T X tile of wave_f32.h), then one
// read-modify-write of mW and W in the accumulator layout -- 16 bytes of HBM traffic per parameter, dW never stored.
// The waves of k tile 0 also form db and update bias / mb.
// The learning rate is looked up per output row n / C: 1000 classes are no multiple of 64, so a tile straddles heads.
__global__ __launch_bounds__(256) void probe_sgd_kernel(float* __restrict__ W, float* __restrict__ bias, float* __restrict__ mW,
                                                       float* __restrict__ mb, const float* __restrict__ dl, int ldl,
                                                       const float* __restrict__ X, int ldx, const float* __restrict__ lr, int B, int N,
                                                       int C, int K, float momentum, int k_tiles, int tasks) {
  const int lane = threadIdx.x & 63, r = lane & 31, half = lane >> 5;
  const int task = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (task >= tasks) return;
  const int n0 = (task / k_tiles) * 64, k0 = (task % k_tiles) * 64;
  const int na = n0 + r, nb = n0 + 32 + r, ka = k0 + r, kb = k0 + 32 + r;
  f32x16 acc[2][2];
  wave_gtx_tile<1>(acc, dl + (na < N ? na : N - 1), dl + (nb < N ? nb : N - 1), ldl, X + (ka < K ? ka : K - 1), X + (kb < K ? kb : K - 1),
                ldx, na >= N, nb >= N, ka >= K, kb >= K, 0, B, half);
  wave_gtx_visit(
      acc, n0, k0, N, K, r, half, [&](int n) { return -lr[n / C]; },
      [&](int n, int k, float d, float nlr) {
        const long idx = (long)n * K + k;
        float m = mW[idx];
        float w = W[idx];
        sgd_momentum_step(w, m, d, momentum, nlr);
        mW[idx] = m;
        W[idx] = w;
      });
  if (k0 == 0) {
    const int n = n0 + lane;
    if (n < N) {
      float w = bias[n], m = mb[n];
      sgd_momentum_step(w, m, wave_gtx_colsum(dl + n, ldl, 0, B), momentum, -lr[n / C]);
      mb[n] = m;
      bias[n] = w;
    }
  }
}

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_probe_logits(const float* X, int ldx, const float* W, const float* bias, float* logits, int ldl, int B, int N,
                                int K, void* stream) {
  VTP_REQUIRE(X && W && bias && logits, "vtp_probe_logits: null pointer");
  VTP_REQUIRE(B >= 1 && N >= 1 && K >= 4 && K % 4 == 0, "vtp_probe_logits: bad shape (B, N >= 1, K %% 4 == 0)");
  VTP_REQUIRE(ldx >= K && ldx % 4 == 0 && ldl >= N, "vtp_probe_logits: bad leading dimension (ldx >= K, ldx %% 4 == 0, ldl >= N)");
  VTP_REQUIRE(aligned16(X) && aligned16(W), "vtp_probe_logits: X and W must be 16-byte aligned");
  const long row_pairs = cdiv(B, 64), tasks = row_pairs * cdiv(N, 32);
  VTP_REQUIRE(tasks <= INT_MAX, "vtp_probe_logits: too many tiles");
  hipLaunchKernelGGL(probe_logits_kernel, dim3(cdiv(tasks, 4)), dim3(256), 0, (hipStream_t)stream, X, ldx, W, bias, logits, ldl, B, N,
                     K, (int)row_pairs, (int)tasks);
  return check_launch("probe_logits");
}

extern "C" int vtp_probe_ce(const float* logits, int ldl, const long* labels, int B, int H, int C, float inv_rows, float* loss,
                            int* correct, float* dlogits, void* stream) {
  VTP_REQUIRE(logits && labels && loss, "vtp_probe_ce: null pointer");
  VTP_REQUIRE(B >= 1 && H >= 1 && H <= 65535 && C >= 1 && (long)H * C <= INT_MAX, "vtp_probe_ce: bad shape (B, H, C >= 1)");
  VTP_REQUIRE(ldl >= (long)H * C, "vtp_probe_ce: bad leading dimension (ldl >= H * C)");
  hipLaunchKernelGGL(probe_ce_kernel, dim3(B, H), dim3(256), 0, (hipStream_t)stream, logits, ldl, labels, C, inv_rows, loss, correct,
                     dlogits);
  return check_launch("probe_ce");
}

extern "C" int vtp_probe_sgd(float* W, float* bias, float* mW, float* mb, const float* dlogits, int ldl, const float* X, int ldx,
                             const float* lr, int B, int H, int C, int K, float momentum, void* stream) {
  VTP_REQUIRE(W && bias && mW && mb && dlogits && X && lr, "vtp_probe_sgd: null pointer");
  VTP_REQUIRE(B >= 1 && H >= 1 && C >= 1 && (long)H * C <= INT_MAX && K >= 4 && K % 4 == 0,
              "vtp_probe_sgd: bad shape (B, H, C >= 1, K %% 4 == 0)");
  VTP_REQUIRE(ldx >= K && ldx % 4 == 0 && ldl >= (long)H * C,
              "vtp_probe_sgd: bad leading dimension (ldx >= K, ldx %% 4 == 0, ldl >= H * C)");
  const int N = H * C;
  const long k_tiles = cdiv(K, 64), tasks = k_tiles * cdiv(N, 64);
  VTP_REQUIRE(tasks <= INT_MAX, "vtp_probe_sgd: too many tiles");
  hipLaunchKernelGGL(probe_sgd_kernel, dim3(cdiv(tasks, 4)), dim3(256), 0, (hipStream_t)stream, W, bias, mW, mb, dlogits, ldl, X, ldx,
                     lr, B, N, C, K, momentum, (int)k_tiles, (int)tasks);
  return check_launch("probe_sgd");
}
