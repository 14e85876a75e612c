// The 128 x 128 exact-fp32 tile product that knn.hip, precision_recall.hip and retrieval.hip share: the main loop of vtp_gemm_nt_f32 (fp32.hip) with
// the bank rows as the A operand and the queries as the B operand, so a query sits on a lane and its candidates are accumulator
// registers.  256 threads, four waves in 2 x 2 (wm, wn), each 2 x 2 MFMA tiles of 32 x 32 on v_mfma_f32_32x32x2_f32, K slabs of 16
// staged through LDS transposed ([k][row]), two buffers, the loads of slab t + 1 in flight under the MFMAs of slab t.  The chain of
// an element runs over k = 0 .. D-1 ascending with no split of k: the bits of vtp_gemm_nt_f32 with the plain epilogue.
//   result: lane (j = lane & 31, half = lane >> 5) of wave (wm, wn) holds in acc[u][v][r] the product of the tile's bank row
//   wm * 64 + u * 32 + acc_row(r, half) with the query wn * 64 + v * 32 + j of the row block.
#pragma once
#include "common.h"
#include "mfma_f32.h"

namespace vtp {

constexpr int TF_BM = 128, TF_BQ = 128, TF_BK = 16;  // bank rows per tile, queries per row block, K slab
constexpr int TF_KQ = TF_BK / 4;                     // 16-byte loads per tile row and slab
constexpr int TF_IT = TF_KQ / 2;                     // loads per thread, operand and slab
constexpr int TF_LD = 128 + 16 / TF_KQ;              // as GF_LD (fp32.hip): the k groups of a wave's write land on disjoint banks

// Thread tid loads the 16 bytes at column 4 * kq (kq = tid & (TF_KQ - 1)) of the tile rows lr[it] = tid / TF_KQ + (256 / TF_KQ) * it:
// ap[it] / bp[it] point there in the bank / the queries, or are null for a row outside the chunk / the batch (read as zeros).
// Every thread of the workgroup calls this; it ends behind a barrier, so the slabs are free again when it returns.
__device__ __forceinline__ void tile_f32_product(const float* (&ap)[TF_IT], const float* (&bp)[TF_IT], int (&lr)[TF_IT],
                                                 int kq, int D, float (&As)[2][TF_BK][TF_LD], float (&Bs)[2][TF_BK][TF_LD], int wm, int wn,
                                                 int j, int half, f32x16 (&acc)[2][2]) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int nslab = (D + TF_BK - 1) / TF_BK;
  f32x4 ar[TF_IT], br[TF_IT];
  auto load_slab = [&](int k0) {
    const bool kin = k0 + 4 * kq < D;
#pragma unroll
    for (int it = 0; it < TF_IT; ++it) {
      ar[it] = (ap[it] && kin) ? *(const f32x4*)(ap[it] + k0) : zero4;
      br[it] = (bp[it] && kin) ? *(const f32x4*)(bp[it] + k0) : zero4;
    }
  };
  auto store_slab = [&](int buf) {
#pragma unroll
    for (int it = 0; it < TF_IT; ++it)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        As[buf][4 * kq + e][lr[it]] = ar[it][e];
        Bs[buf][4 * kq + e][lr[it]] = br[it][e];
      }
  };
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][v][r] = 0.f;

  load_slab(0);
  store_slab(0);
  __syncthreads();
  for (int t = 0; t < nslab; ++t) {
    const int buf = t & 1;
    if (t + 1 < nslab) load_slab((t + 1) * TF_BK);  // in flight under the MFMAs below
#pragma unroll
    for (int kk = 0; kk < TF_BK / 2; ++kk) {
      const int k = 2 * kk + half;
      float a[2], b[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        a[u] = As[buf][k][wm * 64 + u * 32 + j];
        b[u] = Bs[buf][k][wn * 64 + u * 32 + j];
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = mfma32(a[u], b[v], acc[u][v]);
    }
    if (t + 1 < nslab) store_slab(buf ^ 1);
    __syncthreads();
  }
}

}  // namespace vtp
