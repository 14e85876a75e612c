// Zero-shot classification (reference: tools/test_zero_shot_hf.py): the tool's own arithmetic as two fused exact-fp32 kernels --
//   vtp_zs_class_mean : mean over the templates of a class, F.normalize                       (_process_batch, :383-385)
//   vtp_zs_topk       : 100.0 * image_features @ classifier, accuracy(logits, targets, (1, 5))  (:432-437, :312-316) in ONE launch
// The tool runs this at precision 'fp32', so both kernels are fp32 in and out; the product runs on the f32-input MFMA (mfma_f32.h):
// every logit is the same sequential fmaf chain over k whichever tile, lane or launch geometry computes it (no split of k).
// Counters are integers and only integer atomics touch them: counts and ranks are bit-reproducible from run to run.
#include "common.h"
#include "vtp_hip.h"
#include "wave_f32.h"

#include <limits.h>

namespace vtp {

// ---------------------------------------------------------------------------------------------------------------- class mean
// One workgroup per class.  Thread t owns the 16-byte column groups t, t + 256, ...: it sums the T template rows in the order
// 0..T-1, divides by T and leaves the mean in the output row; the sum of squares is reduced in a fixed order (block_sum), then
// every thread rescales the columns it wrote itself.  Nothing depends on how many classes one launch covers.
__global__ __launch_bounds__(256) void zs_class_mean_kernel(const float* __restrict__ feat, int ldf, float* __restrict__ Wt, int ldw,
                                                           int T, int D, float eps) {
  __shared__ float red[4];
  const float* src = feat + (long)blockIdx.x * T * ldf;
  float* dst = Wt + (long)blockIdx.x * ldw;
  const float tf = (float)T;
  float ss = 0.f;
  for (int d = threadIdx.x * 4; d < D; d += 1024) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int t = 0; t < T; ++t) s += *(const f32x4*)(src + (long)t * ldf + d);
    s /= tf;
    *(f32x4*)(dst + d) = s;
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += s[e] * s[e];
  }
  ss = block_sum<4>(ss, red);
  const float den = fmaxf(sqrtf(ss), eps);  // F.normalize: x / max(||x||_2, eps) -- an all-zero class stays a zero row
  for (int d = threadIdx.x * 4; d < D; d += 1024) {
    f32x4 s = *(const f32x4*)(dst + d);
    s /= den;
    *(f32x4*)(dst + d) = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------- logits + top-k
// One workgroup = 32 rows of the batch against every class; its eight waves (two per SIMD) take the 32-column tiles of the
// classifier in turn, each tile over the whole of K in one accumulator (the MFMA's dependent latency equals its issue interval,
// so one chain keeps the matrix pipe full).  The row block's logits stay in LDS ([32][CH], CH <= 1024 columns = 128 KiB): for
// C <= 1024 one pass, beyond that chunk after chunk with the per-row state (rank so far, best five so far) carried in LDS.
// Measured at B = 128 / 256, C = 1000, D = 768: 200 us on 4 / 8 workgroups, 2.4 x the 82 us its MFMAs need; four waves with one
// unit of prefetch took 193 us, so neither occupancy nor prefetch depth is what it waits for.  Every lane loads its own row
// (a wave's 16-byte loads touch 32 cache lines each, and every tile re-reads the feature block): operands staged through LDS
// from line-wide loads, and a split of the classes over workgroups, are not built (profiles/README.md).
//   k order of a chain: the k unit of wave_f32.h, one row of F per lane.  The feature is scaled as it is loaded: (scale * F) rounded
//   once, then the product chain -- the tool's (100.0 * f) @ W.
// The target's logit: with one chunk it is read from LDS.  With several it is needed before its column has been computed, so
// wave 0 first multiplies the row block by the 32 gathered target rows Wt[t_b] and keeps the diagonal -- the same chain on the
// same operands as the element z[b, t_b] of the regular tile, hence the same bits.
constexpr int ZS_ROWS = 32, ZS_MAX_CH = 1024, ZS_WAVES = 8, ZS_PER_LANE = ZS_MAX_CH / 64;

// 32 rows (xp: the lane's row of F) x 32 columns (wp: the lane's row of Wt) over the whole of K.  Two units are in flight beyond
// the one being multiplied (three named units in rotation, no register copies).  Loads past K go to clamped addresses and are
// never multiplied.
__device__ __forceinline__ f32x16 zs_tile(const float* __restrict__ wp, const float* __restrict__ xp, int half, int K, float scale) {
  f32x16 acc[1];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;
  const float* const xs[1] = {xp};
  auto load = [&](WaveUnit<1>& u, int k0) { wave_load_unit<1, true>(u, wp, xs, k0, half, K, scale); };
  WaveUnit<1> u0, u1, u2;
  load(u0, 0);
  load(u1, 32);
  for (int k0 = 0; k0 < K; k0 += 96) {
    load(u2, k0 + 64);
    wave_mma_unit(u0, acc);
    if (k0 + 32 >= K) break;
    load(u0, k0 + 96);
    wave_mma_unit(u1, acc);
    if (k0 + 64 >= K) break;
    load(u1, k0 + 128);
    wave_mma_unit(u2, acc);
  }
  return acc[0];
}

__global__ __launch_bounds__(ZS_WAVES * 64) void zs_topk_kernel(const float* __restrict__ F, int ldf, const float* __restrict__ Wt,
                                                     int ldw, const long* __restrict__ targets, float scale, int B, int C, int K, int CH,
                                                     unsigned long long* __restrict__ counts, int* __restrict__ per_class,
                                                     int* __restrict__ rank, int* __restrict__ pred, float* __restrict__ logits,
                                                     int ldl) {
  extern __shared__ __attribute__((aligned(16))) float zs[];  // [ZS_ROWS][CH]
  __shared__ float zt_s[ZS_ROWS];                             // the target's logit per row
  __shared__ int tgt_s[ZS_ROWS];                              // the target per row, -1 outside [0, C)
  __shared__ int rank_s[ZS_ROWS];
  __shared__ float best_v[ZS_ROWS][5];
  __shared__ int best_i[ZS_ROWS][5];
  __shared__ int hit_s[2];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, half = lane >> 5, w = tid >> 6;
  const int b0 = blockIdx.x * ZS_ROWS;
  const int chunks = (C + CH - 1) / CH;
  if (tid < ZS_ROWS) {
    const long t = b0 + tid < B ? targets[b0 + tid] : -1;
    tgt_s[tid] = (t >= 0 && t < C) ? (int)t : -1;
    rank_s[tid] = 0;
    zt_s[tid] = 0.f;
  }
  if (tid < 2) hit_s[tid] = 0;
  __syncthreads();
  const float* xp = F + (long)(b0 + r < B ? b0 + r : B - 1) * ldf;  // rows past B: a valid row, results never used
  if (chunks > 1) {
    if (w == 0) {
      const int t = tgt_s[r];
      const f32x16 acc = zs_tile(Wt + (long)(t < 0 ? 0 : t) * ldw, xp, half, K, scale);
      // the diagonal element (row r, column r) sits in the lane half (r >> 2) & 1, register (r & 3) + 4 (r >> 3)
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) v = i == (r & 3) + 4 * (r >> 3) ? acc[i] : v;
      if (half == ((r >> 2) & 1)) zt_s[r] = v;
    }
    __syncthreads();
  }
  for (int ch = 0; ch < chunks; ++ch) {
    const int c0 = ch * CH, cw = C - c0 < CH ? C - c0 : CH, tiles = (cw + 31) / 32;
    for (int t = w; t < tiles; t += ZS_WAVES) {
      const int n = c0 + t * 32 + r;
      const f32x16 acc = zs_tile(Wt + (long)(n < C ? n : C - 1) * ldw, xp, half, K, scale);  // columns past C: never read back
#pragma unroll
      for (int i = 0; i < 16; ++i) zs[acc_row(i, half) * CH + t * 32 + r] = acc[i];
    }
    __syncthreads();
    if (chunks == 1) {
      if (tid < ZS_ROWS && tgt_s[tid] >= 0) zt_s[tid] = zs[tid * CH + tgt_s[tid]];
      __syncthreads();
    }
    // wave w owns rows 4 w .. 4 w + 3 of the block: nobody else touches their rank_s / best_* entries.  A lane takes the row's
    // columns lane, lane + 64, ... of the chunk into registers once (at most ZS_PER_LANE of them)
    constexpr int RPW = ZS_ROWS / ZS_WAVES;
    for (int j = 0; j < RPW; ++j) {
      const int row = w * RPW + j, b = b0 + row;
      if (b >= B) break;
      const float* zrow = zs + row * CH;
      const int t = tgt_s[row];
      float v[ZS_PER_LANE];
#pragma unroll
      for (int i = 0; i < ZS_PER_LANE; ++i) v[i] = lane + 64 * i < cw ? zrow[lane + 64 * i] : 0.f;
      if (logits) {
#pragma unroll
        for (int i = 0; i < ZS_PER_LANE; ++i)
          if (lane + 64 * i < cw) logits[(long)b * ldl + c0 + lane + 64 * i] = v[i];
      }
      if (t >= 0) {
        const float ztv = zt_s[row];
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < ZS_PER_LANE; ++i) cnt += (lane + 64 * i < cw && before(v[i], c0 + lane + 64 * i, ztv, t)) ? 1 : 0;
        cnt = wave_sum_int(cnt);
        if (lane == 0) rank_s[row] += cnt;
      }
      if (pred) {
        // five selection rounds over this chunk and the best five of the chunks before it: round q takes the first element in
        // topk order that comes strictly after the pick of round q - 1
        float ov = 0.f;
        int oi = -1;
        if (ch > 0 && lane < 5) ov = best_v[row][lane], oi = best_i[row][lane];
        float pv = INFINITY;
        int pi = -1;
        float nv[5];
        int ni[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
          float mv = 0.f;
          int mi = INT_MAX;  // INT_MAX: nothing found yet
#pragma unroll
          for (int i = 0; i < ZS_PER_LANE; ++i) {
            const int gi = c0 + lane + 64 * i;
            if (lane + 64 * i < cw && before(pv, pi, v[i], gi) && (mi == INT_MAX || before(v[i], gi, mv, mi))) mv = v[i], mi = gi;
          }
          if (oi >= 0 && before(pv, pi, ov, oi) && (mi == INT_MAX || before(ov, oi, mv, mi))) mv = ov, mi = oi;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const float xv = __shfl_xor(mv, o, 64);
            const int xi = __shfl_xor(mi, o, 64);
            if (xi != INT_MAX && (mi == INT_MAX || before(xv, xi, mv, mi))) mv = xv, mi = xi;
          }
          nv[q] = mv, ni[q] = mi == INT_MAX ? -1 : mi;  // fewer than five comparable values (NaN logits): -1
          pv = mi == INT_MAX ? -INFINITY : mv, pi = mi;  // (-inf, INT_MAX): nothing comes after it
        }
        if (lane == 0) {
#pragma unroll
          for (int q = 0; q < 5; ++q) best_v[row][q] = nv[q], best_i[row][q] = ni[q];
        }
      }
    }
    __syncthreads();  // the next chunk overwrites zs
  }
  if (tid < ZS_ROWS && b0 + tid < B) {
    const int b = b0 + tid, t = tgt_s[tid];
    const int rk = t >= 0 ? rank_s[tid] : C;  // a target outside [0, C): rank C, a miss
    if (rank) rank[b] = rk;
    if (rk < 1) atomicAdd(&hit_s[0], 1);
    if (rk < 5) atomicAdd(&hit_s[1], 1);
    if (per_class && t >= 0) {
      atomicAdd(per_class + t, 1);
      if (rk < 1) atomicAdd(per_class + C + t, 1);
    }
    if (pred) {
#pragma unroll
      for (int q = 0; q < 5; ++q) pred[(long)b * 5 + q] = best_i[tid][q];
    }
  }
  __syncthreads();
  if (tid == 0 && counts) {
    atomicAdd(counts + 0, (unsigned long long)hit_s[0]);
    atomicAdd(counts + 1, (unsigned long long)hit_s[1]);
    atomicAdd(counts + 2, (unsigned long long)(B - b0 < ZS_ROWS ? B - b0 : ZS_ROWS));
  }
}

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_zs_class_mean(const float* feat, int ldf, float* Wt, int ldw, int C, int T, int D, float eps, void* stream) {
  VTP_REQUIRE(feat && Wt, "vtp_zs_class_mean: null pointer");
  VTP_REQUIRE(C >= 1 && T >= 1 && D >= 4 && D % 4 == 0, "vtp_zs_class_mean: bad shape (C, T >= 1, D %% 4 == 0)");
  VTP_REQUIRE(ldf >= D && ldf % 4 == 0 && ldw >= D && ldw % 4 == 0,
              "vtp_zs_class_mean: bad leading dimension (ldf, ldw >= D, ldf %% 4 == 0, ldw %% 4 == 0)");
  VTP_REQUIRE(aligned16(feat) && aligned16(Wt), "vtp_zs_class_mean: feat and Wt must be 16-byte aligned");
  hipLaunchKernelGGL(zs_class_mean_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, feat, ldf, Wt, ldw, T, D, eps);
  return check_launch("zs_class_mean");
}

extern "C" int vtp_zs_topk(const float* F, int ldf, const float* Wt, int ldw, const long* targets, float scale, int B, int C, int D,
                           long* counts, int* per_class, int* rank, int* pred, float* logits, int ldl, void* stream) {
  VTP_REQUIRE(F && Wt && targets, "vtp_zs_topk: null pointer (F, Wt, targets)");
  VTP_REQUIRE(B >= 1 && D >= 4 && D % 4 == 0, "vtp_zs_topk: bad shape (B >= 1, D %% 4 == 0)");
  VTP_REQUIRE(C >= 5, "vtp_zs_topk: C >= 5 (the top-5 of fewer classes does not exist)");
  VTP_REQUIRE(ldf >= D && ldf % 4 == 0 && ldw >= D && ldw % 4 == 0,
              "vtp_zs_topk: bad leading dimension (ldf, ldw >= D, ldf %% 4 == 0, ldw %% 4 == 0)");
  VTP_REQUIRE(!logits || ldl >= C, "vtp_zs_topk: bad leading dimension (ldl >= C)");
  VTP_REQUIRE(aligned16(F) && aligned16(Wt), "vtp_zs_topk: F and Wt must be 16-byte aligned");
  const int cpad = (int)(((long)C + 31) / 32 * 32 < ZS_MAX_CH ? ((long)C + 31) / 32 * 32 : ZS_MAX_CH);
  const int lds = ZS_ROWS * cpad * 4;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)zs_topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ZS_ROWS * ZS_MAX_CH * 4);
    attr = true;
  }
  hipLaunchKernelGGL(zs_topk_kernel, dim3(cdiv(B, ZS_ROWS)), dim3(ZS_WAVES * 64), lds, (hipStream_t)stream, F, ldf, Wt, ldw, targets, scale, B, C,
                     D, cpad, (unsigned long long*)counts, per_class, rank, pred, logits, ldl);
  return check_launch("zs_topk");
}
