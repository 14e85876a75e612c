// Cross-modal retrieval on the CLIP heads (image -> text and text -> image recall@K on a captioned set, the evaluation the CLIP paper
// reports on Flickr30k and MSCOCO-5k), restated from the papers' description, as fused exact-fp32 kernels --
//   vtp_retr_best  : per query the best of its ground-truth gallery rows, (s*, j*), from a CSR of ground-truth lists.
//   vtp_retr_rank  : per query the number of rows of a gallery chunk that come before (s*, j*): one sweep of the chunk over a batch
//                    of queries, the similarities formed tile by tile and never written (except sims_out, for tests).
//   vtp_retr_count : ranks -> the R@K counters and the row count, and a copy of the ranks into the evaluation's rank buffer.
// Replaces a chunked torch.matmul + gather + compare + sum; neither the [B, N] matrix nor a row of it is ever held.
//
// Arithmetic.  s(i, j) is the fmaf chain over k = 0 .. D-1 ascending with no split of k, the bits of element [i, j] of
//   vtp_gemm_nt_f32(Q, X) with the plain epilogue.  Gallery rows are ordered by (similarity descending, gallery index ascending), a
//   total order (the tie rule of vtp_zs_topk and vtp_knn_topk: the lower index wins).  (s*, j*) is the first ground-truth row of a
//   query under that order and rank = #{j : s(i, j) > s*} + #{j < j* : s(i, j) == s*}: the rows strictly before (s*, j*).  No
//   ground-truth row is ever counted, by construction.  A query without a ground-truth row has (s*, j*) = (-inf, -1) and every
//   gallery row counts: rank = N, a miss at every K and still a row.  A NaN similarity compares false everywhere: it never beats
//   anything and is never chosen as s*; inputs are finite by contract.
//
// retr_best_kernel.  Work is cut over (query, list entry) pairs, 64 pairs per round and one pair per thread of the first wave, so a
//   set with one ground-truth row per query and one with five cost the same per pair.  Workgroup g owns the queries whose list
//   starts at a pair in [64 g, 64 g + 64) (a query with an empty list starts where the next one does) and walks their pairs in
//   rounds of 64; a list of more than 64 entries simply takes more rounds of its owner.  A round finds the query of every pair by
//   binary search in gt_ptr, stages the 64 query rows and the 64 gallery rows in slabs of 64 columns through LDS with coalesced
//   16-byte loads, and thread r walks pair r with one scalar fmaf chain over k ascending (the way pr_sqnorm_kernel gets the diagonal:
//   the bits of the tile).  Columns past D up to the tile's slab of 16 are zeros, as in the tile.  The thread of the first pair of a
//   query within the round folds the round's pairs of that query into the query's running best, which lives in the output: one
//   owner per query, no atomics.  An index outside [0, n_total) is ignored.
// retr_rank_kernel.  The bank sweep of tile_f32.h (the walk and the tile product that knn_topk_kernel and the precision / recall
//   kernels run as well; the product is the main loop of vtp_gemm_nt_f32 itself): grid = chunk splits x row blocks of 128 queries,
//   256 threads, 128 x 128 tiles on v_mfma_f32_32x32x2_f32; a query sits on a lane and its candidates are accumulator registers.
//   The epilogue compares each of the lane's 64 values with the (s*, j*) of its query and counts per lane; sweep_add_counts sums
//   the four lane-sets of a query (wm x half) in LDS and one integer atomicAdd per query and workgroup reaches memory: exact and
//   order-free, so the result is identical whatever the chunking, the splits, B or the grid.
// LDS: retr_rank 33 KiB of operand slabs + 2 KiB of counts, two workgroups per CU; retr_best 2 x 64 x 65 x 4 B = 33 KiB.
#include "common.h"
#include "mfma_f32.h"
#include "tile_f32.h"
#include "vtp_hip.h"

#include <limits.h>
#include <math.h>

namespace vtp {

constexpr int RT_NB = 64;     // pairs per round of retr_best_kernel
constexpr int RT_MAXNK = 8;   // recall levels per vtp_retr_count call

// ---------------------------------------------------------------------------------------------------------------- best ground truth
__global__ __launch_bounds__(256) void retr_best_kernel(const float* Q, int ldq, const float* X, int ldx, long n_total, const int* gt_ptr,
                                                        const long* gt_idx, int nnz, int B, int D, float* best_s, long* best_j) {
  __shared__ float tq[RT_NB][RT_NB + 1], tx[RT_NB][RT_NB + 1];
  __shared__ long pj[RT_NB];   // the gallery row of the round's pair, -1: none (past the end, or an index out of range)
  __shared__ int pb[RT_NB];    // its query, -1: past the end
  __shared__ float ps[RT_NB];  // its similarity
  const int tid = threadIdx.x;
  // the first query in [0, B) whose list starts at or behind pair v (the same for every thread)
  auto first_from = [&](long v) {
    int a = 0, z = B;
    while (a < z) {
      const int m = (a + z) >> 1;
      if (gt_ptr[m] < v) a = m + 1;
      else z = m;
    }
    return a;
  };
  const long own = (long)blockIdx.x * RT_NB;
  const int b_lo = first_from(own), b_hi = first_from(own + RT_NB);
  if (b_lo == b_hi) return;
  for (int b = b_lo + tid; b < b_hi; b += 256) best_s[b] = -INFINITY, best_j[b] = -1;
  // (the clamps and the range checks below keep every access inside the arrays whatever gt_ptr holds)
  const int pbeg = gt_ptr[b_lo] > 0 ? gt_ptr[b_lo] : 0;
  const int pend = gt_ptr[b_hi] < nnz ? gt_ptr[b_hi] : nnz;  // b_hi <= B: gt_ptr has B + 1 entries
  const int dpad = (D + TF_BK - 1) / TF_BK * TF_BK;          // the tile walks whole slabs of 16 columns
  __syncthreads();

  for (int p0 = pbeg; p0 < pend; p0 += RT_NB) {
    if (tid < RT_NB) {
      const int p = p0 + tid;
      int b = -1;
      long j = -1;
      if (p < pend) {
        int a = b_lo, z = b_hi;  // the last owned query whose list starts at or before p
        while (a < z) {
          const int m = (a + z) >> 1;
          if (gt_ptr[m] <= p) a = m + 1;
          else z = m;
        }
        b = a - 1 >= b_lo ? a - 1 : -1;
        j = gt_idx[p];
        if (j < 0 || j >= n_total || b < 0) j = -1;
      }
      pb[tid] = b, pj[tid] = j;
    }
    __syncthreads();
    float acc = 0.f;
    for (int k0 = 0; k0 < D; k0 += RT_NB) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int e = tid + 256 * it, r = e >> 4, c = 4 * (e & 15);
        f32x4 q = {0.f, 0.f, 0.f, 0.f}, x = {0.f, 0.f, 0.f, 0.f};
        const long j = pj[r];
        if (j >= 0 && k0 + c < D) {
          q = *(const f32x4*)(Q + (size_t)pb[r] * ldq + k0 + c);
          x = *(const f32x4*)(X + (size_t)j * ldx + k0 + c);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) tq[r][c + i] = q[i], tx[r][c + i] = x[i];
      }
      __syncthreads();
      if (tid < RT_NB) {
        const int kn = dpad - k0 < RT_NB ? dpad - k0 : RT_NB;
        for (int k = 0; k < kn; ++k) acc = fmaf(tx[tid][k], tq[tid][k], acc);
      }
      __syncthreads();
    }
    if (tid < RT_NB) ps[tid] = acc;
    __syncthreads();
    // the first pair of a query within the round folds the round's pairs of that query into the query's best
    if (tid < RT_NB && pb[tid] >= 0 && (tid == 0 || pb[tid - 1] != pb[tid])) {
      const int b = pb[tid];
      float s = best_s[b];
      long j = best_j[b];
      for (int t = tid; t < RT_NB && pb[t] == b; ++t)
        if (pj[t] >= 0 && before(ps[t], pj[t], s, j)) s = ps[t], j = pj[t];
      best_s[b] = s, best_j[b] = j;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- rank
struct RetrArgs {
  SweepArgs sw;
  const float* best_s;
  const long* best_j;
  int* beats;
  float* sims_out;
  long index_base;
  int lds;
};

struct RetrLds {
  float As[2][TF_BK][TF_LD];  // gallery rows
  float Bs[2][TF_BK][TF_LD];  // queries
  int cnt[4][TF_BQ];          // [wm * 2 + half][query]
};

__global__ __launch_bounds__(256, 2) void retr_rank_kernel(const RetrArgs g) {
  __shared__ __attribute__((aligned(16))) RetrLds L;
  const SweepCtx c = sweep_begin(g.sw);
  // this lane's two queries c.query(v): the best ground-truth row in rows of the chunk (negative: none), and the count
  float bs[2];
  long bj[2];
  int cnt[2] = {0, 0};
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int ql = c.query(v);
    bs[v] = ql < c.nq ? g.best_s[c.q0 + ql] : -INFINITY;
    bj[v] = ql < c.nq ? g.best_j[c.q0 + ql] : -1;
  }

  for (int tile = c.tile_lo; tile < c.tile_hi; ++tile) {
    f32x16 acc[2][2];
    sweep_tile(g.sw, c, tile, L.As, L.Bs, acc);
    const int n0 = tile * TF_BM + c.wm * 64;  // the first gallery row of this wave's part of the tile
    const bool all[2] = {bj[0] < 0, bj[1] < 0};                                // no ground truth: every row of the chunk counts
    const long ti[2] = {bj[0] - g.index_base - n0, bj[1] - g.index_base - n0};  // j* in rows of this wave's part of the tile
    sweep_visit(g.sw, c, tile, acc, [&](int, int v, int, int ql, int row, float s) {
      if (g.sims_out) g.sims_out[(size_t)(c.q0 + ql) * g.lds + n0 + row] = s;
      cnt[v] += (all[v] || before<long>(s, row, bs[v], ti[v])) ? 1 : 0;
    });
  }
  sweep_add_counts(c, cnt, L.cnt, g.beats);
}

// ---------------------------------------------------------------------------------------------------------------- counters
struct RetrKs {
  int k[RT_MAXNK];
  int nk;
};

__global__ __launch_bounds__(256) void retr_count_kernel(const int* beats, int B, const RetrKs ks, unsigned long long* counts, int* rank_out) {
  __shared__ int red[4][RT_MAXNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x * 256 + tid;
  const bool in = b < B;
  const int v = in ? beats[b] : INT_MAX;
  if (rank_out && in) rank_out[b] = v;
#pragma unroll
  for (int m = 0; m < RT_MAXNK; ++m) {
    const int c = __popcll(__ballot((in && m < ks.nk && v < ks.k[m]) ? 1 : 0));
    if (lane == 0) red[wave][m] = c;
  }
  __syncthreads();
  if (tid < ks.nk) {
    const int c = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    if (c) atomicAdd(counts + tid, (unsigned long long)c);
  }
  if (tid == 0 && blockIdx.x == 0) atomicAdd(counts + ks.nk, (unsigned long long)B);
}

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_retr_best(const float* Q, int ldq, const float* X, int ldx, long n_total, const int* gt_ptr, const long* gt_idx, int nnz,
                             int B, int D, float* best_s, long* best_j, void* stream) {
  VTP_REQUIRE(Q && X && gt_ptr && best_s && best_j, "vtp_retr_best: null pointer (Q, X, gt_ptr, best_s, best_j)");
  VTP_REQUIRE(gt_idx || nnz == 0, "vtp_retr_best: null pointer (gt_idx) with nnz != 0");
  VTP_REQUIRE(nnz >= 0 && nnz <= INT_MAX - RT_NB, "vtp_retr_best: need 0 <= nnz <= 2^31 - 65 (nnz=%d)", nnz);
  VTP_REQUIRE(B >= 1, "vtp_retr_best: need B >= 1 (B=%d)", B);
  VTP_REQUIRE(n_total >= 1 && n_total <= INT_MAX, "vtp_retr_best: need 1 <= n_total <= 2^31 - 1: a rank is an int32 (n_total=%ld)", n_total);
  if (sweep_check_rows("vtp_retr_best", "Q", "ldq", Q, ldq, D) != VTP_OK || sweep_check_rows("vtp_retr_best", "X", "ldx", X, ldx, D) != VTP_OK)
    return VTP_ERR_ARG;
  hipLaunchKernelGGL(retr_best_kernel, dim3(nnz / RT_NB + 1), dim3(256), 0, (hipStream_t)stream, Q, ldq, X, ldx, n_total, gt_ptr, gt_idx, nnz,
                     B, D, best_s, best_j);
  return check_launch("retr_best");
}

extern "C" int vtp_retr_rank(const float* Q, int ldq, const float* X, int ldx, long index_base, int B, int N, int D, const float* best_s,
                             const long* best_j, int* beats, int splits, float* sims_out, int lds, void* stream) {
  VTP_REQUIRE(Q && X && best_s && best_j && beats, "vtp_retr_rank: null pointer (Q, X, best_s, best_j, beats)");
  RetrArgs g;
  dim3 grid;
  if (sweep_prepare("vtp_retr_rank", Q, ldq, X, ldx, B, N, D, splits, 1, g.sw, grid) != VTP_OK) return VTP_ERR_ARG;
  VTP_REQUIRE(index_base >= 0 && index_base <= (long)INT_MAX - N,
              "vtp_retr_rank: index_base must be non-negative and index_base + N at most 2^31 - 1 (index_base=%ld)", index_base);
  VTP_REQUIRE(!sims_out || lds >= N, "vtp_retr_rank: sims_out needs lds >= N (lds=%d)", lds);
  g.best_s = best_s, g.best_j = best_j, g.beats = beats, g.sims_out = sims_out;
  g.index_base = index_base, g.lds = lds;
  hipLaunchKernelGGL(retr_rank_kernel, grid, dim3(256), 0, (hipStream_t)stream, g);
  return check_launch("retr_rank");
}

extern "C" int vtp_retr_count(const int* beats, int B, const int* ks, int nk, long* counts, int* rank, long rank_offset, void* stream) {
  VTP_REQUIRE(beats && ks && counts, "vtp_retr_count: null pointer (beats, ks, counts)");
  VTP_REQUIRE(B >= 1, "vtp_retr_count: need B >= 1 (B=%d)", B);
  VTP_REQUIRE(nk >= 1 && nk <= RT_MAXNK, "vtp_retr_count: 1 <= nk <= 8 (nk=%d)", nk);
  VTP_REQUIRE(rank_offset >= 0, "vtp_retr_count: rank_offset must be non-negative (rank_offset=%ld)", rank_offset);
  RetrKs k;
  for (int m = 0; m < nk; ++m) {
    VTP_REQUIRE(ks[m] >= 1 && (m == 0 || ks[m] > ks[m - 1]), "vtp_retr_count: ks must be positive and ascend (ks[%d]=%d)", m, ks[m]);
    k.k[m] = ks[m];
  }
  for (int m = nk; m < RT_MAXNK; ++m) k.k[m] = 0;
  k.nk = nk;
  hipLaunchKernelGGL(retr_count_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, beats, B, k, (unsigned long long*)counts,
                     rank ? rank + rank_offset : nullptr);
  return check_launch("retr_count");
}
