// k-NN manifold precision / recall of two feature sets (Kynkaanniemi et al. 2019, the estimate the ADM evaluation suite reports with
// k = 3), restated from the paper's description, as fused exact-fp32 kernels --
//   vtp_pr_sqnorm   : the squared norm of every row, one fmaf chain over k ascending (the bits of the diagonal of vtp_gemm_nt_f32(X, X)).
//   vtp_pr_knn_dist : merges one chunk of a bank into the running lists of the 8 smallest squared distances of a batch of queries.
//                     The radius of a row for neighbourhood size k is column k - 1 of its list against its own set.
//   vtp_pr_cover    : per query, the number of bank rows of a chunk whose ball (squared radius r2) holds the query.
// Neither the [B, N] products nor the distances reach memory (except d2_out, for tests).
//
// Arithmetic.  s(a, b) is the fmaf chain over k = 0 .. D-1 ascending with no split of k, the bits of vtp_gemm_nt_f32; n(a) = s(a, a);
//   d2(a, b) = max((n(a) + n(b)) - 2 s(a, b), 0) with the difference formed by one fmaf(-2, s, n(a) + n(b)) (2 s is exact, so the
//   contraction changes no bit).  d2 is symmetric bit for bit and two identical rows give exactly 0.  The clamp is a select, not
//   fmaxf: a NaN stays a NaN, compares false everywhere and is never selected and never a hit; inputs are finite by contract.
//
// Tile loop: the bank sweep of tile_f32.h -- one walk (sweep_begin / sweep_tile / sweep_visit) that knn.hip and retrieval.hip run
//   as well, around the one tile product (tile_f32_product) that is also the main loop of vtp_gemm_nt_f32.  Grid = bank splits x
//   row blocks of 128 queries; 256 threads.  A workgroup walks its slice of the chunk in tiles of 128 bank rows: 128 x 128 tile, four waves in 2 x 2, each 2 x 2 MFMA tiles of 32 x 32 on v_mfma_f32_32x32x2_f32, K slabs of 16
//   staged through LDS transposed ([k][row]), two buffers, the loads of slab t + 1 in flight under the MFMAs of slab t.  The bank
//   rows are the A operand and the queries the B operand, so a query sits on a lane and its candidates are accumulator registers.
//   The tile's 128 bank norms (and radii) go through LDS, two buffers by tile parity; a lane's two query norms stay in registers.
// Selection (pr_knn_kernel).  A lane keeps an ascending 8-list per query in registers (2 x 8 VGPRs, static indices only).  A value
//   is inserted only when it beats the list's last entry, through an unrolled compare-exchange chain.  After the slice's last tile
//   the four lane-lists of a query (wm x half) are merged through LDS (4 x 8 x 128 floats = 16 KiB) and written to the workspace as
//   the split's partial list.  pr_fold_kernel folds the split lists and the incoming dist into the new dist, one thread per query.
//   Only values are kept, no indices: the 8 smallest values of a multiset do not depend on order, so the result is identical bit
//   for bit whatever the chunking of the bank, the splits, B or the grid, and two different rows at the same distance both stay.
//   Self-exclusion is by index (query_base + b == index_base + n), not by value: a duplicate elsewhere in the set counts, at 0.
// Cover (pr_cover_kernel).  The epilogue compares each d2 with the bank row's r2 (<=) and counts per lane; the four lane-sets of a
//   query are summed in LDS and one integer atomicAdd per query and workgroup reaches memory: exact and order-free.
// LDS: operand slabs 2 x 2 x 16 x 132 x 4 B = 33 KiB, norms and radii 2 KiB, merge lists 16 KiB: 51 KiB, two workgroups per CU.
//
// Known and left out: the set-against-itself passes (real x real, fake x fake: about 70 % of the work at the ADM sizes) compute a
//   symmetric matrix in full.  Exploiting the symmetry would halve them; it is out of scope here.
#include "common.h"
#include "mfma_f32.h"
#include "tile_f32.h"
#include "vtp_hip.h"

#include <limits.h>
#include <math.h>

namespace vtp {

constexpr int PR_K = 8;                              // list length (PR_MAX_K)
constexpr int PR_NB = 64;  // rows per workgroup of pr_sqnorm_kernel, queries per workgroup of pr_fold_kernel

struct PrArgs {
  SweepArgs sw;
  const float *qn, *xn, *r2;
  float* part;  // [splits][B][8]
  float* d2_out;
  int* hits;
  long excl;  // index_base - query_base (global bank row - global query row of an excluded pair); LONG_MIN: no exclusion
  int ldo;
};

struct PrLds {
  float As[2][TF_BK][TF_LD];  // bank rows
  float Bs[2][TF_BK][TF_LD];  // queries
  float xn[2][TF_BM];         // by tile parity
  float r2[2][TF_BM];
  union {
    float lists[4][PR_K][TF_BQ];  // [wm * 2 + half][entry][query]
    int cnt[4][TF_BQ];
  };
};

// x into the ascending list l if it beats the last entry: x takes the last place and sinks through compare-exchanges
__device__ __forceinline__ void pr_insert(float (&l)[PR_K], float x) {
  if (x < l[PR_K - 1]) {
    l[PR_K - 1] = x;
#pragma unroll
    for (int i = PR_K - 1; i > 0; --i) {
      const float lo = l[i] < l[i - 1] ? l[i] : l[i - 1];
      const float hi = l[i] < l[i - 1] ? l[i - 1] : l[i];
      l[i - 1] = lo, l[i] = hi;
    }
  }
}

template <bool COVER>
__device__ __forceinline__ void pr_body(const PrArgs& g, PrLds& L) {
  const SweepCtx c = sweep_begin(g.sw);
  const int tid = threadIdx.x, split = blockIdx.x;
  // this lane's two queries c.query(v): norm, and the state of the epilogue
  float qn[2], lst[2][PR_K];
  int cnt[2] = {0, 0};
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int ql = c.query(v);
    qn[v] = ql < c.nq ? g.qn[c.q0 + ql] : 0.f;
#pragma unroll
    for (int i = 0; i < PR_K; ++i) lst[v][i] = INFINITY;
  }

  for (int tile = c.tile_lo; tile < c.tile_hi; ++tile) {
    const int n0 = tile * TF_BM, par = tile & 1;
    // the norms and radii of the tile's bank rows: read behind the barriers of the tile product; the other parity may still be in use
    // by a wave that is in the epilogue of the tile before
    if (tid < TF_BM) {
      const bool in = n0 + tid < g.sw.N;
      L.xn[par][tid] = in ? g.xn[n0 + tid] : 0.f;
      if (COVER) L.r2[par][tid] = in ? g.r2[n0 + tid] : 0.f;
    }
    f32x16 acc[2][2];
    sweep_tile(g.sw, c, tile, L.As, L.Bs, acc);

    const int w0 = c.wm * 64;  // the first row of this wave's part of the tile
    // the excluded pair of each query, in rows of this wave's part of the tile (-1: none here)
    int ex[2] = {-1, -1};
    if (!COVER && g.excl != LONG_MIN) {
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const long e = (long)(c.q0 + c.query(v)) - g.excl - n0 - w0;
        ex[v] = (e >= 0 && e < 64) ? (int)e : -1;
      }
    }
    sweep_visit(g.sw, c, tile, acc, [&](int, int v, int, int ql, int row, float s) {
      float d = fmaf(-2.f, s, qn[v] + L.xn[par][w0 + row]);
      d = d < 0.f ? 0.f : d;
      if (COVER) {
        cnt[v] += d <= L.r2[par][w0 + row] ? 1 : 0;
      } else {
        if (g.d2_out) g.d2_out[(size_t)(c.q0 + ql) * g.ldo + n0 + w0 + row] = d;
        if (row != ex[v]) pr_insert(lst[v], d);
      }
    });
  }

  // the four lane-sets of a query (wm x half) meet in LDS: `lists` / `cnt` are touched nowhere else
  if (COVER) {
    sweep_add_counts(c, cnt, L.cnt, g.hits);
  } else {
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int i = 0; i < PR_K; ++i) L.lists[c.wm * 2 + c.half][i][c.query(v)] = lst[v][i];
    __syncthreads();
    if (tid < c.nq) {
      float m[PR_K];
#pragma unroll
      for (int i = 0; i < PR_K; ++i) m[i] = L.lists[0][i][tid];
#pragma unroll
      for (int s = 1; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < PR_K; ++i) pr_insert(m, L.lists[s][i][tid]);
      f32x4* out = (f32x4*)(g.part + ((size_t)split * g.sw.B + c.q0 + tid) * PR_K);
      out[0] = f32x4{m[0], m[1], m[2], m[3]};
      out[1] = f32x4{m[4], m[5], m[6], m[7]};
    }
  }
}

__global__ __launch_bounds__(256, 2) void pr_knn_kernel(const PrArgs g) {
  __shared__ __attribute__((aligned(16))) PrLds L;
  pr_body<false>(g, L);
}

__global__ __launch_bounds__(256, 2) void pr_cover_kernel(const PrArgs g) {
  __shared__ __attribute__((aligned(16))) PrLds L;
  pr_body<true>(g, L);
}

// one thread per query: dist <- the 8 smallest of (dist, split list 0, split list 1, ...)
__global__ __launch_bounds__(PR_NB) void pr_fold_kernel(float* dist, const float* part, int B, int splits) {
  const int b = blockIdx.x * PR_NB + threadIdx.x;
  if (b >= B) return;
  float m[PR_K];
#pragma unroll
  for (int i = 0; i < PR_K; ++i) m[i] = INFINITY;
  const f32x4* d4 = (const f32x4*)(dist + (size_t)b * PR_K);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x4 x = d4[h];
#pragma unroll
    for (int e = 0; e < 4; ++e) pr_insert(m, x[e]);
  }
  for (int s = 0; s < splits; ++s) {
    const f32x4* p4 = (const f32x4*)(part + ((size_t)s * B + b) * PR_K);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 x = p4[h];
#pragma unroll
      for (int e = 0; e < 4; ++e) pr_insert(m, x[e]);
    }
  }
  f32x4* o4 = (f32x4*)(dist + (size_t)b * PR_K);
  o4[0] = f32x4{m[0], m[1], m[2], m[3]};
  o4[1] = f32x4{m[4], m[5], m[6], m[7]};
}

// 64 rows per workgroup: slabs of 64 columns are loaded coalesced into LDS, thread r < 64 walks row r with one fmaf chain over k
// ascending.  Columns past D are zeros: fmaf(0, 0, acc) = acc.
__global__ __launch_bounds__(256) void pr_sqnorm_kernel(const float* X, int ldx, int N, int D, float* out) {
  __shared__ float t[PR_NB][PR_NB + 1];
  const int tid = threadIdx.x, r0 = blockIdx.x * PR_NB;
  float acc = 0.f;
  for (int k0 = 0; k0 < D; k0 += PR_NB) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int e = tid + 256 * it, r = e >> 4, c = 4 * (e & 15);
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (r0 + r < N && k0 + c < D) x = *(const f32x4*)(X + (size_t)(r0 + r) * ldx + k0 + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) t[r][c + i] = x[i];
    }
    __syncthreads();
    if (tid < PR_NB) {
#pragma unroll 8
      for (int k = 0; k < PR_NB; ++k) acc = fmaf(t[tid][k], t[tid][k], acc);
    }
    __syncthreads();
  }
  if (tid < PR_NB && r0 + tid < N) out[r0 + tid] = acc;
}

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_pr_workspace_bytes(int B, int splits) {
  VTP_REQUIRE(B >= 1 && splits >= 0 && splits <= SWEEP_MAX_SPLITS, "vtp_pr_workspace_bytes: need B >= 1, 0 <= splits <= 1024 (B=%d splits=%d)", B,
              splits);
  const int s = sweep_max_splits(B, splits);
  const long bytes = (long)s * B * PR_K * 4;
  VTP_REQUIRE(bytes <= INT_MAX, "vtp_pr_workspace_bytes: the workspace of B=%d splits=%d exceeds 2 GiB: pass fewer queries per call", B, s);
  return (int)bytes;
}

extern "C" int vtp_pr_sqnorm(const float* X, int ldx, int N, int D, float* out, void* stream) {
  VTP_REQUIRE(X && out, "vtp_pr_sqnorm: null pointer (X, out)");
  VTP_REQUIRE(N >= 1, "vtp_pr_sqnorm: need N >= 1 (N=%d)", N);
  if (sweep_check_rows("vtp_pr_sqnorm", "X", "ldx", X, ldx, D) != VTP_OK) return VTP_ERR_ARG;
  hipLaunchKernelGGL(pr_sqnorm_kernel, dim3(cdiv(N, PR_NB)), dim3(256), 0, (hipStream_t)stream, X, ldx, N, D, out);
  return check_launch("pr_sqnorm");
}

extern "C" int vtp_pr_knn_dist(const float* Q, int ldq, const float* qn, const float* X, int ldx, const float* xn, long query_base,
                               long index_base, int B, int N, int D, float* dist, void* workspace, long workspace_bytes, int splits,
                               float* d2_out, int ldo, void* stream) {
  VTP_REQUIRE(Q && qn && X && xn && dist && workspace, "vtp_pr_knn_dist: null pointer (Q, qn, X, xn, dist, workspace)");
  PrArgs g;
  dim3 grid;
  if (sweep_prepare("vtp_pr_knn_dist", Q, ldq, X, ldx, B, N, D, splits, 1, g.sw, grid) != VTP_OK) return VTP_ERR_ARG;
  VTP_REQUIRE(aligned16(dist) && aligned16(workspace), "vtp_pr_knn_dist: dist and workspace must be 16-byte aligned");
  VTP_REQUIRE(query_base >= -1 && query_base <= LONG_MAX - B, "vtp_pr_knn_dist: query_base must be -1 (no exclusion) or a row index (query_base=%ld)",
              query_base);
  VTP_REQUIRE(index_base >= 0 && index_base <= LONG_MAX - N, "vtp_pr_knn_dist: index_base must be non-negative (index_base=%ld)", index_base);
  VTP_REQUIRE(!d2_out || ldo >= N, "vtp_pr_knn_dist: d2_out needs ldo >= N (ldo=%d)", ldo);
  const int s = grid.x;
  const long need = (long)s * B * PR_K * 4;
  VTP_REQUIRE(workspace_bytes >= need, "vtp_pr_knn_dist: workspace of %ld bytes, %ld needed (vtp_pr_workspace_bytes)", workspace_bytes, need);
  g.qn = qn, g.xn = xn, g.r2 = nullptr;
  g.part = (float*)workspace, g.d2_out = d2_out, g.hits = nullptr;
  g.excl = query_base < 0 ? LONG_MIN : index_base - query_base;
  g.ldo = ldo;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pr_knn_kernel, grid, dim3(256), 0, st, g);
  const int rc = check_launch("pr_knn");
  if (rc != VTP_OK) return rc;
  hipLaunchKernelGGL(pr_fold_kernel, dim3(cdiv(B, PR_NB)), dim3(PR_NB), 0, st, dist, (const float*)g.part, B, s);
  return check_launch("pr_fold");
}

extern "C" int vtp_pr_cover(const float* Q, int ldq, const float* qn, const float* X, int ldx, const float* xn, const float* r2, int B,
                            int N, int D, int* hits, int splits, void* stream) {
  VTP_REQUIRE(Q && qn && X && xn && r2 && hits, "vtp_pr_cover: null pointer (Q, qn, X, xn, r2, hits)");
  PrArgs g;
  dim3 grid;
  if (sweep_prepare("vtp_pr_cover", Q, ldq, X, ldx, B, N, D, splits, 1, g.sw, grid) != VTP_OK) return VTP_ERR_ARG;
  g.qn = qn, g.xn = xn, g.r2 = r2;
  g.part = nullptr, g.d2_out = nullptr, g.hits = hits;
  g.excl = LONG_MIN;
  g.ldo = 0;
  hipLaunchKernelGGL(pr_cover_kernel, grid, dim3(256), 0, (hipStream_t)stream, g);
  return check_launch("pr_cover");
}
