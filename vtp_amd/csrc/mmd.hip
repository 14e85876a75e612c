// The pair sums of the Kernel Inception Distance (Binkowski et al. 2018: the unbiased MMD^2 of two feature sets under the polynomial
// kernel k(x, y) = (gamma x.y + coef0)^degree), restated from the paper's definition, as fused kernels on the exact-fp32 tile product --
//   vtp_mmd_poly_part : per tile of 128 bank rows and per query the sum of k(q_b, x_n) over the tile's rows.
//   vtp_mmd_fold      : rowsum[p][b] += part[p][t][b], t ascending, one owner thread per element.
//   vtp_mmd_total     : total[p] = the sum of rowsum[p][0 .. B) by a fixed tree.
// The [B, N] products and kernel values never reach memory.  No atomics, neither float nor double.
//
// Value of a pair.  s = the fmaf chain over k = 0 .. D-1 ascending with no split of k (tile_f32_product: the bits of vtp_gemm_nt_f32),
//   then in fp64 with every operation rounded on its own (the build contracts a * b + c, so nothing here is written that way):
//   t = (double)s * gamma + coef0 (two roundings), k = t, multiplied by t a further degree - 1 times, left to right.
// Left out (skipped, not added as zero): the pair whose absolute positions coincide (query_base + b == index_base + n, query_base >=
//   0; with index lists the position in the list counts, not the gathered row), bank rows past N, queries past B.
// Index lists.  xi / qi int32 [P, N] / [P, B], null meaning identity: row n of problem p's bank is row xi[p][n] of X, query b is row
//   qi[p][b] of Q.  The gather is the pointer set-up of the tile loads; an index outside the matrix is read as a row of zeros.
//
// ORDER OF THE SUMS (the one place it is written; tests/mmd_ref.py restates it).
//   Tile product: grid = (bank tiles, row blocks of 128 queries, problems), one workgroup = one 128 x 128 tile, four waves in 2 x 2
//   (wm, wn).  Lane (j, half) of wave (wm, wn) holds for its query wn * 64 + v * 32 + j the 32 tile rows
//       row(set, step) = wm * 64 + u * 32 + (r & 3) + 8 (r >> 2) + 4 half,   set = wm * 2 + half, step = u * 16 + r, u < 2, r < 16.
//   part: a lane starts at +0.0 and adds the values of its rows in ascending step; the four sets of a query meet in LDS and are
//     added as ((set 0 + set 1) + set 2) + set 3.  A tile covers the absolute bank rows index_base + 128 tile ..., and index_base is a
//     multiple of 128: the same rows whatever the chunking of the bank.
//   fold: rowsum += part[t] for t = 0, 1, ... of the chunk; chunks are fed in ascending order, so a row sum is the left-to-right sum
//     of its tiles' parts in ascending absolute tile order.
//   total: neighbours are paired level by level: level l + 1 holds a[2 i] + a[2 i + 1] of level l, an odd last element moves up
//     unchanged, until one is left.  The shape depends on B alone.  (Run as: aligned blocks of 512 elements reduced in LDS, then the
//     same tree over the block sums -- an aligned power-of-two block is a subtree, so this is the tree above.)
//   Every sum is __dadd_rn.  Row sums and totals repeat bit for bit whatever the chunk size, the queries per pass or the card.
#include "common.h"
#include "mfma_f32.h"
#include "tile_f32.h"
#include "vtp_hip.h"

#include <limits.h>

#pragma clang fp contract(off)

namespace vtp {

constexpr int MMD_MAX_DEGREE = 8;
constexpr int MMD_NB = 64;                     // elements per workgroup of mmd_fold_kernel
constexpr int MMD_TB = 512, MMD_TOP = 4096;    // block of the total's tree in LDS, and the most blocks: B <= 512 * 4096

struct MmdArgs {
  SweepArgs sw;  // tiles_per_split = 1: blockIdx.x is the tile
  const int *qi, *xi;
  int q_rows, x_rows;
  long excl;  // index_base - query_base; LONG_MIN: no exclusion
  double gamma, coef0;
  int degree;
  double* part;  // [P][tiles][B]
};

struct MmdLds {
  float As[2][TF_BK][TF_LD];  // bank rows
  float Bs[2][TF_BK][TF_LD];  // queries
  double sets[4][TF_BQ];      // [wm * 2 + half][query]
};

__global__ __launch_bounds__(256, 2) void mmd_poly_part_kernel(const MmdArgs g) {
  __shared__ __attribute__((aligned(16))) MmdLds L;
  SweepCtx c = sweep_begin(g.sw);
  const int tid = threadIdx.x, tile = blockIdx.x, p = blockIdx.z, n0 = tile * TF_BM;
  const float* ap[TF_IT];
#pragma unroll
  for (int it = 0; it < TF_IT; ++it) {
    const int r = c.lr[it];
    if (g.qi) {
      const int row = r < c.nq ? g.qi[(size_t)p * g.sw.B + c.q0 + r] : -1;
      c.bp[it] = (row >= 0 && row < g.q_rows) ? g.sw.Q + (size_t)row * g.sw.ldq + 4 * c.kq : nullptr;
    }
    int row = n0 + r < g.sw.N ? n0 + r : -1;
    if (g.xi && row >= 0) {
      row = g.xi[(size_t)p * g.sw.N + row];
      if (row >= g.x_rows) row = -1;
    }
    ap[it] = row >= 0 ? g.sw.X + (size_t)row * g.sw.ldx + 4 * c.kq : nullptr;
  }
  f32x16 acc[2][2];
  tile_f32_product(ap, c.bp, c.lr, c.kq, g.sw.D, L.As, L.Bs, c.wm, c.wn, c.j, c.half, acc);

  const int w0 = c.wm * 64;
  // the excluded pair of each query, in rows of this wave's part of the tile (-1: none here)
  int ex[2] = {-1, -1};
  if (g.excl != LONG_MIN) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const long e = (long)(c.q0 + c.query(v)) - g.excl - n0 - w0;
      ex[v] = (e >= 0 && e < 64) ? (int)e : -1;
    }
  }
  double sum[2] = {0.0, 0.0};
  const double gamma = g.gamma, coef0 = g.coef0;
  const int degree = g.degree;
  sweep_visit(g.sw, c, tile, acc, [&](int, int v, int, int, int row, float s) {
    if (row != ex[v]) {
      const double t = __dadd_rn(__dmul_rn((double)s, gamma), coef0);
      double k = t;
      for (int i = 1; i < degree; ++i) k = __dmul_rn(k, t);
      sum[v] = __dadd_rn(sum[v], k);
    }
  });
  // the four lane-sets of a query meet in LDS (`sets` is touched nowhere else), added in ascending set order
#pragma unroll
  for (int v = 0; v < 2; ++v) L.sets[c.wm * 2 + c.half][c.query(v)] = sum[v];
  __syncthreads();
  if (tid < c.nq) {
    const double a = __dadd_rn(__dadd_rn(__dadd_rn(L.sets[0][tid], L.sets[1][tid]), L.sets[2][tid]), L.sets[3][tid]);
    g.part[((size_t)p * g.sw.tiles + tile) * g.sw.B + c.q0 + tid] = a;
  }
}

// one thread per element of rowsum [P, B]
__global__ __launch_bounds__(MMD_NB) void mmd_fold_kernel(const double* part, double* rowsum, int B, int tiles) {
  const int b = blockIdx.x * MMD_NB + threadIdx.x, p = blockIdx.y;
  if (b >= B) return;
  double a = rowsum[(size_t)p * B + b];
  for (int t = 0; t < tiles; ++t) a = __dadd_rn(a, part[((size_t)p * tiles + t) * B + b]);
  rowsum[(size_t)p * B + b] = a;
}

// a[0] <- the neighbour-pair tree over a[0 .. n) in LDS: at stride s the element 2 s i takes in the element 2 s i + s if there is one
__device__ __forceinline__ void mmd_tree(double* a, int n) {
  for (int s = 1; s < n; s *= 2) {
    for (int i = threadIdx.x;; i += 256) {
      const long lo = 2L * s * i;
      if (lo + s >= n) break;
      a[lo] = __dadd_rn(a[lo], a[lo + s]);
    }
    __syncthreads();
  }
}

// one workgroup per problem
__global__ __launch_bounds__(256) void mmd_total_kernel(const double* rowsum, int B, double* total) {
  __shared__ double blk[MMD_TB], top[MMD_TOP];
  const int tid = threadIdx.x, p = blockIdx.x, nblk = (B + MMD_TB - 1) / MMD_TB;
  const double* src = rowsum + (size_t)p * B;
  for (int bi = 0; bi < nblk; ++bi) {
    const int b0 = bi * MMD_TB, cnt = B - b0 < MMD_TB ? B - b0 : MMD_TB;
    for (int i = tid; i < cnt; i += 256) blk[i] = src[b0 + i];
    __syncthreads();
    mmd_tree(blk, cnt);
    if (tid == 0) top[bi] = blk[0];
    __syncthreads();
  }
  mmd_tree(top, nblk);
  if (tid == 0) total[p] = top[0];
}

static inline long mmd_part_bytes(int B, int N, int P) { return (long)P * cdiv(N, TF_BM) * B * 8; }

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_mmd_workspace_bytes(int B, int N, int P) {
  VTP_REQUIRE(B >= 1 && N >= 1 && P >= 1, "vtp_mmd_workspace_bytes: need B, N, P >= 1 (B=%d N=%d P=%d)", B, N, P);
  const long tiles = cdiv(N, TF_BM);
  VTP_REQUIRE((long)P * tiles <= INT_MAX / 8 / B, "vtp_mmd_workspace_bytes: the workspace of B=%d N=%d P=%d exceeds 2 GiB: pass fewer rows per call",
              B, N, P);
  return (int)mmd_part_bytes(B, N, P);
}

extern "C" int vtp_mmd_poly_part(const float* Q, int ldq, int q_rows, const int* qi, const float* X, int ldx, int x_rows, const int* xi,
                                 long query_base, long index_base, int B, int N, int D, int P, const double* kparams, int degree,
                                 double* part, long part_bytes, void* stream) {
  const char* fn = "vtp_mmd_poly_part";
  VTP_REQUIRE(Q && X && kparams && part, "%s: null pointer (Q, X, kparams, part)", fn);
  VTP_REQUIRE(B >= 1 && N >= 1 && P >= 1, "%s: need B, N, P >= 1 (B=%d N=%d P=%d)", fn, B, N, P);
  if (sweep_check_rows(fn, "Q", "ldq", Q, ldq, D) != VTP_OK || sweep_check_rows(fn, "X", "ldx", X, ldx, D) != VTP_OK) return VTP_ERR_ARG;
  VTP_REQUIRE(degree >= 1 && degree <= MMD_MAX_DEGREE, "%s: degree must be 1 .. 8 (degree=%d)", fn, degree);
  VTP_REQUIRE(query_base >= -1 && query_base <= LONG_MAX - B, "%s: query_base must be -1 (no exclusion) or a row index (query_base=%ld)", fn,
              query_base);
  VTP_REQUIRE(index_base >= 0 && index_base <= LONG_MAX - N && index_base % TF_BM == 0,
              "%s: index_base must be a non-negative multiple of 128 (index_base=%ld)", fn, index_base);
  VTP_REQUIRE((!qi || q_rows >= 1) && (!xi || x_rows >= 1), "%s: an index list needs the row count of its matrix (q_rows=%d x_rows=%d)", fn, q_rows,
              x_rows);
  const int rb = cdiv(B, TF_BQ), tiles = cdiv(N, TF_BM);
  VTP_REQUIRE(rb <= 65535 && P <= 65535, "%s: B or P too large (B=%d P=%d)", fn, B, P);
  VTP_REQUIRE((long)P * tiles <= LONG_MAX / 8 / B && part_bytes >= mmd_part_bytes(B, N, P),
              "%s: part of %ld bytes, P * tiles * B * 8 needed (vtp_mmd_workspace_bytes)", fn, part_bytes);
  MmdArgs g;
  g.sw = SweepArgs{Q, X, ldq, ldx, B, N, D, tiles, 1};
  g.qi = qi, g.xi = xi, g.q_rows = q_rows, g.x_rows = x_rows;
  g.excl = query_base < 0 ? LONG_MIN : index_base - query_base;
  g.gamma = kparams[0], g.coef0 = kparams[1];
  g.degree = degree;
  g.part = part;
  hipLaunchKernelGGL(mmd_poly_part_kernel, dim3(tiles, rb, P), dim3(256), 0, (hipStream_t)stream, g);
  return check_launch("mmd_poly_part");
}

extern "C" int vtp_mmd_fold(const double* part, double* rowsum, int B, int tiles, int P, void* stream) {
  VTP_REQUIRE(part && rowsum, "vtp_mmd_fold: null pointer (part, rowsum)");
  VTP_REQUIRE(B >= 1 && tiles >= 1 && P >= 1 && P <= 65535, "vtp_mmd_fold: need B, tiles >= 1 and 1 <= P <= 65535 (B=%d tiles=%d P=%d)", B, tiles, P);
  hipLaunchKernelGGL(mmd_fold_kernel, dim3(cdiv(B, MMD_NB), P), dim3(MMD_NB), 0, (hipStream_t)stream, part, rowsum, B, tiles);
  return check_launch("mmd_fold");
}

extern "C" int vtp_mmd_total(const double* rowsum, int B, int P, double* total, void* stream) {
  VTP_REQUIRE(rowsum && total, "vtp_mmd_total: null pointer (rowsum, total)");
  VTP_REQUIRE(B >= 1 && B <= MMD_TB * MMD_TOP && P >= 1, "vtp_mmd_total: need 1 <= B <= 2097152 and P >= 1 (B=%d P=%d)", B, P);
  hipLaunchKernelGGL(mmd_total_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, rowsum, B, total);
  return check_launch("mmd_total");
}
