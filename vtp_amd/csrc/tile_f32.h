// The 128 x 128 exact-fp32 tile product, written once: the main loop of vtp_gemm_nt_f32 (fp32.hip) and of the bank sweeps of knn.hip,
// precision_recall.hip and retrieval.hip, which call it with the bank rows as the A operand and the queries as the B operand, so a
// query sits on a lane and its candidates are accumulator registers.  256 threads, four waves in 2 x 2 (wm, wn), each 2 x 2 MFMA
// tiles of 32 x 32 on v_mfma_f32_32x32x2_f32 (four independent accumulators keep the matrix pipe at its issue rate), K slabs of 16
// staged through LDS transposed ([k][row], so the lanes of an MFMA operand read consecutive words), two buffers, the loads of slab
// t + 1 in flight under the MFMAs of slab t: one barrier per slab.  The chain of an element runs over k = 0 .. D-1 ascending with no
// split of k, so its bits depend on its two rows alone -- every caller gets the bits of vtp_gemm_nt_f32 with the plain epilogue.
//   result: lane (j = lane & 31, half = lane >> 5) of wave (wm, wn) holds in acc[u][v][r] the product of the A row
//   wm * 64 + u * 32 + acc_row(r, half) with the B row wn * 64 + v * 32 + j of the tile.
// Below the product: the walk of a bank sweep (which tiles a workgroup takes, which query and bank row an accumulator value belongs
// to, the integer sum over the four lane-sets of a query) and the host prologue of the sweeps' entry points.
#pragma once
#include "common.h"
#include "mfma_f32.h"

namespace vtp {

constexpr int TF_BM = 128, TF_BQ = 128, TF_BK = 16;  // A rows (bank rows) per tile, B rows (queries) per tile, K slab
constexpr int TF_KQ = TF_BK / 4;                     // 16-byte loads per tile row and slab
constexpr int TF_IT = TF_KQ / 2;                     // loads per thread, operand and slab: 128 rows x TF_KQ / 256 threads
constexpr int TF_LD = 128 + 16 / TF_KQ;              // 4 * TF_LD % 32 == 64 / TF_KQ: the TF_KQ k groups of a wave's write land on disjoint banks twice over

// Thread tid loads the 16 bytes at column 4 * kq (kq = tid & (TF_KQ - 1)) of the tile rows lr[it] = tid / TF_KQ + (256 / TF_KQ) * it:
// ap[it] / bp[it] point there in the A / B operand, or are null for a row outside the operand (read as zeros); so is k past D (D % 4
// == 0 keeps a 16-byte load inside its row; a zero product leaves the chain's value unchanged).
// Every thread of the workgroup calls this; it ends behind a barrier, so the slabs are free again when it returns.
__device__ __forceinline__ void tile_f32_product(const float* const (&ap)[TF_IT], const float* const (&bp)[TF_IT], const int (&lr)[TF_IT],
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

// ---------------------------------------------------------------------------------------------------------------- the bank sweep
// Grid = bank splits x row blocks of 128 queries.  A workgroup walks the tiles [tile_lo, tile_hi) of the chunk X[N, D] against its
// queries Q[q0 .. q0 + nq); a split past the last tile walks nothing.  KnnArgs, PrArgs and RetrArgs begin with these arguments.
struct SweepArgs {
  const float *Q, *X;
  int ldq, ldx, B, N, D, tiles, tiles_per_split;
};

struct SweepCtx {
  int wm, wn, j, half, kq;     // the thread's place in the tile product
  int q0, nq;                  // the row block's first query and its number of queries
  int tile_lo, tile_hi;        // the split's tiles
  const float* bp[TF_IT];      // the thread's query loads
  int lr[TF_IT];               // and their tile rows
  __device__ __forceinline__ int query(int v) const { return wn * 64 + v * 32 + j; }  // the lane's local query v = 0, 1
};

__device__ __forceinline__ SweepCtx sweep_begin(const SweepArgs& g) {
  SweepCtx c;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, split = blockIdx.x;
  c.wm = wave >> 1, c.wn = wave & 1, c.j = lane & 31, c.half = lane >> 5, c.kq = tid & (TF_KQ - 1);
  c.q0 = blockIdx.y * TF_BQ;
  c.nq = g.B - c.q0 < TF_BQ ? g.B - c.q0 : TF_BQ;
#pragma unroll
  for (int it = 0; it < TF_IT; ++it) {
    const int r = tid / TF_KQ + (256 / TF_KQ) * it;
    c.lr[it] = r;
    c.bp[it] = r < c.nq ? g.Q + (size_t)(c.q0 + r) * g.ldq + 4 * c.kq : nullptr;
  }
  c.tile_lo = split * g.tiles_per_split;
  c.tile_hi = c.tile_lo + g.tiles_per_split < g.tiles ? c.tile_lo + g.tiles_per_split : g.tiles;
  return c;
}

// the products of the bank rows tile * 128 ... with the row block's queries
__device__ __forceinline__ void sweep_tile(const SweepArgs& g, const SweepCtx& c, int tile, float (&As)[2][TF_BK][TF_LD],
                                           float (&Bs)[2][TF_BK][TF_LD], f32x16 (&acc)[2][2]) {
  const int n0 = tile * TF_BM;
  const float* ap[TF_IT];
#pragma unroll
  for (int it = 0; it < TF_IT; ++it) ap[it] = n0 + c.lr[it] < g.N ? g.X + (size_t)(n0 + c.lr[it]) * g.ldx + 4 * c.kq : nullptr;
  tile_f32_product(ap, c.bp, c.lr, c.kq, g.D, As, Bs, c.wm, c.wn, c.j, c.half, acc);
}

// The lane's values of a tile that lie inside the batch and the chunk, query by query: f(u, v, r, ql, row, value) with the local
// query ql = c.query(v) and the bank row `row` = u * 32 + acc_row(r, half) within the wave's part of the tile (bank row n0 + wm * 64
// + row of the chunk).  Fully unrolled: u, v, r are constants in the body and the accumulator is never indexed at run time.
template <typename F>
__device__ __forceinline__ void sweep_visit(const SweepArgs& g, const SweepCtx& c, int tile, const f32x16 (&acc)[2][2], F&& f) {
  const int rows_left = g.N - tile * TF_BM - c.wm * 64;  // rows of this wave's part of the tile inside the chunk
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int ql = c.query(v);
    if (ql >= c.nq) continue;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = u * 32 + acc_row(r, c.half);
        if (row < rows_left) f(u, v, r, ql, row, acc[u][v][r]);
      }
  }
}

// The four lane-sets of a query (wm x half) each counted their part of the bank rows in cnt[v]: they meet in LDS (`lds` is touched
// nowhere else) and one integer atomicAdd per query and workgroup reaches out[q0 + query] -- exact and order-free.
__device__ __forceinline__ void sweep_add_counts(const SweepCtx& c, const int (&cnt)[2], int (&lds)[4][TF_BQ], int* out) {
#pragma unroll
  for (int v = 0; v < 2; ++v) lds[c.wm * 2 + c.half][c.query(v)] = cnt[v];
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < c.nq) {
    const int n = lds[0][tid] + lds[1][tid] + lds[2][tid] + lds[3][tid];
    if (n) atomicAdd(out + c.q0 + tid, n);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
constexpr int SWEEP_MAX_SPLITS = 1024, SWEEP_AUTO_SPLITS = 256, SWEEP_AUTO_BLOCKS = 512;

// the most sweep_splits takes for this B, whatever N: what a workspace with one part per split is sized for
static inline int sweep_max_splits(int B, int splits) {
  if (splits > 0) return splits;
  const int s = cdiv(SWEEP_AUTO_BLOCKS, cdiv(B, TF_BQ));
  return s > SWEEP_AUTO_SPLITS ? SWEEP_AUTO_SPLITS : s;
}

// The split count of a call: the forced one, or enough workgroups to fill the chip twice (two fit a CU) as long as a split keeps
// min_tiles tiles; splits that would get no tile are dropped.  min_tiles weighs what a split costs beyond its tiles: 1 where that is
// a sum or a 16 KiB merge in LDS (at a bank of 10 000 rows, 79 tiles, a minimum of 8 left two thirds of the chip idle), 8 for the
// K-lists of vtp_knn_topk, which are zeroed, merged through memory and folded per split.
static inline int sweep_splits(int B, int N, int splits, int min_tiles) {
  if (splits > 0) return splits;
  const int tiles = cdiv(N, TF_BM);
  int s = sweep_max_splits(B, 0);
  if (s > tiles / min_tiles) s = tiles / min_tiles;
  if (s < 1) s = 1;
  return cdiv(tiles, cdiv(tiles, s));
}

// one row operand P[rows, D] of a 16-byte-loading kernel; `fn` is the entry point's name, `name` / `ld_name` those of the arguments
static inline int sweep_check_rows(const char* fn, const char* name, const char* ld_name, const float* P, int ld, int D) {
  VTP_REQUIRE(D >= 8 && D % 8 == 0, "%s: need D a positive multiple of 8 (D=%d)", fn, D);
  VTP_REQUIRE(ld >= D && ld % 4 == 0, "%s: the leading dimension must cover the rows, %s a multiple of 4 (%s=%d)", fn, ld_name, ld_name, ld);
  VTP_REQUIRE(aligned16(P), "%s: %s must be 16-byte aligned", fn, name);
  return VTP_OK;
}

// The prologue of a sweep's entry point `fn`: the checks of the common arguments, the split count (grid.x), the grid and the
// common arguments of the kernel.
static inline int sweep_prepare(const char* fn, const float* Q, int ldq, const float* X, int ldx, int B, int N, int D, int splits,
                                int min_tiles, SweepArgs& g, dim3& grid) {
  VTP_REQUIRE(B >= 1 && N >= 1, "%s: need B, N >= 1 (B=%d N=%d)", fn, B, N);
  if (sweep_check_rows(fn, "Q", "ldq", Q, ldq, D) != VTP_OK || sweep_check_rows(fn, "X", "ldx", X, ldx, D) != VTP_OK) return VTP_ERR_ARG;
  VTP_REQUIRE(splits >= 0 && splits <= SWEEP_MAX_SPLITS, "%s: 0 <= splits <= 1024 (splits=%d)", fn, splits);
  const int rb = cdiv(B, TF_BQ);
  VTP_REQUIRE(rb <= 65535, "%s: B too large (B=%d)", fn, B);
  const int s = sweep_splits(B, N, splits, min_tiles), tiles = cdiv(N, TF_BM);
  g = SweepArgs{Q, X, ldq, ldx, B, N, D, tiles, cdiv(tiles, s)};
  grid = dim3(s, rb);
  return VTP_OK;
}

}  // namespace vtp
