// Weighted k-NN classification on frozen, L2-normalised features (the DINO / DINOv2 evaluation protocol, restated from the papers'
// description: k = 10, 20, 100, 200, temperature 0.07, top-1 and top-5) as fused exact-fp32 kernels --
//   vtp_knn_topk : merges one chunk of the bank into the running K-neighbour lists of a batch of queries.  The similarities
//                  are formed tile by tile and never reach memory; replaces a chunked torch.matmul + topk + merge.
//   vtp_knn_vote : neighbour lists -> weighted class votes, rank of every target, top-1 / top-5 / row counters, in one launch;
//                  replaces softmax + one_hot + cumsum + topk(5) + eq + sum.
//
// vtp_knn_topk, first kernel (knn_topk_kernel).  Grid = bank splits x row blocks of 128 queries; 256 threads.
//   Tile.  A workgroup walks its slice of the chunk in tiles of 128 bank rows (the bank sweep of tile_f32.h, the one walk that
//     precision_recall.hip and retrieval.hip run as well) and computes S^T[bank row][query] = X Q^T with the main loop of
//     vtp_gemm_nt_f32 itself (tile_f32_product, which fp32.hip calls too): 128 x 128 tile, four waves in 2 x 2, each
//     2 x 2 MFMA tiles of 32 x 32 on v_mfma_f32_32x32x2_f32, K slabs of 16 staged through LDS transposed ([k][row]), two buffers,
//     the loads of slab t + 1 in flight under the MFMAs of slab t.  The bank rows are the A operand and the queries the B
//     operand, so a query sits on a lane and its candidates are accumulator registers.  A product is commutative and the chain
//     runs over k = 0 .. D-1 ascending with no split of k: s[b, n] has the bits of element [b, n] of vtp_gemm_nt_f32(Q, X) with
//     the plain epilogue, whatever B, N, the tile, the chunk or the grid.
//   Selection.  Every query of the row block has a threshold in LDS: its current K-th neighbour (similarity, global index), or
//     (-inf, -1) while the list is short.  A lane compares its 64 accumulator values with the thresholds of its two queries; a
//     survivor is appended to the query's LDS buffer (32 entries: similarity and row within the chunk; the slot comes from an LDS
//     integer atomic).  A survivor that finds the buffer full stays pending in its register: the workgroup then merges every
//     non-empty buffer into its list, refreshes the thresholds and lets the pending survivors try again -- nothing is ever dropped,
//     so any buffer size is correct.  Buffers are also merged after the slice's last tile.  Survivors are rare once the lists are
//     full, so most tiles cost 64 compares per lane and one barrier.
//   Lists.  The sorted lists live in GLOBAL memory (the workspace: one [B, K] list pair per split), not in LDS: at K = 256 a row
//     block's lists are 128 x 256 x 12 B = 384 KiB.  The row block does not shrink with K.  One wave merges one query: the list
//     is staged into a per-wave LDS scratch, every element's new position is (its old position + the buffered survivors before
//     it), a survivor's position is (list elements before it, by binary search) + (survivors before it); positions >= K fall off.
//   LDS at any K (sized for K = 256): operand slabs 2 x 2 x 16 x 132 x 4 B = 33 KiB, survivor buffers 128 x 32 x 8 B = 32 KiB,
//     merge scratch 4 x 256 x 8 B = 8 KiB, thresholds and counts 2 KiB: 75 KiB of the CU's 160 KiB, two workgroups per CU.
//   Second kernel (knn_merge_kernel): one workgroup per query folds the split lists, in split order, into the incoming state with
//     a stable two-list merge by binary search in LDS; above 8 splits in two stages (groups of about sqrt(splits) lists first).
//   Order.  The K neighbours are the first K bank rows under (similarity descending, global index ascending) -- a total order,
//     since indices are distinct.  Buffers fill in whatever order the atomics land, but every merge sorts by the total order and
//     a threshold is only ever a lower bound of the final K-th neighbour, so the lists are identical bit for bit whatever the number
//     of splits, the chunking of the bank, B or the launch geometry.  NaN compares false with every threshold and is never selected;
//     inputs are finite by contract (a similarity of -inf is indistinguishable from an empty entry).
//   Empty entries are (-inf, -1) and sit at the end of a list; there is no separate count.
//
// vtp_knn_vote: one wave per query.  Neighbour j has weight w_j = expf((s_j - s_0) * inv_T) (the softmax of the protocol without
//   its common denominator: same ranking).  The lane that holds the first neighbour of a class owns that class and adds the class's
//   weights in neighbour order, so a score is the same fp32 sum run to run; the scores at k_1 < k_2 < ... are prefixes of one
//   chain.  There is no [B, C] array: classes without a neighbour have score 0 and are ranked by index, which is arithmetic.
//   Only integer atomics touch the counters.
#include "common.h"
#include "mfma_f32.h"
#include "tile_f32.h"
#include "vtp_hip.h"

#include <limits.h>
#include <math.h>

namespace vtp {

constexpr int KN_CAP = 32;  // buffered survivors per query between two merges
constexpr int KN_MAXK = 256;
constexpr int KN_MERGE_FLAT = 8;  // up to this many splits one merge stage
constexpr int KN_MIN_TILES = 8;   // tiles a split keeps (sweep_splits): its lists are zeroed, merged through memory and folded

// wave-level ordering of LDS traffic: what the lanes of this wave wrote is visible to its other lanes afterwards
__device__ __forceinline__ void kn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct KnnArgs {
  SweepArgs sw;
  float* part_s;  // [splits][B][K]
  long* part_i;   // [splits][B][K]
  float* sims_out;
  long index_base;
  int lds, K;
};

struct KnnLds {
  float As[2][TF_BK][TF_LD];  // bank rows
  float Bs[2][TF_BK][TF_LD];  // queries
  float cand_s[TF_BQ][KN_CAP];
  int cand_n[TF_BQ][KN_CAP];  // row within the chunk
  long thr_i[TF_BQ];
  float ls_s[4][KN_MAXK];
  int ls_n[4][KN_MAXK];  // row within the chunk
  float thr_s[TF_BQ];
  int cnt[TF_BQ];
};

// wave `wave` merges the buffers of its 32 queries (wave * 32 ...) into their lists.  The list of the next query is on its way
// from memory while the current one is merged.
__device__ __forceinline__ void knn_merge_buffers(const KnnArgs& g, KnnLds& L, int q0, int split, int wave, int lane) {
  float ns[4];
  long ni[4];
  auto fetch = [&](int i) {
    const int ql = wave * 32 + i;
    if (L.cnt[ql] == 0) return;  // the same for every lane; a query past B never has a survivor
    const size_t off = ((size_t)split * g.sw.B + (q0 + ql)) * g.K;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int p = lane + 64 * t;
      ns[t] = -INFINITY, ni[t] = -1;
      if (p < g.K) ns[t] = g.part_s[off + p], ni[t] = g.part_i[off + p];
    }
  };
#pragma unroll
  for (int t = 0; t < 4; ++t) ns[t] = -INFINITY, ni[t] = -1;
  fetch(0);
  for (int i = 0; i < 32; ++i) {
    const int ql = wave * 32 + i;
    float es[4];
    long ei[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) es[t] = ns[t], ei[t] = ni[t];
    if (i + 1 < 32) fetch(i + 1);
    const int n = L.cnt[ql] < KN_CAP ? L.cnt[ql] : KN_CAP;  // the same for every lane
    if (n == 0) continue;
    const size_t off = ((size_t)split * g.sw.B + (q0 + ql)) * g.K;
    float* ps = g.part_s + off;
    long* pi = g.part_i + off;
    // within one call every list entry is a row of this chunk: orders are compared on the 32-bit row, not the 64-bit index
    int el[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int p = lane + 64 * t;
      el[t] = ei[t] < 0 ? -1 : (int)(ei[t] - g.index_base);
      if (p < g.K) L.ls_s[wave][p] = es[t], L.ls_n[wave][p] = el[t];
    }
    float cs = -INFINITY;
    int cn = INT_MAX;
    if (lane < n) cs = L.cand_s[ql][lane], cn = L.cand_n[ql][lane];
    kn_wave_sync();
    int ahead[4] = {0, 0, 0, 0}, crank = 0;
    for (int c = 0; c < n; ++c) {  // survivor c, broadcast from its lane's registers
      const float xs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cs), c));
      const int xn = __builtin_amdgcn_readlane(cn, c);
#pragma unroll
      for (int t = 0; t < 4; ++t) ahead[t] += before(xs, xn, es[t], el[t]) ? 1 : 0;
      crank += before(xs, xn, cs, cn) ? 1 : 0;
    }
    int cpos = g.K;
    if (lane < n) {
      int lo = 0, hi = g.K;  // the number of list elements before the survivor
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (before(L.ls_s[wave][mid], L.ls_n[wave][mid], cs, cn)) lo = mid + 1;
        else hi = mid;
      }
      cpos = lo + crank;
    }
    const long ci = g.index_base + cn;
    kn_wave_sync();  // every read of the scratch and the buffer is done
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int p = lane + 64 * t, np = p + ahead[t];
      if (p < g.K && np < g.K) {
        ps[np] = es[t], pi[np] = ei[t];
        if (np == g.K - 1) L.thr_s[ql] = es[t], L.thr_i[ql] = ei[t];
      }
    }
    if (cpos < g.K) {
      ps[cpos] = cs, pi[cpos] = ci;
      if (cpos == g.K - 1) L.thr_s[ql] = cs, L.thr_i[ql] = ci;
    }
    if (lane == 0) L.cnt[ql] = 0;
    kn_wave_sync();
  }
}

__global__ __launch_bounds__(256, 2) void knn_topk_kernel(const KnnArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds_raw[];
  KnnLds& L = *reinterpret_cast<KnnLds*>(knn_lds_raw);
  const SweepCtx c = sweep_begin(g.sw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = c.half;
  const int split = blockIdx.x, q0 = c.q0;

  // this workgroup's lists start empty
  {
    float* ps = g.part_s + ((size_t)split * g.sw.B + q0) * g.K;
    long* pi = g.part_i + ((size_t)split * g.sw.B + q0) * g.K;
    for (int e = tid; e < c.nq * g.K; e += 256) ps[e] = -INFINITY, pi[e] = -1;
    if (tid < TF_BQ) L.thr_s[tid] = -INFINITY, L.thr_i[tid] = -1, L.cnt[tid] = 0;
  }
  __syncthreads();

  for (int tile = c.tile_lo; tile < c.tile_hi; ++tile) {
    f32x16 acc[2][2];
    sweep_tile(g.sw, c, tile, L.As, L.Bs, acc);
    const int n0 = tile * TF_BM + c.wm * 64;  // the first bank row of this wave's part of the tile

    if (g.sims_out)
      sweep_visit(g.sw, c, tile, acc, [&](int, int, int, int ql, int row, float s) { g.sims_out[(size_t)(q0 + ql) * g.lds + n0 + row] = s; });

    // bit (u * 2 + v) * 16 + r: the value is inside the chunk and the batch and has not been decided yet
    unsigned long long pend = 0;
    sweep_visit(g.sw, c, tile, acc, [&](int u, int v, int r, int, int, float) { pend |= 1ull << ((u * 2 + v) * 16 + r); });
    const bool last = tile + 1 == c.tile_hi;
    for (;;) {
      // what is behind its query's threshold is decided for good: the threshold only rises.  Every value is compared, inside
      // the chunk or not (`pend` knows): the thresholds are read again on every turn, so this loop is not a sweep_visit
      unsigned long long pass = 0;
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const float ts = L.thr_s[c.query(v)];
        const long ti = L.thr_i[c.query(v)] - g.index_base - n0;  // in rows of this wave's part of the tile
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (before<long>(acc[u][v][r], u * 32 + acc_row(r, half), ts, ti)) pass |= 1ull << ((u * 2 + v) * 16 + r);
      }
      pend &= pass;
      // the survivors, one at a time (rare once the lists are full): the register is picked by a select chain
      bool full = false;
#pragma unroll 1
      for (unsigned long long todo = pend; todo; todo &= todo - 1) {
        const int bit = __builtin_ctzll(todo);
        const int ql = c.query((bit >> 4) & 1);
        if (L.cnt[ql] >= KN_CAP) {  // full already: wait for the merge
          full = true;
          continue;
        }
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 64; ++e) s = bit == e ? acc[e >> 5][(e >> 4) & 1][e & 15] : s;
        const int slot = atomicAdd(&L.cnt[ql], 1);
        if (slot < KN_CAP) {
          L.cand_s[ql][slot] = s;
          L.cand_n[ql][slot] = n0 + (bit >> 5) * 32 + acc_row(bit & 15, half);
          pend &= ~(1ull << bit);
        } else {
          full = true;  // stays pending: the merge below makes room and raises the threshold
        }
      }
      const int any_full = __syncthreads_or(full ? 1 : 0);
      if (!any_full && !last) break;
      knn_merge_buffers(g, L, q0, split, wave, lane);
      __syncthreads();
      if (!any_full) break;
    }
  }
}

// One workgroup per (query, group): dst <- first K of (dst, src 0, src 1, ...), two lists at a time.  Element t of dst goes to
// t + #(src elements strictly before it), element t of the src list to t + #(dst elements not after it): a stable merge, every
// position below K is written exactly once.  Stage 1 (many splits only): group y folds the split lists y * per + 1 .. y * per +
// per - 1 into the split list y * per, in place.  Stage 2: the group heads (or all split lists), in split order, into the state.
// The first K of a union does not depend on how the union is bracketed, so the stages change no bit.
__global__ __launch_bounds__(256) void knn_merge_kernel(float* dst_s, long* dst_i, long dst_group_stride,
                                                        const float* part_s, const long* part_i, int B, int K, int first, int per,
                                                        int step, int splits) {
  __shared__ float as[KN_MAXK], bs[KN_MAXK];
  __shared__ long ai[KN_MAXK], bi[KN_MAXK];
  const int t = threadIdx.x, b = blockIdx.x, grp = blockIdx.y;
  float* ds = dst_s + grp * dst_group_stride + (size_t)b * K;
  long* di = dst_i + grp * dst_group_stride + (size_t)b * K;
  if (t < K) as[t] = ds[t], ai[t] = di[t];
  for (int jn = first; jn < per; ++jn) {
    const int s = (grp * per + jn) * step;
    if (s >= splits) break;
    const size_t off = ((size_t)s * B + b) * K;
    if (t < K) bs[t] = part_s[off + t], bi[t] = part_i[off + t];
    __syncthreads();
    float xs = 0.f, ys = 0.f;
    long xi = 0, yi = 0;
    int px = K, py = K;
    if (t < K && bi[0] >= 0) {  // an empty list changes nothing
      xs = as[t], xi = ai[t], ys = bs[t], yi = bi[t];
      int lo = 0, hi = K;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (before(bs[mid], bi[mid], xs, xi)) lo = mid + 1;
        else hi = mid;
      }
      px = t + lo;
      lo = 0, hi = K;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!before(ys, yi, as[mid], ai[mid])) lo = mid + 1;
        else hi = mid;
      }
      py = t + lo;
    }
    __syncthreads();
    if (px < K) as[px] = xs, ai[px] = xi;
    if (py < K) as[py] = ys, ai[py] = yi;
    __syncthreads();
  }
  if (t < K) ds[t] = as[t], di[t] = ai[t];
}

// ---------------------------------------------------------------------------------------------------------------- votes
constexpr int KV_MAXNK = 8;

struct KnnVoteArgs {
  const float* sims;
  const long* idx;
  const int* labels;
  const long* targets;
  unsigned long long* counts;
  int* rank_out;
  int* pred_out;
  long n_total;
  int ks[KV_MAXNK];
  int nk, num_classes, B, K;
  float inv_T;
};

// class order: before() on (score, class index) -- score descending, lower class index first among equals
__global__ __launch_bounds__(64) void knn_vote_kernel(const KnnVoteArgs g) {
  __shared__ int lab_s[KN_MAXK];
  __shared__ float w_s[KN_MAXK];
  const int lane = threadIdx.x, b = blockIdx.x, K = g.K, C = g.num_classes;
  const int kmax = g.ks[g.nk - 1];
  const long tl = g.targets[b];
  const int tgt = (tl >= 0 && tl < C) ? (int)tl : -1;
  const float s0 = g.sims[(size_t)b * K];
  // neighbour lane + 64 t: its label (-1: an empty entry, or a label outside [0, C) -- it votes for nothing) and weight
  int lab[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int jn = lane + 64 * t;
    lab[t] = -1;
    if (jn < kmax) {
      const long i = g.idx[(size_t)b * K + jn];
      const int l = (i >= 0 && i < g.n_total) ? g.labels[i] : -1;
      lab[t] = (l >= 0 && l < C) ? l : -1;
      lab_s[jn] = lab[t];
      w_s[jn] = lab[t] >= 0 ? expf((g.sims[(size_t)b * K + jn] - s0) * g.inv_T) : 0.f;
    }
  }
  __syncthreads();
  // the first neighbour of a class owns the class
  bool own[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) own[t] = lab[t] >= 0;
  for (int i = 0; i < kmax; ++i) {
    const int li = lab_s[i];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (i < lane + 64 * t && li == lab[t]) own[t] = false;
  }
  float score[4] = {0.f, 0.f, 0.f, 0.f};
  int m = 0;
  for (int i = 0; i < kmax; ++i) {
    const int li = lab_s[i];
    const float wi = w_s[i];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (own[t] && li == lab[t]) score[t] += wi;  // neighbour order: one fixed chain per class
    if (g.ks[m] != i + 1) continue;
    const int k = i + 1;
    // the classes seen among the first k neighbours: owners at a position below k
    bool act[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) act[t] = own[t] && lane + 64 * t < k;
    float st = -1.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (act[t] && lab[t] == tgt) st = score[t];
    st = wave_max(st);
    if (st < 0.f) st = 0.f;  // no neighbour of the target's class: score 0
    int ahead = 0, below = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      ahead += (act[t] && before(score[t], lab[t], st, tgt)) ? 1 : 0;
      below += (act[t] && lab[t] < tgt) ? 1 : 0;
    }
    ahead = wave_sum_int(ahead);
    below = wave_sum_int(below);
    // at score 0 every class without a neighbour and with a lower index is ranked before the target as well
    const int rank = tgt < 0 ? C : ahead + (st == 0.f ? tgt - below : 0);
    if (lane == 0) {
      if (g.rank_out) g.rank_out[(size_t)b * g.nk + m] = rank;
      if (g.counts) {
        if (rank < 1) atomicAdd(g.counts + 3 * m + 0, 1ull);
        if (rank < 5) atomicAdd(g.counts + 3 * m + 1, 1ull);
        atomicAdd(g.counts + 3 * m + 2, 1ull);
      }
    }
    if (g.pred_out) {
      // five rounds: the first class in class order strictly after the pick of the round before, among the classes seen and the
      // unseen ones (score 0, ascending index, from `unseen` on)
      float pv = INFINITY;
      int pc = -1, unseen = 0;
#pragma unroll 1
      for (int q = 0; q < 5; ++q) {
        float mv = 0.f;
        int mc = INT_MAX;  // INT_MAX: nothing found
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (act[t] && before(pv, pc, score[t], lab[t]) && (mc == INT_MAX || before(score[t], lab[t], mv, mc))) mv = score[t], mc = lab[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float xv = __shfl_xor(mv, o, 64);
          const int xc = __shfl_xor(mc, o, 64);
          if (xc != INT_MAX && (mc == INT_MAX || before(xv, xc, mv, mc))) mv = xv, mc = xc;
        }
        if (mc == INT_MAX || mv == 0.f) {  // an unseen class may come first
          for (; unseen < C; ++unseen) {
            bool seen = false;
#pragma unroll
            for (int t = 0; t < 4; ++t) seen = seen || (act[t] && lab[t] == unseen);
            if (!__any(seen ? 1 : 0)) break;
          }
          if (unseen < C && (mc == INT_MAX || !before(mv, mc, 0.f, unseen))) mv = 0.f, mc = unseen++;
        }
        if (lane == 0) g.pred_out[((size_t)b * g.nk + m) * 5 + q] = mc == INT_MAX ? -1 : mc;
        pv = mc == INT_MAX ? -INFINITY : mv, pc = mc;
      }
    }
    if (++m == g.nk) break;
  }
}

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_knn_workspace_bytes(int B, int K, int splits) {
  VTP_REQUIRE(B >= 1 && K >= 1 && K <= KN_MAXK && splits >= 0 && splits <= SWEEP_MAX_SPLITS,
              "vtp_knn_workspace_bytes: need B >= 1, 1 <= K <= 256, 0 <= splits <= 1024 (B=%d K=%d splits=%d)", B, K, splits);
  const int s = sweep_max_splits(B, splits);
  const long bytes = (long)s * B * K * 12;
  VTP_REQUIRE(bytes <= INT_MAX, "vtp_knn_workspace_bytes: the workspace of B=%d K=%d splits=%d exceeds 2 GiB: pass fewer queries per call", B, K, s);
  return (int)bytes;
}

extern "C" int vtp_knn_topk(const float* Q, int ldq, const float* X, int ldx, long index_base, int B, int N, int D, int K, float* sims,
                            long* idx, void* workspace, long workspace_bytes, int splits, float* sims_out, int lds, void* stream) {
  VTP_REQUIRE(Q && X && sims && idx && workspace, "vtp_knn_topk: null pointer (Q, X, sims, idx, workspace)");
  VTP_REQUIRE(K >= 1 && K <= KN_MAXK, "vtp_knn_topk: need 1 <= K <= 256 (K=%d)", K);
  KnnArgs g;
  dim3 grid;
  if (sweep_prepare("vtp_knn_topk", Q, ldq, X, ldx, B, N, D, splits, KN_MIN_TILES, g.sw, grid) != VTP_OK) return VTP_ERR_ARG;
  VTP_REQUIRE(aligned16(workspace), "vtp_knn_topk: workspace must be 16-byte aligned");
  VTP_REQUIRE(index_base >= 0 && index_base <= LONG_MAX - N, "vtp_knn_topk: index_base must be non-negative (index_base=%ld)", index_base);
  VTP_REQUIRE(!sims_out || lds >= N, "vtp_knn_topk: sims_out needs lds >= N (lds=%d)", lds);
  const int s = grid.x;
  const long need = (long)s * B * K * 12;
  VTP_REQUIRE(workspace_bytes >= need, "vtp_knn_topk: workspace of %ld bytes, %ld needed (vtp_knn_workspace_bytes)", workspace_bytes, need);
  g.part_i = (long*)workspace;  // the 8-byte entries first: both parts stay aligned
  g.part_s = (float*)((long*)workspace + (size_t)s * B * K);
  g.sims_out = sims_out;
  g.index_base = index_base;
  g.lds = lds, g.K = K;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)knn_topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(KnnLds));
    attr = true;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(knn_topk_kernel, grid, dim3(256), sizeof(KnnLds), st, g);
  const int rc = check_launch("knn_topk");
  if (rc != VTP_OK) return rc;
  int per = 1;  // split lists per group of the first merge stage: about sqrt(splits)
  while (per * per < s) ++per;
  if (s <= KN_MERGE_FLAT) per = 1;
  if (per > 1) {
    hipLaunchKernelGGL(knn_merge_kernel, dim3(B, cdiv(s, per)), dim3(256), 0, st, g.part_s, g.part_i, (long)per * B * K, g.part_s, g.part_i, B, K,
                       1, per, 1, s);
    const int rc1 = check_launch("knn_merge (groups)");
    if (rc1 != VTP_OK) return rc1;
  }
  hipLaunchKernelGGL(knn_merge_kernel, dim3(B, 1), dim3(256), 0, st, sims, idx, 0L, g.part_s, g.part_i, B, K, 0, cdiv(s, per), per, s);
  return check_launch("knn_merge");
}

extern "C" int vtp_knn_vote(const float* sims, const long* idx, const int* labels, long n_total, const long* targets, const int* ks, int nk,
                            float inv_T, int num_classes, int B, int K, long* counts, int* rank_out, int* pred_out, void* stream) {
  VTP_REQUIRE(sims && idx && labels && targets && ks, "vtp_knn_vote: null pointer (sims, idx, labels, targets, ks)");
  VTP_REQUIRE(B >= 1 && K >= 1 && K <= KN_MAXK && n_total >= 1, "vtp_knn_vote: need B >= 1, 1 <= K <= 256, n_total >= 1 (B=%d K=%d)", B, K);
  VTP_REQUIRE(nk >= 1 && nk <= KV_MAXNK, "vtp_knn_vote: 1 <= nk <= 8 (nk=%d)", nk);
  VTP_REQUIRE(num_classes >= 5, "vtp_knn_vote: num_classes >= 5 (the top-5 of fewer classes does not exist)");
  KnnVoteArgs g;
  for (int m = 0; m < nk; ++m) {
    VTP_REQUIRE(ks[m] >= 1 && ks[m] <= K && (m == 0 || ks[m] > ks[m - 1]), "vtp_knn_vote: ks must ascend within [1, K] (ks[%d]=%d, K=%d)", m,
                ks[m], K);
    g.ks[m] = ks[m];
  }
  for (int m = nk; m < KV_MAXNK; ++m) g.ks[m] = 0;
  g.sims = sims, g.idx = idx, g.labels = labels, g.targets = targets;
  g.counts = (unsigned long long*)counts, g.rank_out = rank_out, g.pred_out = pred_out;
  g.n_total = n_total, g.nk = nk, g.num_classes = num_classes, g.B = B, g.K = K, g.inv_T = inv_T;
  hipLaunchKernelGGL(knn_vote_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, g);
  return check_launch("knn_vote");
}
