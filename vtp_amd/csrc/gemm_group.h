// Argument records of the grouped weight-gradient launches: the 8-phase kernel (gemm8p.hip, vtp_gemm_tn_grouped) runs a uniform
// tiles x splits grid, the one-wave-per-SIMD kernel (gemm4w_tn.hip, vtp_gemm_tn_grouped_items) a host-built work-item list.
#pragma once
#include "gemm_common.h"

namespace vtp {

struct GroupProblem {  // 64-bit fields: written by the host as an int64 tensor
  const bf16* A;
  const bf16* B;
  float* C;
  float* colsum;
  long lda, ldb, ldc;
  long M, N;
  long c_grp, c_pre;
  long tile0;       // first tile of this problem in the launch's tile list
  long accumulate;  // 1: C += result, 0: C = result
  long K;           // token rows of THIS problem (item-list launches only: its items cut [0, K)); 0 = GroupArgs.K
  long pad[2];
};
struct GroupItem {  // one workgroup of an item-list launch (vtp_gemm_tn_grouped_items): 8 x int32, written by the host
  int tile;           // index in the launch's tile list
  int kbeg, kcount;   // its K range (kbeg a multiple of 64, kcount of 8)
  int nparts, part;   // workgroups sharing the tile, and this one's slot among them
  int pad[3];
};
struct GroupArgs {
  const GroupProblem* probs;
  float* part;
  int* ticket;
  int nprob, ntiles, splits, K, k_split;  // splits: slices per tile (8-phase kernel) | partial-sum slots per tile (item lists)
  unsigned long long* timing;
  const GroupItem* items;  // one-wave-per-SIMD kernel: one record per workgroup, never null | 8-phase kernel: unused (null)
  // 8-phase kernel, one K slice only (vtp_gemm_tn_grouped_limit): device count of the token rows that hold data -- every problem sums
  // over rows [0, min(K, *k_rows)) and no row beyond them is read.  null: off.  The item-list kernel does not read it.
  const int* k_rows;
};

}  // namespace vtp
