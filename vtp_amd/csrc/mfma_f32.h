// The f32-input MFMA v_mfma_f32_32x32x2_f32 as the exact-fp32 kernels use it -- the LDS-staged 128 x 128 tile of tile_f32.h (fp32.hip,
// knn.hip, precision_recall.hip, retrieval.hip, mmd.hip), the one-wave tiles of wave_f32.h (probe.hip, segprobe.hip, zeroshot.hip) and
// the convolution of fid.hip: bit-for-bit a k-ordered fmaf chain per output element, one rounding per product, the same chain whichever tile or lane the element
// sits in.
//   operand maps (one f32 VGPR each): lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31];
//   C/D: column j = l & 31, row i = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5), reg in [0, 16).
#pragma once
#include "common.h"

namespace vtp {

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

}  // namespace vtp
