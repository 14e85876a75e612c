// RMSNorm / LayerNorm forward + backward for the fp32 residual stream (HBM-bound, one wave per row).
//   fwd:  y(bf16) = norm(x f32) * w (+ b);  stats[m] = (mean, rstd)    [normalization.py:17-22, nn.LayerNorm]
//   bwd:  dx f32 = dres + d(norm)/dx ;  dw/db accumulated with one atomicAdd per column per workgroup.
// Rows are read as float4 per lane (16 B), row-resident in registers (D <= 2048).
#include "common.h"
#include <cstdlib>
#include <type_traits>
#include "vtp_hip.h"

namespace vtp {

constexpr int NORM_MAXC = 8;  // float4 chunks per lane -> D <= 8*64*4 = 2048 (template NC = ceil(D/256))

template <int KIND, int NC, typename OUT = bf16>  // KIND 0 rms, 1 layernorm; NC float4 chunks per lane; OUT float: the un-rounded output
__global__ __launch_bounds__(256) void norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ b, OUT* __restrict__ y,
                                                       float* __restrict__ stats, int M, int D, float eps,
                                                       uint8_t* __restrict__ y8 = nullptr, const float* __restrict__ q_scale = nullptr,
                                                       const int* __restrict__ m_rows = nullptr) {
  // y8 / q_scale: the fp8 forward path -- the bf16-rounded output leaves as e4m3(y * q_scale[0]) (1 byte per element) instead
  // m_rows: device row limit -- rows >= *m_rows are neither read nor written (the grid is that of the static M)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m_rows) M = min(M, *m_rows);
  if (row >= M) return;
  const float* xr = x + (size_t)row * D;
  f32x4 v[NC];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = (c * 64 + lane) * 4;
    if (col < D) {
      v[c] = *(const f32x4*)(xr + col);
      s += (KIND == 0) ? (v[c][0] * v[c][0] + v[c][1] * v[c][1] + v[c][2] * v[c][2] + v[c][3] * v[c][3])
                       : (v[c][0] + v[c][1] + v[c][2] + v[c][3]);
    }
  }
  s = wave_sum(s);
  float mean = 0.f, rstd;
  if (KIND == 0) {
    rstd = rsqrtf(s / D + eps);
  } else {
    mean = s / D;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = (c * 64 + lane) * 4;
      if (col < D) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = v[c][e] - mean;
          q += d * d;
        }
      }
    }
    q = wave_sum(q);
    rstd = rsqrtf(q / D + eps);
  }
  OUT* yr = y + (size_t)row * D;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = (c * 64 + lane) * 4;
    if (col < D) {
      f32x4 wv = *(const f32x4*)(w + col);
      f32x4 o;
      if (KIND == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[c][e] * rstd * wv[e];
      } else {
        f32x4 bv = *(const f32x4*)(b + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (v[c][e] - mean) * rstd * wv[e] + bv[e];
      }
      if constexpr (std::is_same_v<OUT, float>) {  // the fp32 forward: the value the bf16 output rounds
        *(f32x4*)(yr + col) = o;
        continue;
      }
      const bf16x4 ob = __builtin_convertvector(o, bf16x4);
      if (y8) {
        const float qs = *q_scale;
        const uint32_t wq = pack4_e4m3(bf2f(ob[0]) * qs, bf2f(ob[1]) * qs, bf2f(ob[2]) * qs, bf2f(ob[3]) * qs);  // a NaN stays a NaN code
        *(uint32_t*)(y8 + (size_t)row * D + col) = wq;
      } else if constexpr (!std::is_same_v<OUT, float>) {
        *(bf16x4*)(yr + col) = ob;
      }
    }
  }
  if (lane == 0 && stats) {
    stats[2 * row] = mean;
    stats[2 * row + 1] = rstd;
  }
}

// PV: the rows prow0 + b*pN + t (b < pB, 1 <= t < pN) -- the patch rows of one list item -- take pvec[b] (f32 [pB, D]) on top of
// dy, added in f32 before anything reads dy (the gradient of a mean-pooled feature, spread over the rows it averaged)
// MAPPED: dres is a COMPACT buffer and row r adds dres[dres_rows[r]] (zero when the entry is -1 or out of range): the residual gradient
// of the rows the last block's tail ran on (engine.py), without an expanded f32 copy
template <int KIND, int NC, bool PV = false, bool MAPPED = false>
__global__ __launch_bounds__(256, 2) void norm_bwd_kernel(const bf16* __restrict__ dy, const float* __restrict__ x,
                                                       const float* __restrict__ w, const float* __restrict__ stats,
                                                       const float* __restrict__ dres, float* __restrict__ dx,
                                                       bf16* __restrict__ dxb, float* __restrict__ dw, float* __restrict__ db,
                                                       float* __restrict__ dxsum, int M, int D,
                                                       const float* __restrict__ pvec = nullptr, int prow0 = 0, int pB = 0,
                                                       int pN = 1, const int* __restrict__ dres_rows = nullptr, int dres_M = 0,
                                                       const int* __restrict__ m_rows = nullptr) {
  if (m_rows) M = min(M, *m_rows);  // device row limit: rows >= *m_rows are not read, not written and add nothing to dw / db / dxsum
  constexpr int R = NC <= 3 ? 2 : 1;  // rows in flight per wave: the x / dy loads of all R rows are issued before the first reduction
  const int lane = threadIdx.x & 63;
  const int wv_id = threadIdx.x >> 6;
  // dbacc: LayerNorm bias gradient (column sums of dy) -- or, for RMSNorm (no bias), the column sums of the bf16 OUTPUT
  // (dxsum): the bias gradient of the linear layer whose dy this output is, so that layer needs no separate colsum pass
  f32x4 wreg[NC], dwacc[NC], dbacc[NC], dsacc[KIND == 1 ? NC : 1];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = (c * 64 + lane) * 4;
    if (col < D) wreg[c] = *(const f32x4*)(w + col);
    dwacc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dbacc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (KIND == 1) dsacc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  for (int row0 = (blockIdx.x * 4 + wv_id) * R; row0 < M; row0 += gridDim.x * 4 * R) {
    // narrow rows (NC <= 3): the residual-gradient row is fetched together with x and dy, ahead of the two wave
    // reductions (2 waves/SIMD leave 256 VGPRs per lane); wide rows load it after them to stay inside the budget
    constexpr bool PRE = NC <= 3;
    f32x4 xv[R][NC], dr[PRE ? R : 1][PRE ? NC : 1];
    bf16x4 gy[R][NC];
    float mean[R], rstd[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int row = min(row0 + r, M - 1);
      mean[r] = stats[2 * row];
      rstd[r] = stats[2 * row + 1];
      int drow = row;
      if constexpr (MAPPED && PRE) {
        drow = dres_rows[row];
        if (drow >= dres_M) drow = -1;
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = (c * 64 + lane) * 4;
        if (col < D) {
          xv[r][c] = *(const f32x4*)(x + (size_t)row * D + col);
          gy[r][c] = *(const bf16x4*)(dy + (size_t)row * D + col);
          if constexpr (PRE) {
            if constexpr (MAPPED) dr[r][c] = drow >= 0 ? *(const f32x4*)(dres + (size_t)drow * D + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
            else if (dres) dr[r][c] = *(const f32x4*)(dres + (size_t)row * D + col);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int row = row0 + r;
      if (row >= M) break;
      f32x4 xh[NC], g[NC];
      float s1 = 0.f, s2 = 0.f;
      const float* pv = nullptr;
      if constexpr (PV) {
        const int loc = row - prow0;
        if (loc >= 0 && loc < pB * pN && loc % pN != 0) pv = pvec + (size_t)(loc / pN) * D;
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = (c * 64 + lane) * 4;
        if (col < D) {
          f32x4 gyf = __builtin_convertvector(gy[r][c], f32x4);
          if constexpr (PV) {
            if (pv) gyf += *(const f32x4*)(pv + col);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            xh[c][e] = (xv[r][c][e] - mean[r]) * rstd[r];
            g[c][e] = gyf[e] * wreg[c][e];
            s1 += g[c][e];
            s2 += g[c][e] * xh[c][e];
            dwacc[c][e] += gyf[e] * xh[c][e];
            if (KIND == 1) dbacc[c][e] += gyf[e];
          }
        }
      }
      s2 = wave_sum(s2) / D;
      if (KIND == 1) s1 = wave_sum(s1) / D; else s1 = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = (c * 64 + lane) * 4;
        if (col < D) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = rstd[r] * (g[c][e] - s1 - xh[c][e] * s2);
          if (dres) {
            if constexpr (PRE) o += dr[r][c];
            else if constexpr (MAPPED) {
              const int drow = dres_rows[row];
              o += (drow >= 0 && drow < dres_M) ? *(const f32x4*)(dres + (size_t)drow * D + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
            } else o += *(const f32x4*)(dres + (size_t)row * D + col);
          }
          *(f32x4*)(dx + (size_t)row * D + col) = o;
          if (dxb) {
            const bf16x4 ob = __builtin_convertvector(o, bf16x4);
            *(bf16x4*)(dxb + (size_t)row * D + col) = ob;
            if (dxsum) {
              const f32x4 of = __builtin_convertvector(ob, f32x4);
              if (KIND == 1) dsacc[c] += of; else dbacc[c] += of;
            }
          }
        }
      }
    }
  }
  // reduce dw/db over the 4 waves of the block through LDS, then one atomic per column
  __shared__ float red[4][NC * 256];
  for (int pass = 0; pass < 3; ++pass) {
    // pass 0: dw | pass 1: db (LayerNorm) | pass 2: dxsum (RMSNorm keeps it in dbacc, LayerNorm in dsacc)
    if (pass == 0 && dw == nullptr) continue;
    if (pass == 1 && (KIND == 0 || db == nullptr)) continue;
    if (pass == 2 && (dxsum == nullptr || dxb == nullptr)) continue;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        red[wv_id][(c * 64 + lane) * 4 + e] =
            pass == 0 ? dwacc[c][e] : (pass == 1 ? dbacc[c][e] : (KIND == 1 ? dsacc[KIND == 1 ? c : 0][e] : dbacc[c][e]));
    __syncthreads();
    float* out = pass == 0 ? dw : (pass == 1 ? db : dxsum);
    for (int col = threadIdx.x; col < D; col += 256)
      unsafeAtomicAdd(out + col, red[0][col] + red[1][col] + red[2][col] + red[3][col]);
  }
}

// out[b] = scale * sum_{t=1}^{N-1} x[b*N + t]: one workgroup per (image, 256 columns); its 8 waves take every 8th row, four rows in
// flight per wave, and are summed through LDS in a fixed order (deterministic, no atomics)
constexpr int POOL_WAVES = 8;

template <typename IN>  // bf16 token rows, or the fp32 forward's
__global__ __launch_bounds__(POOL_WAVES * 64) void pool_patch_rows_kernel(const IN* __restrict__ x, float* __restrict__ out, int N,
                                                                         int D, float scale) {
  typedef __attribute__((ext_vector_type(4))) IN in4;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + lane) * 4;
  const int b = blockIdx.y;
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (col < D) {
    const IN* xb = x + (size_t)b * N * D + col;
    int t = 1 + wv;
    for (; t + 3 * POOL_WAVES < N; t += 4 * POOL_WAVES) {
      in4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const in4*)(xb + (size_t)(t + u * POOL_WAVES) * D);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += __builtin_convertvector(v[u], f32x4);
    }
    for (; t < N; t += POOL_WAVES) acc += __builtin_convertvector(*(const in4*)(xb + (size_t)t * D), f32x4);
  }
  __shared__ f32x4 red[POOL_WAVES][64];
  red[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && col < D) {
    f32x4 s = red[0][lane];
#pragma unroll
    for (int k = 1; k < POOL_WAVES; ++k) s += red[k][lane];
    *(f32x4*)(out + (size_t)b * D + col) = s * scale;
  }
}

}  // namespace vtp
using namespace vtp;

// everything norm_fwd_kernel takes (y8 / q_scale: the e4m3 output instead of y; m_rows: device row limit, null = all M rows)
struct NormFwdArgs {
  const float *x, *w, *b;
  bf16* y;
  uint8_t* y8;
  const float* q_scale;
  float* stats;
  int M, D;
  float eps;
  int kind;
  const int* m_rows;
  float* y32 = nullptr;  // the fp32 output instead of y
};

// everything norm_bwd_kernel takes (pvec .. pN: the pooled-vector variant; dres_rows / dres_M: the row-mapped one)
struct NormBwdArgs {
  const bf16* dy;
  const float *x, *w, *stats, *dres;
  float* dx;
  bf16* dxb;
  float *dw, *db, *dxsum;
  int M, D, kind;
  const float* pvec;
  int prow0, pB, pN;
  const int* dres_rows;
  int dres_M;
  const int* m_rows;
};

// the one KIND x NC dispatch: f(KIND, NC) as integral constants, NC = float4 chunks per lane of a D-wide row.  WIDE = false stops at
// NC = 4 (D <= 1024): the pooled-vector and row-mapped backward have no NC = 8 variant -- the wide rows leave no registers for the
// vector's / the mapped read (it spilled ~2 100 VGPRs)
template <bool WIDE, class F>
static void norm_dispatch(int kind, int D, F f) {
  auto by_nc = [&](auto kc) {
    const int nc = cdiv(D, 256);
    if (nc <= 1) f(kc, std::integral_constant<int, 1>{});
    else if (nc == 2) f(kc, std::integral_constant<int, 2>{});
    else if (nc == 3) f(kc, std::integral_constant<int, 3>{});
    else if (!WIDE || nc == 4) f(kc, std::integral_constant<int, 4>{});
    else if constexpr (WIDE) f(kc, std::integral_constant<int, 8>{});
  };
  if (kind == 0) by_nc(std::integral_constant<int, 0>{});
  else by_nc(std::integral_constant<int, 1>{});
}

// A row limit (m_rows, device int) keeps the grid of the static M: rows >= *m_rows are neither read nor written.
static int launch_norm_fwd(const char* who, const char* label, const NormFwdArgs& a, void* stream) {
  VTP_REQUIRE(a.M > 0 && a.D > 0 && a.D % 4 == 0 && a.D <= NORM_MAXC * 256, "%s: need 0 < D <= %d, D %% 4 == 0 (D=%d)", who,
              NORM_MAXC * 256, a.D);
  VTP_REQUIRE(a.kind == 0 || (a.kind == 1 && a.b), "%s: kind must be 0 (rms) or 1 (layernorm, needs bias)", who);
  norm_dispatch<true>(a.kind, a.D, [&](auto kc, auto nc) {
    if (a.y32)
      hipLaunchKernelGGL((norm_fwd_kernel<decltype(kc)::value, decltype(nc)::value, float>), dim3(cdiv(a.M, 4)), dim3(256), 0,
                         (hipStream_t)stream, a.x, a.w, a.b, a.y32, a.stats, a.M, a.D, a.eps, nullptr, nullptr, a.m_rows);
    else
      hipLaunchKernelGGL((norm_fwd_kernel<decltype(kc)::value, decltype(nc)::value>), dim3(cdiv(a.M, 4)), dim3(256), 0, (hipStream_t)stream,
                         a.x, a.w, a.b, a.y, a.stats, a.M, a.D, a.eps, a.y8, a.q_scale, a.m_rows);
  });
  return check_launch(label);
}

static int norm_bwd_blocks(int M, int D) {
  int blocks = cdiv(M, D <= 768 ? 8 : 4);
  // every block ends with one atomic per column and target (dw, db, the column sums of dx): with 1024 blocks that is 1024 adds queued on
  // each of ~2 300 addresses, ~11 us of serialised atomics -- a third of the launch at 8 192 rows.  Fewer, longer-running blocks
  // (tools/norm_bench.py, round 6): 8 192 rows 39.0 -> 25.0 us (256 blocks), 16 448 rows 45.1 -> 39.1, 34 144 rows 87.2 -> 83.7 (512;
  // 256 blocks no longer keep enough loads in flight there), 2 464 rows 15.4 -> 13.3 (128).  VTP_NORM_BWD_BLOCKS=n overrides.
  static int cap_env = -1;
  if (cap_env < 0) {
    const char* e = getenv("VTP_NORM_BWD_BLOCKS");
    cap_env = e && atoi(e) > 0 ? atoi(e) : 0;
  }
  const int cap = cap_env ? cap_env : (M >= 24576 ? 512 : (M >= 4096 ? 256 : 128));
  return blocks > cap ? cap : blocks;
}

// A row limit (m_rows, device int) keeps the grid of the static M: rows >= *m_rows are not read, not written and add nothing to
// dw / db / dx_colsum.
template <bool PV, bool MAPPED>
static int launch_norm_bwd(const char* who, const char* label, const NormBwdArgs& a, void* stream) {
  constexpr bool WIDE = !PV && !MAPPED;
  constexpr int MAXD = WIDE ? NORM_MAXC * 256 : 1024;
  VTP_REQUIRE(!a.dxsum || a.dxb, "%s: dx_colsum sums the bf16 output and needs dx_bf16", who);
  VTP_REQUIRE(a.M > 0 && a.D > 0 && a.D % 4 == 0 && a.D <= MAXD, "%s: need 0 < D <= %d, D %% 4 == 0 (D=%d)", who, MAXD, a.D);
  VTP_REQUIRE(a.kind == 0 || a.kind == 1, "%s: kind must be 0 or 1", who);
  const dim3 grid(norm_bwd_blocks(a.M, a.D));
  norm_dispatch<WIDE>(a.kind, a.D, [&](auto kc, auto nc) {
    hipLaunchKernelGGL((norm_bwd_kernel<decltype(kc)::value, decltype(nc)::value, PV, MAPPED>), grid, dim3(256), 0, (hipStream_t)stream,
                       a.dy, a.x, a.w, a.stats, a.dres, a.dx, a.dxb, a.dw, a.db, a.dxsum, a.M, a.D, a.pvec, a.prow0, a.pB, a.pN,
                       a.dres_rows, a.dres_M, a.m_rows);
  });
  return check_launch(label);
}

extern "C" int vtp_norm_fwd(const float* x, const float* w, const float* b, void* y, float* stats, int M, int D,
                            float eps, int kind, void* stream) {
  VTP_REQUIRE(x && w && y, "vtp_norm_fwd: null pointer");
  return launch_norm_fwd("vtp_norm_fwd", "norm_fwd", {x, w, b, (bf16*)y, nullptr, nullptr, stats, M, D, eps, kind, nullptr}, stream);
}

extern "C" int vtp_norm_fwd_limit(const float* x, const float* w, const float* b, void* y, float* stats, int M, int D, float eps,
                                 int kind, const int* m_rows, void* stream) {
  VTP_REQUIRE(x && w && y && m_rows, "vtp_norm_fwd_limit: null pointer");
  return launch_norm_fwd("vtp_norm_fwd_limit", "norm_fwd_limit", {x, w, b, (bf16*)y, nullptr, nullptr, stats, M, D, eps, kind, m_rows},
                         stream);
}

extern "C" int vtp_norm_fwd_e4m3(const float* x, const float* w, const float* b, void* y8, const float* q_scale, float* stats, int M,
                                 int D, float eps, int kind, void* stream) {
  VTP_REQUIRE(x && w && y8 && q_scale, "vtp_norm_fwd_e4m3: null pointer");
  return launch_norm_fwd("vtp_norm_fwd_e4m3", "norm_fwd_e4m3", {x, w, b, nullptr, (uint8_t*)y8, q_scale, stats, M, D, eps, kind, nullptr},
                         stream);
}

extern "C" int vtp_norm_fwd_f32(const float* x, const float* w, const float* b, float* y, float* stats, int M, int D, float eps, int kind,
                                void* stream) {
  VTP_REQUIRE(x && w && y, "vtp_norm_fwd_f32: null pointer");
  NormFwdArgs a = {x, w, b, nullptr, nullptr, nullptr, stats, M, D, eps, kind, nullptr};
  a.y32 = y;
  return launch_norm_fwd("vtp_norm_fwd_f32", "norm_fwd_f32", a, stream);
}

// the arguments every backward entry has; the variants set their own fields on top
static NormBwdArgs norm_bwd_args(const void* dy, const float* x, const float* w, const float* stats, const float* dres, float* dx,
                                 void* dx_bf16, float* dw, float* db, float* dx_colsum, int M, int D, int kind) {
  return {(const bf16*)dy, x, w, stats, dres, dx, (bf16*)dx_bf16, dw, db, dx_colsum, M, D, kind, nullptr, 0, 0, 1, nullptr, 0, nullptr};
}

extern "C" int vtp_norm_bwd(const void* dy, const float* x, const float* w, const float* stats, const float* dres,
                            float* dx, void* dx_bf16, float* dw, float* db, float* dx_colsum, int M, int D, int kind,
                            void* stream) {
  VTP_REQUIRE(dy && x && w && stats && dx, "vtp_norm_bwd: null pointer");
  return launch_norm_bwd<false, false>("vtp_norm_bwd", "norm_bwd",
                                       norm_bwd_args(dy, x, w, stats, dres, dx, dx_bf16, dw, db, dx_colsum, M, D, kind), stream);
}

// vtp_norm_bwd over the rows [0, min(M, *m_rows)) (m_rows: device int; the grid is that of the static M)
extern "C" int vtp_norm_bwd_limit(const void* dy, const float* x, const float* w, const float* stats, const float* dres, float* dx,
                                  void* dx_bf16, float* dw, float* db, float* dx_colsum, int M, int D, int kind, const int* m_rows,
                                  void* stream) {
  VTP_REQUIRE(dy && x && w && stats && dx && m_rows, "vtp_norm_bwd_limit: null pointer");
  NormBwdArgs a = norm_bwd_args(dy, x, w, stats, dres, dx, dx_bf16, dw, db, dx_colsum, M, D, kind);
  a.m_rows = m_rows;
  return launch_norm_bwd<false, false>("vtp_norm_bwd_limit", "norm_bwd_limit", a, stream);
}

extern "C" int vtp_norm_bwd_pvec(const void* dy, const float* x, const float* w, const float* stats, const float* dres, float* dx,
                                 void* dx_bf16, float* dw, float* db, float* dx_colsum, const float* pvec, int prow0, int pB, int pN,
                                 int M, int D, int kind, void* stream) {
  VTP_REQUIRE(dy && x && w && stats && dx && pvec, "vtp_norm_bwd_pvec: null pointer");
  VTP_REQUIRE(pB > 0 && pN >= 2 && prow0 >= 0 && (long)prow0 + (long)pB * pN <= M,
              "vtp_norm_bwd_pvec: segment rows [%d, %d + %d*%d) must lie in [0, M=%d), N >= 2", prow0, prow0, pB, pN, M);
  NormBwdArgs a = norm_bwd_args(dy, x, w, stats, dres, dx, dx_bf16, dw, db, dx_colsum, M, D, kind);
  a.pvec = pvec; a.prow0 = prow0; a.pB = pB; a.pN = pN;
  return launch_norm_bwd<true, false>("vtp_norm_bwd_pvec", "norm_bwd_pvec", a, stream);
}

extern "C" int vtp_norm_bwd_rows(const void* dy, const float* x, const float* w, const float* stats, const float* dres,
                                 const int* dres_rows, int dres_M, float* dx, void* dx_bf16, float* dw, float* db, float* dx_colsum,
                                 int M, int D, int kind, void* stream) {
  if (!dres_rows)
    return vtp_norm_bwd(dy, x, w, stats, dres, dx, dx_bf16, dw, db, dx_colsum, M, D, kind, stream);
  VTP_REQUIRE(dy && x && w && stats && dx && dres, "vtp_norm_bwd_rows: null pointer (a row map needs dres)");
  VTP_REQUIRE(dres_M > 0, "vtp_norm_bwd_rows: a row map needs dres_M > 0 (dres_M=%d)", dres_M);
  NormBwdArgs a = norm_bwd_args(dy, x, w, stats, dres, dx, dx_bf16, dw, db, dx_colsum, M, D, kind);
  a.dres_rows = dres_rows; a.dres_M = dres_M;
  return launch_norm_bwd<false, true>("vtp_norm_bwd_rows", "norm_bwd_rows", a, stream);
}

extern "C" int vtp_pool_patch_rows(const void* x, float* out, int B, int N, int D, float scale, void* stream) {
  VTP_REQUIRE(x && out, "vtp_pool_patch_rows: null pointer");
  VTP_REQUIRE(B > 0 && N >= 2 && D > 0 && D % 4 == 0, "vtp_pool_patch_rows: need B > 0, N >= 2, D %% 4 == 0 (B=%d N=%d D=%d)", B, N, D);
  VTP_REQUIRE((long)B * N * D < (1L << 40), "vtp_pool_patch_rows: matrix too large");
  hipLaunchKernelGGL(pool_patch_rows_kernel<bf16>, dim3(cdiv(D, 256), B), dim3(POOL_WAVES * 64), 0, (hipStream_t)stream, (const bf16*)x, out,
                     N, D, scale);
  return check_launch("pool_patch_rows");
}

extern "C" int vtp_pool_patch_rows_f32(const float* x, float* out, int B, int N, int D, float scale, void* stream) {
  VTP_REQUIRE(x && out, "vtp_pool_patch_rows_f32: null pointer");
  VTP_REQUIRE(B > 0 && N >= 2 && D > 0 && D % 4 == 0, "vtp_pool_patch_rows_f32: need B > 0, N >= 2, D %% 4 == 0 (B=%d N=%d D=%d)", B, N, D);
  VTP_REQUIRE((long)B * N * D < (1L << 40), "vtp_pool_patch_rows_f32: matrix too large");
  hipLaunchKernelGGL(pool_patch_rows_kernel<float>, dim3(cdiv(D, 256), B), dim3(POOL_WAVES * 64), 0, (hipStream_t)stream, x, out, N, D, scale);
  return check_launch("pool_patch_rows_f32");
}
