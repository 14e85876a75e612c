// The fp32 inference forward (Stack._forward_fp32): every linear map and the attention in exact fp32 on the f32-input MFMA
// (mfma_f32.h: v_mfma_f32_32x32x2_f32, bit for bit one fmaf chain per output element).
//   vtp_gemm_nt_f32 : C[M,N] = epi(A[M,K] W[N,K]^T), fp32 in and out.  One accumulator per output element over the whole of K in
//                     ascending k, no split of K: an element's bits depend on its row of A and its row of W alone -- not on M, the
//                     tile it falls in or the batch it came with.
//   vtp_attn_fwd_f32: softmax(Q K^T scale) V, head dimension 64, fp32 in and out, online softmax; both products on the same MFMA, no
//                     atomics, one wave per 32 query rows; a query's result depends on its own sequence alone.
#include "common.h"
#include "mfma_f32.h"
#include "tile_f32.h"
#include "vtp_hip.h"

#include <math.h>

namespace vtp {

// ---------------------------------------------------------------------------------------------------------------- GEMM
// Workgroup = 128 x 128 output tile, computed by tile_f32_product (tile_f32.h: the one main loop, which the bank sweeps of knn.hip,
// precision_recall.hip and retrieval.hip call as well): four waves in 2 x 2, each 2 x 2 MFMA tiles of 32 x 32, K in slabs of 16
// through two transposed LDS buffers, one barrier per slab.  The kernel chooses the rows: A rows m0 .. and W rows n0 .. of the
// tile, null (read as zeros) past M / N.
// SwiGLU: the tile's 128 W rows are 64 rows of w1 and the same 64 rows of w2, laid out so that a wave's tile column 0 is x1 and its
// tile column 1 is x2 of the same hidden columns: the epilogue pairs acc[.][0] with acc[.][1] lane by lane and the block covers 64
// hidden columns.
constexpr int GF_BM = TF_BM, GF_BN = TF_BQ;  // the output tile; the K slab and the LDS layout are those of tile_f32.h

enum { GF_PLAIN = 0, GF_RESID = 1, GF_SWIGLU = 2, GF_GELU = 3, GF_QUICK_GELU = 4 };

struct GemmF32Args {
  const float *A, *W, *W2;
  float* C;
  const float *bias, *bias2, *gamma, *resid;
  int lda, ldw, ldc, ldr, M, N, K;
};

__device__ __forceinline__ float silu_exact(float x) { return x / (1.f + expf(-x)); }

template <int EPI>
__global__ __launch_bounds__(256) void gemm_nt_f32_kernel(const GemmF32Args g) {
  __shared__ float As[2][TF_BK][TF_LD];
  __shared__ float Bs[2][TF_BK][TF_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, j = lane & 31, half = lane >> 5;
  const int m0 = blockIdx.y * GF_BM;
  const int n0 = blockIdx.x * (EPI == GF_SWIGLU ? GF_BN / 2 : GF_BN);

  // the TF_IT 16-byte loads of this thread per operand and slab: tile row lr[it], k offset 4 * kq
  const int kq = tid & (TF_KQ - 1);
  const float* ap[TF_IT];
  const float* bp[TF_IT];
  int lr[TF_IT];
#pragma unroll
  for (int it = 0; it < TF_IT; ++it) {
    const int r = tid / TF_KQ + (256 / TF_KQ) * it;
    lr[it] = r;
    const int m = m0 + r;
    ap[it] = m < g.M ? g.A + (size_t)m * g.lda + 4 * kq : nullptr;
    if (EPI == GF_SWIGLU) {  // tile row r: wave column r / 64, tile column (r / 32) & 1 (0: w1, 1: w2), hidden column n0 + 32 (r / 64) + r % 32
      const int n = n0 + 32 * (r >> 6) + (r & 31);
      bp[it] = n < g.N ? (((r >> 5) & 1) ? g.W2 : g.W) + (size_t)n * g.ldw + 4 * kq : nullptr;
    } else {
      const int n = n0 + r;
      bp[it] = n < g.N ? g.W + (size_t)n * g.ldw + 4 * kq : nullptr;
    }
  }
  f32x16 acc[2][2];
  tile_f32_product(ap, bp, lr, kq, g.K, As, Bs, wm, wn, j, half, acc);

  // epilogue: lane = output column, register = output row
  if (EPI == GF_SWIGLU) {
    const int n = n0 + 32 * wn + j;
    if (n >= g.N) return;
    const float b1 = g.bias ? g.bias[n] : 0.f, b2 = g.bias2 ? g.bias2[n] : 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + u * 32 + acc_row(r, half);
        if (m < g.M) g.C[(size_t)m * g.ldc + n] = silu_exact(acc[u][0][r] + b1) * (acc[u][1][r] + b2);
      }
    return;
  }
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int n = n0 + wn * 64 + v * 32 + j;
    if (n >= g.N) continue;
    const float bias = g.bias ? g.bias[n] : 0.f;
    const float gam = (EPI == GF_RESID && g.gamma) ? g.gamma[n] : 1.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + u * 32 + acc_row(r, half);
        if (m >= g.M) continue;
        float y = acc[u][v][r] + bias;
        if (EPI == GF_RESID) {
          if (g.gamma) y = y * gam;
          y = g.resid[(size_t)m * g.ldr + n] + y;
        } else if (EPI == GF_GELU) {
          y = gelu_erf(y);
        } else if (EPI == GF_QUICK_GELU) {
          y = y / (1.f + expf(-1.702f * y));
        }
        g.C[(size_t)m * g.ldc + n] = y;
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------- attention
// One wave = 32 query rows of one (image, head), over the keys in blocks of 32.  Both products are computed TRANSPOSED so that a
// query sits on a lane and never moves:
//   S^T[key][query] = K Q^T : A operand = the lane's key row, B operand = the lane's query row; the head dimension is summed in the
//                             fixed order (t, 32 + t), t = 0..31 (lane half h holds columns [32 h, 32 h + 32) of its row: 8 loads of 16 bytes);
//   the accumulator holds, per lane (query j, half h), the 16 keys acc_row(r, h): row maximum and sum are 16 registers and ONE
//   exchange with the other half;
//   O^T[dv][query] = V^T P^T : step r sums the key acc_row(r, h) of each half -- the B operand is the probability register r as it
//                             stands, the A operand the V row of that key (lanes = 32 consecutive columns, one 128-byte line).
// Keys past N (and, with the causal mask, past the query) enter the softmax as -inf, never as padding; their loads go to clamped
// rows.  Key 0 is visible to every query, so the running maximum is finite from the first block on.
template <bool CAUSAL>
__global__ __launch_bounds__(64) void attn_fwd_f32_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                          const float* __restrict__ v, float* __restrict__ o, int N, long sb, long sn,
                                                          long sbo, long sno, float scale) {
  const int lane = threadIdx.x, j = lane & 31, half = lane >> 5;
  const int q0 = blockIdx.x * 32, h = blockIdx.y;
  const long b = blockIdx.z;
  const float* qb = q + b * sb + h * 64;
  const float* kb = k + b * sb + h * 64;
  const float* vb = v + b * sb + h * 64;
  float qr[32];
  {
    const float* p = qb + (long)min(q0 + j, N - 1) * sn + 32 * half;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const f32x4 t = *(const f32x4*)(p + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) qr[4 * c + e] = t[e];
    }
  }
  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) o0[r] = o1[r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int kend = CAUSAL ? min(N, q0 + 32) : N;
  for (int k0 = 0; k0 < kend; k0 += 32) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    {
      const float* p = kb + (long)min(k0 + j, N - 1) * sn + 32 * half;
      f32x4 kr[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) kr[c] = *(const f32x4*)(p + 4 * c);
#pragma unroll
      for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) s = mfma32(kr[c][e], qr[4 * c + e], s);
    }
    // the V rows of this block's keys: issued before the softmax arithmetic
    float va[16], vc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* p = vb + (long)min(k0 + acc_row(r, half), N - 1) * sn + j;
      va[r] = p[0];
      vc[r] = p[32];
    }
    float mloc = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, half);
      const bool ok = key < N && (!CAUSAL || key <= q0 + j);
      s[r] = ok ? s[r] * scale : -INFINITY;
      mloc = fmaxf(mloc, s[r]);
    }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    const float mn = fmaxf(m, mloc);
    const float alpha = expf(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = expf(s[r] - mn);
      ps += s[r];
    }
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      o0[r] *= alpha;
      o1[r] *= alpha;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      o0 = mfma32(va[r], s[r], o0);
      o1 = mfma32(vc[r], s[r], o1);
    }
  }
  if (q0 + j < N) {
    const float inv = 1.f / l;
    float* op = o + b * sbo + (long)(q0 + j) * sno + h * 64 + 4 * half;
#pragma unroll
    for (int c = 0; c < 4; ++c) {  // registers 4c .. 4c + 3 = head columns 8c + 4 half + (0..3)
      const f32x4 t0 = {o0[4 * c] * inv, o0[4 * c + 1] * inv, o0[4 * c + 2] * inv, o0[4 * c + 3] * inv};
      const f32x4 t1 = {o1[4 * c] * inv, o1[4 * c + 1] * inv, o1[4 * c + 2] * inv, o1[4 * c + 3] * inv};
      *(f32x4*)(op + 8 * c) = t0;
      *(f32x4*)(op + 32 + 8 * c) = t1;
    }
  }
}

}  // namespace vtp
using namespace vtp;

extern "C" int vtp_gemm_nt_f32(const float* A, int lda, const float* W, int ldw, const float* W2, float* C, int ldc, const float* bias,
                               const float* bias2, const float* gamma, const float* resid, int ldr, int M, int N, int K, int epi,
                               void* stream) {
  VTP_REQUIRE(A && W && C, "vtp_gemm_nt_f32: null pointer");
  VTP_REQUIRE(M >= 1 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0, "vtp_gemm_nt_f32: need M >= 1 and N, K positive multiples of 8 (M=%d N=%d K=%d)",
              M, N, K);
  VTP_REQUIRE(lda >= K && ldw >= K && ldc >= N && lda % 4 == 0 && ldw % 4 == 0,
              "vtp_gemm_nt_f32: leading dimensions must cover the rows, lda and ldw multiples of 4 (lda=%d ldw=%d ldc=%d)", lda, ldw, ldc);
  VTP_REQUIRE(aligned16(A) && aligned16(W) && aligned16(W2), "vtp_gemm_nt_f32: A, W and W2 must be 16-byte aligned");
  VTP_REQUIRE(epi >= GF_PLAIN && epi <= GF_QUICK_GELU, "vtp_gemm_nt_f32: unknown epilogue %d", epi);
  VTP_REQUIRE(epi != GF_RESID || (resid && ldr >= N), "vtp_gemm_nt_f32: the residual epilogue needs resid with ldr >= N");
  VTP_REQUIRE(epi != GF_SWIGLU || W2, "vtp_gemm_nt_f32: the SwiGLU epilogue needs W2");
  VTP_REQUIRE((epi == GF_SWIGLU) == (W2 != nullptr) && (epi == GF_SWIGLU || !bias2), "vtp_gemm_nt_f32: W2 / bias2 belong to the SwiGLU epilogue alone");
  VTP_REQUIRE((epi == GF_RESID) || (!gamma && !resid), "vtp_gemm_nt_f32: gamma / resid belong to the residual epilogue alone");
  const long by = ((long)M + GF_BM - 1) / GF_BM;
  VTP_REQUIRE(by <= 65535, "vtp_gemm_nt_f32: M too large (M=%d)", M);
  const GemmF32Args g = {A, W, W2, C, bias, bias2, gamma, resid, lda, ldw, ldc, ldr, M, N, K};
  const int bn = epi == GF_SWIGLU ? GF_BN / 2 : GF_BN;
  const dim3 grid((N + bn - 1) / bn, (unsigned)by);
  hipStream_t s = (hipStream_t)stream;
  switch (epi) {
    case GF_PLAIN: hipLaunchKernelGGL(gemm_nt_f32_kernel<GF_PLAIN>, grid, dim3(256), 0, s, g); break;
    case GF_RESID: hipLaunchKernelGGL(gemm_nt_f32_kernel<GF_RESID>, grid, dim3(256), 0, s, g); break;
    case GF_SWIGLU: hipLaunchKernelGGL(gemm_nt_f32_kernel<GF_SWIGLU>, grid, dim3(256), 0, s, g); break;
    case GF_GELU: hipLaunchKernelGGL(gemm_nt_f32_kernel<GF_GELU>, grid, dim3(256), 0, s, g); break;
    default: hipLaunchKernelGGL(gemm_nt_f32_kernel<GF_QUICK_GELU>, grid, dim3(256), 0, s, g); break;
  }
  return check_launch("gemm_nt_f32");
}

extern "C" int vtp_attn_fwd_f32(const float* q, const float* k, const float* v, float* o, int B, int N, int heads, long sb, long sn,
                                long sbo, long sno, float scale, int causal, void* stream) {
  VTP_REQUIRE(q && k && v && o, "vtp_attn_fwd_f32: null pointer");
  VTP_REQUIRE(B >= 1 && N >= 1 && heads >= 1 && B <= 65535 && heads <= 65535, "vtp_attn_fwd_f32: bad shape (B=%d N=%d heads=%d)", B, N, heads);
  VTP_REQUIRE(sn >= 64L * heads && sno >= 64L * heads && sn % 4 == 0 && sno % 4 == 0 && sb % 4 == 0 && sbo % 4 == 0,
              "vtp_attn_fwd_f32: row strides must cover heads * 64 columns, all strides multiples of 4");
  VTP_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o), "vtp_attn_fwd_f32: q, k, v, o must be 16-byte aligned");
  const dim3 grid((N + 31) / 32, heads, B);
  if (causal)
    hipLaunchKernelGGL(attn_fwd_f32_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, q, k, v, o, N, sb, sn, sbo, sno, scale);
  else
    hipLaunchKernelGGL(attn_fwd_f32_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, q, k, v, o, N, sb, sn, sbo, sno, scale);
  return check_launch("attn_fwd_f32");
}
