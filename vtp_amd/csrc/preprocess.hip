// PIL's 8-bit resampling (Resample.c: Image.resize with BOX / BILINEAR / BICUBIC) and the crop, flip, ToTensor + Normalize behind
// it, bit for bit, over a ragged batch of decoded byte images -- the first stage of the linear-probing, zero-shot and
// reconstruction tools and of the tokenizer (center_crop_arr), which ran only as PIL on the host.
//
// The host (vtp_amd/preprocess.py) forms every coefficient in float64 as PIL does and rounds it to 22-bit fixed point; the device
// does the integer part:  acc = 2^21 + sum_j K[j] src[min + j]  (int32, |acc| < 2^31: sum |K| <= 1.3 * 2^22),
// dst = clamp(acc >> 22, 0, 255).  PIL runs the horizontal pass, rounds to 8 bits, then the vertical pass; so do we, as one launch
// per pass over the whole batch.  A job row (16 x int64, on the device) is one pass of one image:
//    0 src     byte offset of the pass's first source byte (in the source buffer, or in scratch: flag 1)
//    1 dst     byte offset of the output in scratch; in the last launch: the image's index in the batch
//    2,3 oh ow the output of this pass, in pixels
//    4,5 sy sx source bytes per output row / column (horizontal pass: pitch, 0; vertical pass: 0, 3)
//    6 ts      bytes between two taps (horizontal: 3; vertical: the source pitch)
//    7 bnd     index in tab of the (min, n) pair of this pass's first output column (horizontal) / row (vertical)
//    8 coef    index in tab of that entry's coefficients;  9 ksize: coefficients per entry
//    10 sub    subtracted from min: the first source row the buffer holds (the pass before wrote only the rows the window needs)
//    11 flags  1 source in scratch | 2 the table runs along y (vertical pass) | 4 flip (last launch only)
//    12 block  the job's first block in its launch; a block resamples 256 consecutive output pixels, one per thread
// A block finds its job by bisection over slot 12.  The last launch is the vertical pass of each image's last resize over the final
// crop window only, with the flip, and writes (float(u8) / 255 - mean) / std -- the expression of vtp_u8_to_images -- as f32 NCHW,
// and the bytes as uint8 NHWC if asked.  An axis PIL skips gets the one-tap table K = 2^22: (2^21 + p 2^22) >> 22 == p.
//
// The job table lives on the device, so nothing here can refuse a bad row: the host checks every offset of every job against its
// buffer before anything is uploaded (check_jobs) and raises.  Every output element is written exactly once, by plain stores; no
// atomics, no floating-point sums: a run repeats bit for bit.
#include "common.h"
#include "vtp_hip.h"

namespace vtp {

constexpr int PP_T = 256;     // output pixels per block
constexpr int PP_SLOTS = 16;  // int64 slots per job row
constexpr int PP_BITS = 22;   // PIL's PRECISION_BITS

struct PpJob {
  long src, dst;
  int oh, ow;
  long sy, sx, ts;
  long bnd, coef;
  int ksize, sub, flags;
  long block;
};

__device__ __forceinline__ PpJob pp_job(const long* __restrict__ jobs, int njobs, long blk) {
  int lo = 0, hi = njobs - 1;  // the last job whose first block is <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[(long)mid * PP_SLOTS + 12] <= blk) lo = mid;
    else hi = mid - 1;
  }
  const long* j = jobs + (long)lo * PP_SLOTS;
  PpJob p;
  p.src = j[0], p.dst = j[1], p.oh = (int)j[2], p.ow = (int)j[3], p.sy = j[4], p.sx = j[5], p.ts = j[6], p.bnd = j[7], p.coef = j[8];
  p.ksize = (int)j[9], p.sub = (int)j[10], p.flags = (int)j[11], p.block = j[12];
  return p;
}

// the three channels of output pixel (oy, ox) of pass p; xs: the source column (ox, or its mirror)
__device__ __forceinline__ void pp_pixel(const PpJob& p, const uint8_t* base, const int* __restrict__ tab, int oy, int xs, int (&v)[3]) {
  const int e = (p.flags & 2) ? oy : xs;  // a flipped column is flipped only in a vertical pass: its table runs along y
  const int mn = tab[p.bnd + 2 * (long)e] - p.sub, n = tab[p.bnd + 2 * (long)e + 1];
  const int* __restrict__ k = tab + p.coef + (long)e * p.ksize;
  const uint8_t* s = base + p.src + oy * p.sy + xs * p.sx + mn * p.ts;
  int a0 = 1 << (PP_BITS - 1), a1 = a0, a2 = a0;
  for (int j = 0; j < n; ++j) {
    const int w = k[j];
    a0 += w * (int)s[0], a1 += w * (int)s[1], a2 += w * (int)s[2];
    s += p.ts;
  }
  v[0] = min(max(a0 >> PP_BITS, 0), 255), v[1] = min(max(a1 >> PP_BITS, 0), 255), v[2] = min(max(a2 >> PP_BITS, 0), 255);
}

// one pass of every image that has one in this launch: bytes to bytes (scratch)
__global__ __launch_bounds__(PP_T) void preprocess_pass_kernel(const uint8_t* __restrict__ src, uint8_t* scratch,
                                                               const long* __restrict__ jobs, int njobs, const int* __restrict__ tab) {
  const PpJob p = pp_job(jobs, njobs, blockIdx.x);
  const long px = ((long)blockIdx.x - p.block) * PP_T + threadIdx.x;
  if (px >= (long)p.oh * p.ow) return;
  const int oy = (int)(px / p.ow), ox = (int)(px - (long)oy * p.ow);
  int v[3];
  pp_pixel(p, (p.flags & 1) ? scratch : src, tab, oy, ox, v);
  uint8_t* d = scratch + p.dst + px * 3;
  d[0] = (uint8_t)v[0], d[1] = (uint8_t)v[1], d[2] = (uint8_t)v[2];
}

// the last vertical pass of every image over its crop window, the flip, ToTensor + Normalize
__global__ __launch_bounds__(PP_T) void preprocess_final_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ scratch,
                                                                const long* __restrict__ jobs, int njobs, const int* __restrict__ tab,
                                                                f32x4 mean, f32x4 stdv, float* __restrict__ out,
                                                                uint8_t* __restrict__ out_u8) {
  const PpJob p = pp_job(jobs, njobs, blockIdx.x);
  const long px = ((long)blockIdx.x - p.block) * PP_T + threadIdx.x;
  const long plane = (long)p.oh * p.ow;
  if (px >= plane) return;
  const int oy = (int)(px / p.ow), ox = (int)(px - (long)oy * p.ow);
  int v[3];
  pp_pixel(p, (p.flags & 1) ? scratch : src, tab, oy, (p.flags & 4) ? p.ow - 1 - ox : ox, v);
  float* o = out + p.dst * 3 * plane + px;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * plane] = ((float)v[c] / 255.0f - mean[c]) / stdv[c];
  if (out_u8) {
    uint8_t* d = out_u8 + (p.dst * plane + px) * 3;
    d[0] = (uint8_t)v[0], d[1] = (uint8_t)v[1], d[2] = (uint8_t)v[2];
  }
}

}  // namespace vtp

using namespace vtp;

extern "C" int vtp_preprocess(const void* src_u8, long src_len, void* scratch, long scratch_len, const long* jobs, const int* tab,
                              const int* launches, int n_launches, long B, int Ho, int Wo, const float* mean3, const float* std3,
                              float* out, void* out_u8, void* stream) {
  VTP_REQUIRE(src_u8 && jobs && tab && launches && mean3 && std3 && out,
              "vtp_preprocess: null pointer (src_u8, jobs, tab, launches, mean3, std3, out)");
  VTP_REQUIRE(src_len >= 3 && scratch_len >= 0 && (scratch || scratch_len == 0), "vtp_preprocess: src_len >= 3, scratch_len >= 0");
  VTP_REQUIRE(n_launches >= 1 && B >= 1 && B <= 0x7fffffffL && Ho >= 1 && Wo >= 1, "vtp_preprocess: n_launches, B, Ho, Wo >= 1");
  VTP_REQUIRE(scratch || n_launches == 1, "vtp_preprocess: passes in front of the last one need scratch");
  VTP_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "vtp_preprocess: std3 must not be zero");
  VTP_REQUIRE(((uintptr_t)jobs & 7) == 0 && ((uintptr_t)tab & 3) == 0 && ((uintptr_t)out & 3) == 0,
              "vtp_preprocess: jobs must be 8-byte aligned, tab and out 4-byte aligned");
  long at = 0;
  for (int l = 0; l < n_launches; ++l) {
    const int first = launches[3 * l], count = launches[3 * l + 1], blocks = launches[3 * l + 2];
    VTP_REQUIRE(first == at && count >= 1 && blocks >= count, "vtp_preprocess: launch %d: jobs [%d, %d), %d blocks", l, first,
                first + count, blocks);
    at += count;
  }
  VTP_REQUIRE(launches[3 * (n_launches - 1) + 1] == B, "vtp_preprocess: the last launch needs one job per image (%ld), got %d", B,
              launches[3 * (n_launches - 1) + 1]);
  const f32x4 m = {mean3[0], mean3[1], mean3[2], 0.f}, s = {std3[0], std3[1], std3[2], 1.f};
  for (int l = 0; l < n_launches; ++l) {
    const long* j = jobs + (long)launches[3 * l] * PP_SLOTS;
    const int count = launches[3 * l + 1];
    const dim3 grid((unsigned)launches[3 * l + 2]);
    if (l < n_launches - 1) {
      hipLaunchKernelGGL(preprocess_pass_kernel, grid, dim3(PP_T), 0, (hipStream_t)stream, (const uint8_t*)src_u8, (uint8_t*)scratch, j,
                         count, tab);
      const int rc = check_launch("preprocess_pass");
      if (rc != VTP_OK) return rc;
    } else {
      hipLaunchKernelGGL(preprocess_final_kernel, grid, dim3(PP_T), 0, (hipStream_t)stream, (const uint8_t*)src_u8,
                         (const uint8_t*)scratch, j, count, tab, m, s, out, (uint8_t*)out_u8);
    }
  }
  return check_launch("preprocess_final");
}
