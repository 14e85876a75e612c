// Diagnostics of the production kernels: the gate of the process-global hooks (vtp_gemm_debug, vtp_attn_debug, vtp_cu_thief), the
// timeline stamp and the delayed start.  Stamps are 100 MHz wall-clock ticks (s_memrealtime) in a caller-owned device buffer.
#pragma once
#include "common.h"
#include <stdlib.h>

namespace vtp {

// hooks of PRODUCTION kernels are accepted only in a process that asked for diagnostics: VTP_DIAG=1 in its environment
// (the tools/ scripts set it), read at every call
inline bool diag_allowed(const char* who) {
  const char* diag = getenv("VTP_DIAG");
  if (diag && diag[0] == '1') return true;
  set_error("%s: diagnostics hooks need VTP_DIAG=1 in the environment", who);
  return false;
}

// one stamp (null buffer: off): a plain store from the lane the caller selects, buffer size unchecked.  A kernel tests the buffer itself
// in front of its lane test (wave-uniform first: one scalar branch while off); the other order changes the production kernels' code
__device__ __forceinline__ void diag_stamp(unsigned long long* buf, size_t slot) {
  if (__builtin_expect(buf != nullptr, 0)) buf[slot] = wall_clock64();
}

// start-delay experiments: wait `ticks` x 10 ns; the caller selects the workgroups that wait
__device__ __forceinline__ void diag_delay(int ticks) {
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < (unsigned long long)ticks) __builtin_amdgcn_s_sleep(16);
}

}  // namespace vtp
