// What the decode-step translation units share (decode.hip, decode_gemm.hip, decode_row.hip, decode_beam.hip): the wave
// priority, the debug timeline, the activation and the 256-thread switch.
#pragma once
#include "kernels.h"

namespace d2t {

using f32x4 = __attribute__((ext_vector_type(4))) float;
#ifndef D2T_DECODE_PRIO
#define D2T_DECODE_PRIO 3
#endif

// The decode step is a dependent chain of small latency-bound kernels that runs BESIDE the next batches' convolutions
// (pipelined serving).  Instruction issue on a SIMD is arbitrated by priority, then age (MI355X_MICROARCH.md "Two waves per
// SIMD" item 2): a decode wave is always younger than the persistent convolution waves it shares the SIMD with and would
// get only the issue slots they leave.  Its few instructions cost the matrix-bound convolution next to nothing, so the
// decode kernels simply outrank it.
__device__ __forceinline__ void decode_wave_priority() { __builtin_amdgcn_s_setprio(D2T_DECODE_PRIO); }

// debug timeline (D2T_DECODE_TRACE): every block folds its own start / end time into the launch's record
struct TraceScope {
  unsigned long long* t;
  __device__ __forceinline__ explicit TraceScope(unsigned long long* tr) : t(tr) {
    if (t && threadIdx.x == 0) atomicMin(t, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  }
  __device__ __forceinline__ ~TraceScope() {
    if (t) {
      __syncthreads();
      if (threadIdx.x == 0) atomicMax(t + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
  }
};

__device__ __forceinline__ float act_fn(float v, int act) {
  if (act == ACT_RELU) return fmaxf(v, 0.f);
  if (act == ACT_GELU) return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
  return v;
}

// small = 1: the 256-thread forms of the decode kernels (one wave per SIMD, <= 128 VGPRs), which fit on a CU beside the
// pipelined convolution kernel's three 128-register waves per SIMD; identical arithmetic per row, so identical results.
// inline: the environment is read once per library, not once per translation unit (hidden: not part of the library's surface)
#pragma GCC visibility push(hidden)
inline int decode_small() {
  static const int v = D2T_PROBE_ENV("D2T_DECODE_SMALL");
  return v;
}
#pragma GCC visibility pop

}  // namespace d2t
