// Wave-wide reductions shared by the training kernels (train_kernels.hip, train_attn.hip, train_recurrent.hip), the
// recurrent kernels (recurrent_common.h) and, through that header, the encoder's small kernels (ops.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace d2t {
static __device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
static __device__ __forceinline__ float wmax(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
}  // namespace d2t
