// fp32 <-> split records and weight planes: the element-wise kernels around the record convolutions (conv_common.h: the
// record formats) and their launchers.
#include "conv_common.h"

namespace d2t {

// grid of the element-wise kernels below: 256 threads per block, grid-stride loops, at most `cap` blocks
__global__ void split_bf16_kernel(const float* __restrict__ w, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo,
                                  size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float x = w[i];
    const __bf16 h = (__bf16)x;  // v_cvt_pk_bf16_f32: round to nearest even
    const __bf16 l = (__bf16)(x - (float)h);
    hi[i] = *reinterpret_cast<const uint16_t*>(&h);
    lo[i] = *reinterpret_cast<const uint16_t*>(&l);
  }
}
__global__ void split_f16_kernel(const float* __restrict__ w, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float x = w[i];
    const uint16_t h = f32_to_f16_bits(x);
    hi[i] = h;
    lo[i] = f32_to_f16_bits(x - f16_bits_to_f32(h));
  }
}
__global__ void split_act_kernel(const float* __restrict__ x, uint16_t* __restrict__ planes, size_t rows, int C, int fmt) {
  const size_t n = rows * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint16_t hi, lo;
    split_rec(x[i], hi, lo, fmt);
    const size_t o = plane_idx(i / C, (int)(i % C), C);
    planes[o] = hi;
    planes[o + 32] = lo;
  }
}
__global__ void merge_act_kernel(const uint16_t* __restrict__ planes, float* __restrict__ x, size_t rows, int C, int fmt) {
  const size_t n = rows * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t o = plane_idx(i / C, (int)(i % C), C);
    x[i] = join_rec(planes[o], planes[o + 32], fmt);
  }
}
// the same, eight channels per thread: two 16-byte loads, one 16-byte store into each half of the record (C % 32 == 0)
__global__ void split_act8_kernel(const float* __restrict__ x, uint16_t* __restrict__ planes, size_t n8, int fmt) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = reinterpret_cast<const float4*>(x)[2 * i], b = reinterpret_cast<const float4*>(x)[2 * i + 1];
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint16_t hi[8], lo[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) split_rec(v[k], hi[k], lo[k], fmt);
    // element e = 8 i of the row-major [rows][C] tensor lies in record e / 32 at position e % 32 (C % 32 == 0)
    const size_t rec = i >> 2, pos = (i & 3) * 8;
    uint16_t* dst = planes + rec * 64 + pos;
    *reinterpret_cast<uint4*>(dst) = make_uint4(hi[0] | (uint32_t)hi[1] << 16, hi[2] | (uint32_t)hi[3] << 16,
                                                hi[4] | (uint32_t)hi[5] << 16, hi[6] | (uint32_t)hi[7] << 16);
    *reinterpret_cast<uint4*>(dst + 32) = make_uint4(lo[0] | (uint32_t)lo[1] << 16, lo[2] | (uint32_t)lo[3] << 16,
                                                     lo[4] | (uint32_t)lo[5] << 16, lo[6] | (uint32_t)lo[7] << 16);
  }
}
hipError_t launch_split_act(const float* x, uint16_t* planes, size_t rows, int C, hipStream_t s, int fmt) {
  const size_t n = rows * C;
  if (C % 32 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    const size_t n8 = n / 8;
    hipLaunchKernelGGL(split_act8_kernel, grid_1d(n8, 8192), dim3(256), 0, s, x,
                       planes, n8, fmt);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(split_act_kernel, grid_1d(n, 4096), dim3(256), 0,
                     s, x, planes, rows, C, fmt);
  return hipGetLastError();
}
hipError_t launch_merge_act(const uint16_t* planes, float* x, size_t rows, int C, hipStream_t s, int fmt) {
  const size_t n = rows * C;
  hipLaunchKernelGGL(merge_act_kernel, grid_1d(n, 4096), dim3(256), 0,
                     s, planes, x, rows, C, fmt);
  return hipGetLastError();
}

hipError_t launch_split_f16(const float* w, uint16_t* hi, uint16_t* lo, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(split_f16_kernel, grid_1d(n, 4096), dim3(256), 0,
                     s, w, hi, lo, n);
  return hipGetLastError();
}
hipError_t launch_split_bf16(const float* w, uint16_t* hi, uint16_t* lo, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(split_bf16_kernel, grid_1d(n, 4096), dim3(256), 0,
                     s, w, hi, lo, n);
  return hipGetLastError();
}

}  // namespace d2t
