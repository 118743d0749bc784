// What the optimizer kernels of optim.hip (Adam / AdamW) and optim_family.hip (LAMB, AdamP, MADGRAD, Lookahead) share: the
// d2t_optim object with its table staging rotation, the fixed-order block sum, the per-thread sum of squares of the global
// gradient norm, and the pointer validation of every entry point.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/d2t.h"

namespace d2t {

constexpr int OPT_THREADS = 256;

// sum of the 256 threads' values in a fixed order (lanes by halving strides, then waves 0..3); valid in thread 0
__device__ inline double block_sum(double x) {
  __shared__ double part[OPT_THREADS / 64];
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < OPT_THREADS / 64; ++w) r += part[w];
  return r;
}

// this thread's serial fp32 sum of squares over its (at most D2T_OPTIM_CHUNK / 256) elements of one chunk's gradient
__device__ inline float chunk_sumsq(const float* __restrict__ g, int n) {
  float acc = 0.f;
  int i = threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int n4 = n >> 2;
    for (; i < n4; i += OPT_THREADS) {
      const float4 q = reinterpret_cast<const float4*>(g)[i];
      acc += q.x * q.x;
      acc += q.y * q.y;
      acc += q.z * q.z;
      acc += q.w * q.w;
    }
    i = (n4 << 2) + threadIdx.x;
  }
  for (; i < n; i += OPT_THREADS) acc += g[i] * g[i];
  return acc;
}

}  // namespace d2t

struct d2t_optim {
  int device = 0;
  std::string err;
  // the chunk table travels through a pinned block and its device mirror, four in rotation: the host never waits on the
  // previous step's copy
  struct Stage { void *h = nullptr, *d = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool pending = false; } stage[4];
  unsigned calls = 0;
  double* partial = nullptr;
  size_t partial_cap = 0;  // entries
  float* coef = nullptr;
  void* family = nullptr;  // optim_family.hip: per-chunk, per-row and per-tensor sums and the projection decisions
  size_t family_cap = 0;   // bytes
};

namespace d2t {

inline int ofail(d2t_optim* o, int code, const char* fmt, ...) {
  if (o) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    o->err = buf;
  }
  return code;
}
#define OHIP(o, expr)                                                                                \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return d2t::ofail(o, D2T_EHIP, "%s: %s", #expr, hipGetErrorString(e_));  \
  } while (0)

struct OptDevGuard {
  int prev = -1;
  explicit OptDevGuard(const d2t_optim* o) {
    int cur = -1;
    if (o && hipGetDevice(&cur) == hipSuccess && cur != o->device && hipSetDevice(o->device) == hipSuccess) prev = cur;
  }
  ~OptDevGuard() { if (prev >= 0) hipSetDevice(prev); }
};

// the kernels dereference every pointer of a record: each must be device memory of the optimizer's device
inline int optim_dev_ptr(d2t_optim* o, const void* p, int rec, const char* what) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return ofail(o, D2T_EINVAL, "tensor %d: %s is not device memory", rec, what);
  }
  if (a.type != hipMemoryTypeDevice) return ofail(o, D2T_EINVAL, "tensor %d: %s is not device memory", rec, what);
  if (a.device != o->device)
    return ofail(o, D2T_EINVAL, "tensor %d: %s is on HIP device %d but this optimizer lives on device %d", rec, what, a.device, o->device);
  return D2T_OK;
}

// the next staging pair of the rotation with room for `bytes`: fill (*out)->h, then optim_stage_send
inline int optim_stage_take(d2t_optim* o, size_t bytes, d2t_optim::Stage** out) {
  d2t_optim::Stage& g = o->stage[o->calls++ & 3];
  if (g.pending) {
    OHIP(o, hipEventSynchronize(g.ev));
    g.pending = false;
  }
  if (bytes > g.cap) {
    if (g.h) { OHIP(o, hipHostFree(g.h)); OHIP(o, hipFree(g.d)); }
    g.h = g.d = nullptr;
    g.cap = 0;
    OHIP(o, hipHostMalloc(&g.h, bytes * 2, hipHostMallocDefault));
    OHIP(o, hipMalloc(&g.d, bytes * 2));
    g.cap = bytes * 2;
    if (!g.ev) OHIP(o, hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
  }
  *out = &g;
  return D2T_OK;
}

inline int optim_stage_send(d2t_optim* o, d2t_optim::Stage& g, size_t bytes, hipStream_t s) {
  OHIP(o, hipMemcpyAsync(g.d, g.h, bytes, hipMemcpyHostToDevice, s));
  OHIP(o, hipEventRecord(g.ev, s));
  g.pending = true;
  return D2T_OK;
}

}  // namespace d2t
