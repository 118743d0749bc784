// The optimizer step of the training loop (engine/training.py:139-150: clip_grad_norm_ + optimizer.step()) as multi-tensor
// kernels: the global gradient norm, then Adam / AdamW with the clip coefficient applied on the fly and the new parameter
// written twice -- to the module's tensor and to the engine's raw copy of it -- so that the next forward uploads nothing.
// include/d2t.h has the contract.  Three launches and one table copy per step, no host synchronisation.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "optim_common.h"

namespace d2t {

// one block's work: `n` (<= D2T_OPTIM_CHUNK) consecutive elements of one tensor, and that tensor's scalars as the kernel
// uses them (derived on the host in double, rounded once)
struct OptimChunk {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* mirror;  // engine copy of p, or nullptr
  int n;
  float decay;    // AdamW: 1 - lr * wd.  Adam: unused
  float wd;       // Adam: g += wd * p.  AdamW: unused
  float w1;       // 1 - beta1
  float b2, w2;   // beta2, 1 - beta2
  float step;     // lr / bc1
  float sbc2;     // sqrt(bc2)
  float eps;
  int pad_;
};
static_assert(sizeof(OptimChunk) == 80, "table entries are 16-byte multiples");

__device__ inline bool chunk_vec(const OptimChunk& c) {
  return ((reinterpret_cast<uintptr_t>(c.p) | reinterpret_cast<uintptr_t>(c.g) | reinterpret_cast<uintptr_t>(c.m) |
           reinterpret_cast<uintptr_t>(c.v) | reinterpret_cast<uintptr_t>(c.mirror)) & 15) == 0;
}

// partial[blockIdx.x] = sum of squares of the chunk's gradient: each thread a serial fp32 sum of its (at most
// D2T_OPTIM_CHUNK / 256) elements, everything above that in double
__global__ __launch_bounds__(OPT_THREADS) void optim_sumsq_kernel(const OptimChunk* __restrict__ table, double* __restrict__ partial) {
  const OptimChunk c = table[blockIdx.x];
  const float acc = chunk_sumsq(c.g, c.n);
  const double s = block_sum((double)acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one block: norm = sqrt(sum of the partials), in double and in a fixed order; coef = min(1, max_norm / (norm + 1e-6)) in fp32
// as clip_grad_norm_ forms it (a NaN norm gives a NaN coefficient there too)
__global__ __launch_bounds__(OPT_THREADS) void optim_norm_kernel(const double* __restrict__ partial, int count, float max_norm,
                                                                 float* __restrict__ norm_out, float* __restrict__ coef_out) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += OPT_THREADS) acc += partial[i];
  const double s = block_sum(acc);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    const float c = max_norm / (norm + 1e-6f);
    *norm_out = norm;
    *coef_out = c < 1.f ? c : (c != c ? c : 1.f);
  }
}

template <bool DECOUPLED>
__device__ inline void adam_one(const OptimChunk& c, float coef, float g, float& p, float& m, float& v) {
  g *= coef;
  if (DECOUPLED) p *= c.decay;
  else if (c.wd != 0.f) g += c.wd * p;
  m += (g - m) * c.w1;
  v = c.b2 * v + c.w2 * g * g;
  p -= c.step * (m / (sqrtf(v) / c.sbc2 + c.eps));
}

template <bool DECOUPLED>
__global__ __launch_bounds__(OPT_THREADS) void optim_adam_kernel(const OptimChunk* __restrict__ table, const float* __restrict__ coef_dev) {
  const OptimChunk c = table[blockIdx.x];
  const float coef = coef_dev ? *coef_dev : 1.f;
  int i = threadIdx.x;
  if (chunk_vec(c)) {
    const int n4 = c.n >> 2;
    for (; i < n4; i += OPT_THREADS) {
      const float4 g = reinterpret_cast<const float4*>(c.g)[i];
      float4 p = reinterpret_cast<float4*>(c.p)[i], m = reinterpret_cast<float4*>(c.m)[i], v = reinterpret_cast<float4*>(c.v)[i];
      adam_one<DECOUPLED>(c, coef, g.x, p.x, m.x, v.x);
      adam_one<DECOUPLED>(c, coef, g.y, p.y, m.y, v.y);
      adam_one<DECOUPLED>(c, coef, g.z, p.z, m.z, v.z);
      adam_one<DECOUPLED>(c, coef, g.w, p.w, m.w, v.w);
      reinterpret_cast<float4*>(c.p)[i] = p;
      reinterpret_cast<float4*>(c.m)[i] = m;
      reinterpret_cast<float4*>(c.v)[i] = v;
      if (c.mirror) reinterpret_cast<float4*>(c.mirror)[i] = p;
    }
    i = (n4 << 2) + threadIdx.x;
  }
  for (; i < c.n; i += OPT_THREADS) {
    float p = c.p[i], m = c.m[i], v = c.v[i];
    adam_one<DECOUPLED>(c, coef, c.g[i], p, m, v);
    c.p[i] = p;
    c.m[i] = m;
    c.v[i] = v;
    if (c.mirror) c.mirror[i] = p;
  }
}

}  // namespace d2t

using d2t::OptimChunk;

using d2t::ofail;
using d2t::optim_dev_ptr;
using d2t::OptDevGuard;

extern "C" {

int32_t d2t_optim_chunk(void) { return D2T_OPTIM_CHUNK; }

int d2t_optim_create(d2t_optim** out) {
  if (!out) return D2T_EINVAL;
  *out = nullptr;
  d2t_optim* o = new d2t_optim();
  if (hipGetDevice(&o->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&o->coef), 16) != hipSuccess) {
    (void)hipGetLastError();
    delete o;
    return D2T_EHIP;
  }
  *out = o;
  return D2T_OK;
}

void d2t_optim_destroy(d2t_optim* o) {
  if (!o) return;
  OptDevGuard dg_(o);
  hipDeviceSynchronize();
  for (auto& s : o->stage) {
    if (s.h) hipHostFree(s.h);
    if (s.d) hipFree(s.d);
    if (s.ev) hipEventDestroy(s.ev);
  }
  if (o->partial) hipFree(o->partial);
  if (o->coef) hipFree(o->coef);
  if (o->family) hipFree(o->family);
  delete o;
}

const char* d2t_optim_last_error(d2t_optim* o) { return o ? o->err.c_str() : "null optimizer"; }

int d2t_optim_step(d2t_optim* o, const d2t_optim_tensor* recs, int32_t n, int32_t decoupled, float max_grad_norm,
                   float* norm_dev, d2t_stream stream) {
  if (!o) return D2T_EINVAL;
  OptDevGuard dg_(o);
  if (n < 0 || (n && !recs)) return ofail(o, D2T_EINVAL, "bad argument: %d tensors", n);
  const bool clip = max_grad_norm > 0.f;
  if (clip && !norm_dev) return ofail(o, D2T_EINVAL, "clipping needs a device float for the norm");
  if (clip)
    if (int rc = optim_dev_ptr(o, norm_dev, -1, "norm")) return rc;
  size_t chunks = 0;
  for (int i = 0; i < n; ++i) {
    const d2t_optim_tensor& r = recs[i];
    if (r.numel < 0 || (r.numel > 0 && (!r.param || !r.grad || !r.exp_avg || !r.exp_avg_sq)))
      return ofail(o, D2T_EINVAL, "tensor %d: null pointer or negative size", i);
    if (!(r.bc1 > 0.0) || !(r.sqrt_bc2 > 0.0) || !(r.eps >= 0.0) || !std::isfinite(r.lr) || !std::isfinite(r.weight_decay))
      return ofail(o, D2T_EINVAL, "tensor %d: bad scalars (bc1 %g, sqrt_bc2 %g, eps %g, lr %g, weight_decay %g)", i, r.bc1,
                   r.sqrt_bc2, r.eps, r.lr, r.weight_decay);
    if (r.numel == 0) continue;
    int rc;
    if ((rc = optim_dev_ptr(o, r.param, i, "param")) || (rc = optim_dev_ptr(o, r.grad, i, "grad")) ||
        (rc = optim_dev_ptr(o, r.exp_avg, i, "exp_avg")) || (rc = optim_dev_ptr(o, r.exp_avg_sq, i, "exp_avg_sq")) ||
        (r.mirror && (rc = optim_dev_ptr(o, r.mirror, i, "mirror"))))
      return rc;
    chunks += (size_t)((r.numel + D2T_OPTIM_CHUNK - 1) / D2T_OPTIM_CHUNK);
    if (chunks > (1u << 24)) return ofail(o, D2T_EINVAL, "more than %u chunks in one step", 1u << 24);
  }
  hipStream_t s = (hipStream_t)stream;
  if (chunks == 0) {
    if (clip) OHIP(o, hipMemsetAsync(norm_dev, 0, 4, s));
    return D2T_OK;
  }
  const size_t bytes = chunks * sizeof(OptimChunk);
  d2t_optim::Stage* gp = nullptr;
  if (int rc = d2t::optim_stage_take(o, bytes, &gp)) return rc;
  d2t_optim::Stage& g = *gp;
  if (clip && chunks > o->partial_cap) {
    if (o->partial) { OHIP(o, hipDeviceSynchronize()); OHIP(o, hipFree(o->partial)); }
    o->partial = nullptr;
    o->partial_cap = 0;
    OHIP(o, hipMalloc(reinterpret_cast<void**>(&o->partial), chunks * 2 * sizeof(double)));
    o->partial_cap = chunks * 2;
  }
  OptimChunk* t = static_cast<OptimChunk*>(g.h);
  for (int i = 0; i < n; ++i) {
    const d2t_optim_tensor& r = recs[i];
    OptimChunk c{};
    c.decay = (float)(1.0 - r.lr * r.weight_decay);
    c.wd = (float)r.weight_decay;
    c.w1 = (float)(1.0 - r.beta1);
    c.b2 = (float)r.beta2;
    c.w2 = (float)(1.0 - r.beta2);
    c.step = (float)(r.lr / r.bc1);
    c.sbc2 = (float)r.sqrt_bc2;
    c.eps = (float)r.eps;
    for (int64_t off = 0; off < r.numel; off += D2T_OPTIM_CHUNK) {
      c.p = r.param + off;
      c.g = r.grad + off;
      c.m = r.exp_avg + off;
      c.v = r.exp_avg_sq + off;
      c.mirror = r.mirror ? r.mirror + off : nullptr;
      c.n = (int)std::min<int64_t>(D2T_OPTIM_CHUNK, r.numel - off);
      *t++ = c;
    }
  }
  if (int rc = d2t::optim_stage_send(o, g, bytes, s)) return rc;
  const OptimChunk* table = static_cast<const OptimChunk*>(g.d);
  if (clip) {
    hipLaunchKernelGGL(d2t::optim_sumsq_kernel, dim3((unsigned)chunks), dim3(d2t::OPT_THREADS), 0, s, table, o->partial);
    hipLaunchKernelGGL(d2t::optim_norm_kernel, dim3(1), dim3(d2t::OPT_THREADS), 0, s, o->partial, (int)chunks, max_grad_norm,
                       norm_dev, o->coef);
  }
  const float* coef = clip ? o->coef : nullptr;
  if (decoupled) hipLaunchKernelGGL(d2t::optim_adam_kernel<true>, dim3((unsigned)chunks), dim3(d2t::OPT_THREADS), 0, s, table, coef);
  else hipLaunchKernelGGL(d2t::optim_adam_kernel<false>, dim3((unsigned)chunks), dim3(d2t::OPT_THREADS), 0, s, table, coef);
  OHIP(o, hipGetLastError());
  return D2T_OK;
}

}  // extern "C"
