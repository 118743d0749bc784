// Kernels of the training step (train.hip): everything module.train() + loss.backward() needs beyond the
// forward GEMM/convolution kernel, the weight gradients (train_wgrad.hip), softmax attention (train_attn.hip) and the
// recurrent paths (train_recurrent.hip), all fp32.
//
//   colreduce_kernel    per-channel sums over rows: BatchNorm batch statistics, BatchNorm / LayerNorm parameter
//                       gradients, bias gradients
//   bn_*                BatchNorm2d in training mode (batch statistics, running-statistics update, backward)
//   ln_*                LayerNorm forward with saved statistics, backward
//   ce_*                fused cross-entropy, plain and smoothed / class-weighted
//   maxpool_bwd, relu/gelu backward, embedding, dropout masks, GlobalContext, small data-movement helpers
//
// Reference semantics: torch autograd of feature_extractor/resnet.py:205-245, seq_modeling/vit/vision_transformer.py:26-122,
// prediction_head/tfm.py:103-118 as driven by engine/training.py:76-164.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_common.h"
#include "kernels.h"
#include "train_common.h"

namespace d2t {

namespace {
constexpr int EW_THREADS = 256;
inline int ew_grid(size_t n4) { return (int)std::min<size_t>((n4 + EW_THREADS - 1) / EW_THREADS, 65535u * 16u); }
}  // namespace

// ---------------------------------------------------------------------------
// Column reductions over the rows of row-major [R][C] matrices -> part[chunk][2][C]
// ---------------------------------------------------------------------------
// rows per block: about 2048 blocks per launch (eight per CU -- these kernels are HBM streams and one block per CU, which
// 2048-row chunks gave on the large maps, kept them near 2 TB/s), at least 128 rows each
static int colreduce_rows(long long R, int C) {
  const long long col_blocks = (C + 63) / 64, chunks = std::max<long long>(1, 2048 / col_blocks);
  const long long rows = ((R + chunks - 1) / chunks + 15) / 16 * 16;
  return (int)std::max<long long>(128, rows);
}
__global__ __launch_bounds__(256) void colreduce_kernel(const ColRedP p, int rows_per_block) {
  __shared__ float red[16][2][64];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int c = blockIdx.x * 64 + tx * 4;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  const long long r1 = r0 + rows_per_block < p.R ? r0 + rows_per_block : p.R;
  float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < p.C) {
    float mu[4] = {0, 0, 0, 0}, rs[4] = {1, 1, 1, 1};
    if (p.mode == CR_BN_BWD) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { mu[k] = p.mean[c + k]; rs[k] = p.rstd[c + k]; }
    } else if (p.mode == CR_SUM_SQ) {
      // the sums are taken about the channel's value in row 0 (read once per thread): sum (a - k) and sum (a - k)^2 keep
      // their bits where the mean lies many standard deviations from zero, E[a^2] - mean^2 from raw fp32 sums does not
      const float4 k4 = *reinterpret_cast<const float4*>(p.a + c);
      mu[0] = k4.x; mu[1] = k4.y; mu[2] = k4.z; mu[3] = k4.w;
    }
#pragma unroll 8
    for (long long r = r0 + ty; r < r1; r += 16) {
      const size_t off = (size_t)r * p.C + c;
      const float4 a4 = *reinterpret_cast<const float4*>(p.a + off);
      const float a[4] = {a4.x, a4.y, a4.z, a4.w};
      if (p.mode == CR_SUM) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s0[k] += a[k];
      } else if (p.mode == CR_SUM_SQ) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float d = a[k] - mu[k]; s0[k] += d; s1[k] = fmaf(d, d, s1[k]); }
      } else if (p.mode == CR_BN_BWD) {  // a = dy, y = post-activation output (nullable), z = pre-BN conv output
        const float4 z4 = *reinterpret_cast<const float4*>(p.z + off);
        const float z[4] = {z4.x, z4.y, z4.z, z4.w};
        float g[4] = {a[0], a[1], a[2], a[3]};
        if (p.y) {
          const float4 y4 = *reinterpret_cast<const float4*>(p.y + off);
          const float y[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) g[k] = y[k] > 0.f ? g[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { s0[k] += g[k]; s1[k] = fmaf(g[k], (z[k] - mu[k]) * rs[k], s1[k]); }
      } else {  // CR_LN_BWD: a = dy, z = LayerNorm input, mean / rstd per ROW
        const float4 z4 = *reinterpret_cast<const float4*>(p.z + off);
        const float z[4] = {z4.x, z4.y, z4.z, z4.w};
        const float m = p.mean[r], q = p.rstd[r];
#pragma unroll
        for (int k = 0; k < 4; ++k) { s0[k] += a[k]; s1[k] = fmaf(a[k], (z[k] - m) * q, s1[k]); }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { red[ty][0][tx * 4 + k] = s0[k]; red[ty][1][tx * 4 + k] = s1[k]; }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int which = threadIdx.x >> 6, col = threadIdx.x & 63;
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) v += red[t][which][col];
    const int cc = blockIdx.x * 64 + col;
    if (cc < p.C) p.part[((size_t)blockIdx.y * 2 + which) * p.C + cc] = v;
  }
}
int colreduce_chunks(long long R, int C) {
  const int rows = colreduce_rows(R, C);
  return (int)((R + rows - 1) / rows);
}
hipError_t launch_colreduce(const ColRedP& p, hipStream_t s) {
  if (p.C % 4 || p.R <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(colreduce_kernel, dim3((p.C + 63) / 64, colreduce_chunks(p.R, p.C)), dim3(256), 0, s, p,
                     colreduce_rows(p.R, p.C));
  return hipGetLastError();
}
// out0[c] = (acc ? out0[c] : 0) + sum_chunks part[.][0][c];  out1 likewise (nullable)
// sums over the chunks of part[chunk][2][C] for 32 channels per 256-thread block: eight threads per channel take every
// eighth chunk (double accumulators), thread 0 of the eight adds their partial sums in a fixed order
__device__ __forceinline__ void chunk_sums(const float* __restrict__ part, int chunks, int C, int c, int lane8, double (*red)[8][32],
                                           double& a, double& b) {
  a = 0.0; b = 0.0;
  if (c < C) {
#pragma unroll 8
    for (int k = lane8; k < chunks; k += 8) { a += part[((size_t)k * 2) * C + c]; b += part[((size_t)k * 2 + 1) * C + c]; }
  }
  red[0][lane8][threadIdx.x & 31] = a;
  red[1][lane8][threadIdx.x & 31] = b;
  __syncthreads();
  if (lane8 == 0) {
    a = 0.0; b = 0.0;
#pragma unroll
    for (int t = 0; t < 8; ++t) { a += red[0][t][threadIdx.x & 31]; b += red[1][t][threadIdx.x & 31]; }
  }
}
__global__ __launch_bounds__(256) void colreduce_final_kernel(const float* __restrict__ part, int chunks, int C, float* out0,
                                                              float* out1, int accumulate) {
  __shared__ double red[2][8][32];
  const int c = blockIdx.x * 32 + (threadIdx.x & 31), lane8 = threadIdx.x >> 5;
  double a, b;
  chunk_sums(part, chunks, C, c, lane8, red, a, b);
  if (lane8 != 0 || c >= C) return;
  if (out0) out0[c] = (accumulate ? out0[c] : 0.f) + (float)a;
  if (out1) out1[c] = (accumulate ? out1[c] : 0.f) + (float)b;
}
hipError_t launch_colreduce_final(const float* part, int chunks, int C, float* out0, float* out1, int accumulate,
                                  hipStream_t s) {
  hipLaunchKernelGGL(colreduce_final_kernel, dim3((C + 31) / 32), dim3(256), 0, s, part, chunks, C, out0, out1, accumulate);
  return hipGetLastError();
}
// BatchNorm batch statistics from the CR_SUM_SQ partials of z (sums of z - k and of (z - k)^2, k = z[0][c]: the shift);
// running statistics updated in place (momentum 0.1, unbiased variance: nn.BatchNorm2d defaults used by resnet.py).
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ part, int chunks, int C, long long R, float eps,
                                                          float momentum, const float* __restrict__ shift, float* mean,
                                                          float* rstd, float* run_mean, float* run_var) {
  __shared__ double red[2][8][32];
  const int c = blockIdx.x * 32 + (threadIdx.x & 31), lane8 = threadIdx.x >> 5;
  double a, b;
  chunk_sums(part, chunks, C, c, lane8, red, a, b);
  if (lane8 != 0 || c >= C) return;
  const double md = a / (double)R;  // E[z - k]
  double var = b / (double)R - md * md;
  if (var < 0.0) var = 0.0;
  const double m = (double)shift[c] + md;
  mean[c] = (float)m;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (run_mean) {
    const double unb = R > 1 ? var * (double)R / (double)(R - 1) : var;
    run_mean[c] = (float)((1.0 - momentum) * run_mean[c] + momentum * m);
    run_var[c] = (float)((1.0 - momentum) * run_var[c] + momentum * unb);
  }
}
hipError_t launch_bn_finalize(const float* part, int chunks, int C, long long R, float eps, float momentum, const float* z,
                              float* mean, float* rstd, float* run_mean, float* run_var, hipStream_t s) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 31) / 32), dim3(256), 0, s, part, chunks, C, R, eps, momentum, z, mean,
                     rstd, run_mean, run_var);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// BatchNorm apply (train forward) and backward apply, float4 over [R][C]
// ---------------------------------------------------------------------------
// the four values of flat float4 index i4 of a row-major [rows][C] tensor (C % 32 == 0) as split-bf16 record entries
// (conv_common.h plane_idx): what the LDS-DMA convolution kernels read
__device__ __forceinline__ void store_split4(uint16_t* planes, size_t i4, const float (&v)[4]) {
  uint16_t hi[4], lo[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) split_f32(v[k], hi[k], lo[k]);
  const size_t e = i4 * 4;
  uint16_t* dst = planes + (e >> 5) * 64 + (e & 31);
  *reinterpret_cast<uint2*>(dst) = make_uint2(hi[0] | (uint32_t)hi[1] << 16, hi[2] | (uint32_t)hi[3] << 16);
  *reinterpret_cast<uint2*>(dst + 32) = make_uint2(lo[0] | (uint32_t)lo[1] << 16, lo[2] | (uint32_t)lo[3] << 16);
}
__global__ void bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ rstd,
                                const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ res,
                                float* __restrict__ y, size_t n4, int C, int relu, uint16_t* __restrict__ planes) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)((i * 4) % C);
    const float4 v = reinterpret_cast<const float4*>(z)[i];
    float o[4] = {v.x, v.y, v.z, v.w};
    float r4[4] = {0, 0, 0, 0};
    if (res) { const float4 t = reinterpret_cast<const float4*>(res)[i]; r4[0] = t.x; r4[1] = t.y; r4[2] = t.z; r4[3] = t.w; }
    // (per-channel parameters as 16-byte loads: c and C are multiples of 4)
    const float4 m4 = *reinterpret_cast<const float4*>(mean + c), q4 = *reinterpret_cast<const float4*>(rstd + c);
    const float4 g4 = *reinterpret_cast<const float4*>(g + c), b4 = *reinterpret_cast<const float4*>(b + c);
    const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, qq[4] = {q4.x, q4.y, q4.z, q4.w};
    const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float t = (o[k] - mm[k]) * qq[k] * gg[k] + bb[k] + r4[k];
      o[k] = relu ? fmaxf(t, 0.f) : t;
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(o[0], o[1], o[2], o[3]);
    if (planes) store_split4(planes, i, o);
  }
}
hipError_t launch_bn_apply(const float* z, const float* mean, const float* rstd, const float* g, const float* b,
                           const float* res, float* y, long long R, int C, int relu, hipStream_t s, uint16_t* planes) {
  const size_t n4 = (size_t)R * C / 4;
  if (planes && C % 32 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_apply_kernel, dim3(ew_grid(n4)), dim3(EW_THREADS), 0, s, z, mean, rstd, g, b, res, y, n4, C, relu, planes);
  return hipGetLastError();
}
// dz = gamma*rstd * (g - s0/R - xhat * s1/R),  g = dy * (y > 0) (y nullable = no ReLU);  gout (nullable) receives g
// (the gradient of the residual branch that was added before the ReLU).
__global__ void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ z,
                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                    const float* __restrict__ gamma, const float* __restrict__ s0,
                                    const float* __restrict__ s1, float invR, float* __restrict__ dz,
                                    float* __restrict__ gout, size_t n4, int C, uint16_t* __restrict__ planes) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)((i * 4) % C);
    const float4 d4 = reinterpret_cast<const float4*>(dy)[i];
    const float4 z4 = reinterpret_cast<const float4*>(z)[i];
    float g[4] = {d4.x, d4.y, d4.z, d4.w};
    const float zz[4] = {z4.x, z4.y, z4.z, z4.w};
    if (y) {
      const float4 y4 = reinterpret_cast<const float4*>(y)[i];
      const float yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = yy[k] > 0.f ? g[k] : 0.f;
    }
    float o[4];
    const float4 m4 = *reinterpret_cast<const float4*>(mean + c), q4 = *reinterpret_cast<const float4*>(rstd + c);
    const float4 g4 = *reinterpret_cast<const float4*>(gamma + c);
    const float4 a4 = *reinterpret_cast<const float4*>(s0 + c), b4 = *reinterpret_cast<const float4*>(s1 + c);
    const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, qq[4] = {q4.x, q4.y, q4.z, q4.w}, gm[4] = {g4.x, g4.y, g4.z, g4.w};
    const float sa[4] = {a4.x, a4.y, a4.z, a4.w}, sb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xh = (zz[k] - mm[k]) * qq[k];
      o[k] = gm[k] * qq[k] * (g[k] - sa[k] * invR - xh * sb[k] * invR);
    }
    reinterpret_cast<float4*>(dz)[i] = make_float4(o[0], o[1], o[2], o[3]);
    if (planes) store_split4(planes, i, o);
    if (gout) reinterpret_cast<float4*>(gout)[i] = make_float4(g[0], g[1], g[2], g[3]);
  }
}
hipError_t launch_bn_bwd_apply(const float* dy, const float* y, const float* z, const float* mean, const float* rstd,
                               const float* gamma, const float* s0, const float* s1, float* dz, float* gout, long long R,
                               int C, hipStream_t s, uint16_t* planes) {
  const size_t n4 = (size_t)R * C / 4;
  if (planes && C % 32 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_grid(n4)), dim3(EW_THREADS), 0, s, dy, y, z, mean, rstd, gamma, s0, s1,
                     1.f / (float)R, dz, gout, n4, C, planes);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Elementwise: out = f(a, b)
// ---------------------------------------------------------------------------
__global__ void ew_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, size_t n4,
                          int op) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 x4 = reinterpret_cast<const float4*>(a)[i];
    float x[4] = {x4.x, x4.y, x4.z, x4.w}, y[4] = {0, 0, 0, 0}, o[4];
    if (b) { const float4 y4 = reinterpret_cast<const float4*>(b)[i]; y[0] = y4.x; y[1] = y4.y; y[2] = y4.z; y[3] = y4.w; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      switch (op) {
        case EW_ADD: o[k] = x[k] + y[k]; break;
        case EW_RELU_BWD: o[k] = y[k] > 0.f ? x[k] : 0.f; break;  // a = dy, b = forward output
        case EW_RELU: o[k] = fmaxf(x[k], 0.f); break;
        case EW_GELU: o[k] = 0.5f * x[k] * (1.f + erff(x[k] * 0.70710678118654752440f)); break;
        case EW_GELU_BWD: {  // a = dy, b = pre-activation u: d/du [u * Phi(u)] = Phi(u) + u * phi(u)
          const float u = y[k];
          const float cdf = 0.5f * (1.f + erff(u * 0.70710678118654752440f));
          const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
          o[k] = x[k] * (cdf + u * pdf);
          break;
        }
        default: o[k] = x[k];
      }
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}
hipError_t launch_ew(const float* a, const float* b, float* out, size_t n, int op, hipStream_t s) {
  if (n % 4) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(ew_kernel, dim3(ew_grid(n / 4)), dim3(EW_THREADS), 0, s, a, b, out, n / 4, op);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// MaxPool2d(k=2) backward, gather form (deterministic): every input pixel collects dy of the windows whose
// FIRST maximum (scan order kh, kw; padding = -inf) it is -- the rule of torch's max_pool2d_with_indices.
// ---------------------------------------------------------------------------
__global__ void maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int B,
                                   int H, int W, int C, int OH, int OW, int SH, int SW, int PH, int PW, int KW) {
  const int C4 = C >> 2;  // four channels per thread (C % 4 == 0): one set of index arithmetic, 16-byte accesses
  const size_t total = (size_t)B * H * W * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    const int w = (int)((i / C4) % W), h = (int)((i / ((size_t)C4 * W)) % H), b = (int)(i / ((size_t)C4 * W * H));
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    // windows (oh, ow) that contain (h, w): oh*SH - PH <= h <= oh*SH - PH + 1
    const int oh_lo = h + PH - 1 > 0 ? (h + PH - 1 + SH - 1) / SH : 0, oh_hi = min((h + PH) / SH, OH - 1);
    const int ow_lo = w + PW - (KW - 1) > 0 ? (w + PW - (KW - 1) + SW - 1) / SW : 0, ow_hi = min((w + PW) / SW, OW - 1);
    for (int oh = oh_lo; oh <= oh_hi; ++oh)
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        bool mine[4] = {false, false, false, false};  // is (h, w) the first maximum so far
        bool any = false;
        for (int kh = 0; kh < 2; ++kh)
          for (int kw = 0; kw < KW; ++kw) {
            const int ih = oh * SH - PH + kh, iw = ow * SW - PW + kw;
            if ((unsigned)ih >= (unsigned)H || (unsigned)iw >= (unsigned)W) continue;
            const float4 v4 = *reinterpret_cast<const float4*>(x + (((size_t)b * H + ih) * W + iw) * C + c);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            const bool here = ih == h && iw == w;
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (v[k] > best[k] || !any) { best[k] = v[k]; mine[k] = here; }
            any = true;
          }
        const float4 d4 = *reinterpret_cast<const float4*>(dy + (((size_t)b * OH + oh) * OW + ow) * C + c);
        const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (mine[k]) acc[k] += d[k];
      }
    *reinterpret_cast<float4*>(dx + i * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
}
hipError_t launch_maxpool_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, int SH, int SW, int PH,
                              int PW, hipStream_t s, int KW) {  // window 2 x KW (KW = 1: VGG's (2,1) pools)
  const int OH = (H + 2 * PH - 2) / SH + 1, OW = (W + 2 * PW - KW) / SW + 1;
  if (C % 4) return hipErrorInvalidValue;
  const size_t total = (size_t)B * H * W * (C / 4);
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1u << 20)), dim3(256), 0, s, x,
                     dy, dx, B, H, W, C, OH, OW, SH, SW, PH, PW, KW);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Fused cross-entropy (nn.CrossEntropyLoss(ignore_index, reduction='none') of engine/training.py:50-53,83,90): one wave per
// row of the [rows][V] logits.  Forward: lse = max + log(sum exp(x - max)); loss = lse - x[target] (0 where target ==
// ignore_index); backward: dx[v] = (exp(x[v] - lse) - [v == target]) * dloss, 0 for ignored rows.  Replaces torch's
// log_softmax + nll_loss pair (four passes over the logits) with one pass each way.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                     float* __restrict__ loss, float* __restrict__ lse, int rows, int V,
                                                     long long ignore) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const float* xr = x + (size_t)row * V;
  float m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, xr[v]);
  m = wmax(m);
  float sum = 0.f;
  for (int v = lane; v < V; v += 64) sum += expf(xr[v] - m);
  sum = wsum(sum);
  if (lane == 0) {
    const float l = m + logf(sum);
    const long long t = tgt[row];
    lse[row] = l;
    loss[row] = (t == ignore || t < 0 || t >= V) ? 0.f : l - xr[t];
  }
}
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                     const float* __restrict__ lse, const float* __restrict__ dloss,
                                                     float* __restrict__ dx, int rows, int V, long long ignore) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const float* xr = x + (size_t)row * V;
  float* dr = dx + (size_t)row * V;
  const long long t = tgt[row];
  const bool live = !(t == ignore || t < 0 || t >= V);
  const float g = live ? dloss[row] : 0.f, l = lse[row];
  for (int v = lane; v < V; v += 64) dr[v] = live ? (expf(xr[v] - l) - (v == t ? 1.f : 0.f)) * g : 0.f;
}
hipError_t launch_ce_fwd(const float* x, const int64_t* tgt, float* loss, float* lse, int rows, int V, long long ignore,
                         hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(ce_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, tgt, loss, lse, rows, V, ignore);
  return hipGetLastError();
}
hipError_t launch_ce_bwd(const float* x, const int64_t* tgt, const float* lse, const float* dloss, float* dx, int rows, int V,
                         long long ignore, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, tgt, lse, dloss, dx, rows, V, ignore);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Smoothed / class-weighted cross-entropy: the other criteria modules/loss/builder.py:18-24 can build.  Per live row with
// target t the criterion spreads a mass m[v] over the classes,
//     m[v] = on * w[t] * [v == t]  +  off * w[v] * [v in S],        M = sum_v m[v],
//     loss = sum_v m[v] * (lse - x[v]),        dx[v] = dloss * (M * exp(x[v] - lse) - m[v]),
//   mode 0 (nn.CrossEntropyLoss(weight, label_smoothing = e)):  on = 1 - e, off = e / V, S = every class, w = weight or 1;
//   mode 1 (LabelSmoothingLoss, labelsmoothing.py:15-30):  on = 1 - s, off = s / (classes - 2), S = every class but t and
//          the padding column, w = 1 -- M is then not 1, and the gradient carries it.
// One wave per row as above, but ONE pass over the logits each way: the forward keeps a running maximum with the rescaled
// exp-sum (online softmax) beside U = sum off-mass and UX = sum off-mass * x, so loss = on*w[t]*(lse - x[t]) + U*lse - UX
// and M = on*w[t] + U; it saves lse and M per row, the backward redoes no reduction.  A row is read as float4 from its first
// 16-byte boundary on (up to three scalar elements in front and behind), whatever V is.  Ignored rows (target ==
// ignore_index or outside [0, V)) are not read: loss 0, gradient row 0.
// (tools/probe/ce_smooth_host.cpp runs the code between the two markers lane by lane on the host, under AddressSanitizer.)
// ---------------------------------------------------------------------------
// [ce_smooth: begin]
namespace {
struct CeSmooth {
  const float* w;  // class weights or nullptr (mode 0)
  float on, off;
  int ref;          // mode 1
  long long t, pad;
  // off-target mass of class v (the target's own `on` share is added by the caller)
  __device__ __forceinline__ float u(int v, float wv) const { return (ref && (v == t || v == pad)) ? 0.f : off * wv; }
  __device__ __forceinline__ float wt(int v) const { return w ? w[v] : 1.f; }
};
// elements in front of the first 16-byte boundary of a row
__device__ __forceinline__ int ce_head(const float* p, int V) {
  return min(V, (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u));
}
__device__ __forceinline__ float4 ce_w4(const CeSmooth& c, int v, bool wvec) {
  if (!c.w) return make_float4(1.f, 1.f, 1.f, 1.f);
  if (wvec) return *reinterpret_cast<const float4*>(c.w + v);
  return make_float4(c.w[v], c.w[v + 1], c.w[v + 2], c.w[v + 3]);
}
}  // namespace

__global__ __launch_bounds__(256) void ce_smooth_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                            const float* __restrict__ w, float* __restrict__ loss,
                                                            float* __restrict__ lse, float* __restrict__ mass, int rows, int V,
                                                            long long ignore, float on, float off, int ref, long long pad) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const long long t = tgt[row];
  if (t == ignore || t < 0 || t >= V) {
    if (lane == 0) loss[row] = 0.f, lse[row] = 0.f, mass[row] = 0.f;
    return;
  }
  const CeSmooth c{w, on, off, ref, t, pad};
  const float* xr = x + (size_t)row * V;
  float m = -INFINITY, sum = 0.f, U = 0.f, UX = 0.f;  // per lane: running maximum, sum exp(x - m), off-mass, off-mass * x
  auto take = [&](float xv, int v) {
    if (xv > m) sum *= expf(m - xv), m = xv;
    if (m > -INFINITY) sum += expf(xv - m);
    const float u = c.u(v, c.wt(v));
    if (u != 0.f) U += u, UX = fmaf(u, xv, UX);  // (a class without mass may sit at -inf)
  };
  const int head = ce_head(xr, V), nvec = (V - head) >> 2, tail = head + (nvec << 2);
  const bool wvec = w && (((uintptr_t)(w + head)) & 15) == 0;
  if (lane < head) take(xr[lane], lane);
#pragma unroll 2
  for (int i = lane; i < nvec; i += 64) {
    const int v = head + (i << 2);
    const float4 q = *reinterpret_cast<const float4*>(xr + v);
    const float4 wq = ce_w4(c, v, wvec);
    const float mx = fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w));
    if (mx > m) sum *= expf(m - mx), m = mx;
    if (m > -INFINITY) sum += (expf(q.x - m) + expf(q.y - m)) + (expf(q.z - m) + expf(q.w - m));
    const float u0 = c.u(v, wq.x), u1 = c.u(v + 1, wq.y), u2 = c.u(v + 2, wq.z), u3 = c.u(v + 3, wq.w);
    if (u0 != 0.f) U += u0, UX = fmaf(u0, q.x, UX);
    if (u1 != 0.f) U += u1, UX = fmaf(u1, q.y, UX);
    if (u2 != 0.f) U += u2, UX = fmaf(u2, q.z, UX);
    if (u3 != 0.f) U += u3, UX = fmaf(u3, q.w, UX);
  }
  if (tail + lane < V) take(xr[tail + lane], tail + lane);
  const float mrow = wmax(m);
  sum = wsum(m > -INFINITY ? sum * expf(m - mrow) : 0.f);  // lanes that held no element (V < 64) add nothing
  U = wsum(U);
  UX = wsum(UX);
  if (lane == 0) {
    const float l = mrow + logf(sum), hit = on * c.wt((int)t);
    lse[row] = l;
    mass[row] = hit + U;
    loss[row] = hit * (l - xr[t]) + (U != 0.f ? U * l - UX : 0.f);
  }
}
__global__ __launch_bounds__(256) void ce_smooth_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                            const float* __restrict__ w, const float* __restrict__ lse,
                                                            const float* __restrict__ mass, const float* __restrict__ dloss,
                                                            float* __restrict__ dx, int rows, int V, long long ignore, float on,
                                                            float off, int ref, long long pad) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const float* xr = x + (size_t)row * V;
  float* dr = dx + (size_t)row * V;
  const long long t = tgt[row];
  const bool live = !(t == ignore || t < 0 || t >= V);
  const CeSmooth c{w, on, off, ref, t, pad};
  const float g = live ? dloss[row] : 0.f, l = live ? lse[row] : 0.f, M = live ? mass[row] : 0.f;
  const float hit = live ? on * c.wt((int)t) : 0.f;
  auto grad = [&](float xv, int v, float wv) { return (M * expf(xv - l) - (c.u(v, wv) + (v == t ? hit : 0.f))) * g; };
  // float4 only where the row of x and the row of dx reach a 16-byte boundary together
  const bool same = ((((uintptr_t)xr) ^ ((uintptr_t)dr)) & 15) == 0;
  const int head = same ? ce_head(xr, V) : V, nvec = (V - head) >> 2, tail = head + (nvec << 2);
  if (!live) {
    for (int v = lane; v < head; v += 64) dr[v] = 0.f;
    for (int i = lane; i < nvec; i += 64) *reinterpret_cast<float4*>(dr + head + (i << 2)) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tail + lane < V) dr[tail + lane] = 0.f;
    return;
  }
  const bool wvec = w && (((uintptr_t)(w + head)) & 15) == 0;
  for (int v = lane; v < head; v += 64) dr[v] = grad(xr[v], v, c.wt(v));
#pragma unroll 2
  for (int i = lane; i < nvec; i += 64) {
    const int v = head + (i << 2);
    const float4 q = *reinterpret_cast<const float4*>(xr + v);
    const float4 wq = ce_w4(c, v, wvec);
    *reinterpret_cast<float4*>(dr + v) =
        make_float4(grad(q.x, v, wq.x), grad(q.y, v + 1, wq.y), grad(q.z, v + 2, wq.z), grad(q.w, v + 3, wq.w));
  }
  if (tail + lane < V) dr[tail + lane] = grad(xr[tail + lane], tail + lane, c.wt(tail + lane));
}
// [ce_smooth: end]
hipError_t launch_ce_smooth_fwd(const float* x, const int64_t* tgt, const float* w, float* loss, float* lse, float* mass,
                                int rows, int V, long long ignore, float on, float off, int ref, long long pad, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(ce_smooth_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, tgt, w, loss, lse, mass, rows, V, ignore,
                     on, off, ref, pad);
  return hipGetLastError();
}
hipError_t launch_ce_smooth_bwd(const float* x, const int64_t* tgt, const float* w, const float* lse, const float* mass,
                                const float* dloss, float* dx, int rows, int V, long long ignore, float on, float off, int ref,
                                long long pad, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(ce_smooth_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, tgt, w, lse, mass, dloss, dx, rows, V,
                     ignore, on, off, ref, pad);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The discrete decisions of a training forward, for tests that replay them in the oracle (d2t_train_read_decision):
// ReLU keep masks (y > 0) and, per max-pool output element, which window element (kh*2 + kw) the backward routes the
// gradient to -- the same first-maximum scan as maxpool_bwd_kernel.
// ---------------------------------------------------------------------------
__global__ void relu_mask_kernel(const float* __restrict__ y, uint8_t* __restrict__ m, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) m[i] = y[i] > 0.f;
}
hipError_t launch_relu_mask(const float* y, uint8_t* m, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1u << 20)), dim3(256), 0, s, y, m, n);
  return hipGetLastError();
}
__global__ void pool_argmax_kernel(const float* __restrict__ x, uint8_t* __restrict__ k, int B, int H, int W, int C, int OH,
                                   int OW, int SH, int SW, int PH, int PW, int KW) {
  const size_t total = (size_t)B * OH * OW * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int ow = (int)((i / C) % OW), oh = (int)((i / ((size_t)C * OW)) % OH), b = (int)(i / ((size_t)C * OW * OH));
    float best = -INFINITY;
    int bk = -1;
    for (int kh = 0; kh < 2; ++kh)
      for (int kw = 0; kw < KW; ++kw) {
        const int ih = oh * SH - PH + kh, iw = ow * SW - PW + kw;
        if ((unsigned)ih >= (unsigned)H || (unsigned)iw >= (unsigned)W) continue;
        const float v = x[(((size_t)b * H + ih) * W + iw) * C + c];
        if (v > best || bk < 0) { best = v; bk = kh * KW + kw; }
      }
    k[i] = (uint8_t)bk;
  }
}
hipError_t launch_pool_argmax(const float* x, uint8_t* k, int B, int H, int W, int C, int SH, int SW, int PH, int PW,
                              hipStream_t s, int KW) {
  const int OH = (H + 2 * PH - 2) / SH + 1, OW = (W + 2 * PW - KW) / SW + 1;
  const size_t total = (size_t)B * OH * OW * C;
  hipLaunchKernelGGL(pool_argmax_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1u << 20)), dim3(256), 0, s, x, k,
                     B, H, W, C, OH, OW, SH, SW, PH, PW, KW);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// LayerNorm with saved statistics / backward.  One wave per row, D = 128, 256 or 512.
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void ln_train_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                       const float* __restrict__ b, float* __restrict__ y,
                                                       float* __restrict__ mean, float* __restrict__ rstd, int rows,
                                                       float eps) {
  constexpr int PER = D / 64;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float v[PER], s = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) { v[k] = x[(size_t)row * D + lane + 64 * k]; s += v[k]; }
  const float m = wsum(s) / D;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) q = fmaf(v[k] - m, v[k] - m, q);
  const float r = rsqrtf(wsum(q) / D + eps);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int c = lane + 64 * k;
    y[(size_t)row * D + c] = (v[k] - m) * r * g[c] + b[c];
  }
  if (lane == 0) { mean[row] = m; rstd[row] = r; }
}
hipError_t launch_ln_train(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, int rows,
                           int D, float eps, hipStream_t s) {
  if (D == 128) hipLaunchKernelGGL(ln_train_kernel<128>, dim3((rows + 3) / 4), dim3(256), 0, s, x, g, b, y, mean, rstd, rows, eps);
  else if (D == 256) hipLaunchKernelGGL(ln_train_kernel<256>, dim3((rows + 3) / 4), dim3(256), 0, s, x, g, b, y, mean, rstd, rows, eps);
  else if (D == 512) hipLaunchKernelGGL(ln_train_kernel<512>, dim3((rows + 3) / 4), dim3(256), 0, s, x, g, b, y, mean, rstd, rows, eps);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
// dx = rstd * (dyg - mean_c(dyg) - xhat * mean_c(dyg * xhat)) (+ add),  dyg = dy * gamma
template <int D>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ g, const float* __restrict__ add,
                                                     float* __restrict__ dx, int rows) {
  constexpr int PER = D / 64;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float m = mean[row], r = rstd[row];
  float dg[PER], xh[PER], a = 0.f, bsum = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int c = lane + 64 * k;
    dg[k] = dy[(size_t)row * D + c] * g[c];
    xh[k] = (x[(size_t)row * D + c] - m) * r;
    a += dg[k];
    bsum = fmaf(dg[k], xh[k], bsum);
  }
  a = wsum(a) / D;
  bsum = wsum(bsum) / D;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int c = lane + 64 * k;
    float o = r * (dg[k] - a - xh[k] * bsum);
    if (add) o += add[(size_t)row * D + c];
    dx[(size_t)row * D + c] = o;
  }
}
hipError_t launch_ln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g,
                         const float* add, float* dx, int rows, int D, hipStream_t s) {
  if (D == 128) hipLaunchKernelGGL(ln_bwd_kernel<128>, dim3((rows + 3) / 4), dim3(256), 0, s, dy, x, mean, rstd, g, add, dx, rows);
  else if (D == 256) hipLaunchKernelGGL(ln_bwd_kernel<256>, dim3((rows + 3) / 4), dim3(256), 0, s, dy, x, mean, rstd, g, add, dx, rows);
  else if (D == 512) hipLaunchKernelGGL(ln_bwd_kernel<512>, dim3((rows + 3) / 4), dim3(256), 0, s, dy, x, mean, rstd, g, add, dx, rows);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Embedding: x[r][:] = E[tok[r]][:] * scale + pe[r % L][:];  backward (deterministic, block per vocabulary row):
// dE[v][:] = scale * sum_{r: tok[r] == v} dx[r][:], zero for the padding row (nn.Embedding padding_idx).
// ---------------------------------------------------------------------------
__global__ void embed_train_kernel(const float* __restrict__ E, const float* __restrict__ pe, const int64_t* __restrict__ tok,
                                   float* __restrict__ x, int rows, int L, int D, float scale) {
  const int r = blockIdx.x;
  const int64_t t = tok[r];
  for (int c = threadIdx.x; c < D; c += blockDim.x) x[(size_t)r * D + c] = E[(size_t)t * D + c] * scale + pe[(size_t)(r % L) * D + c];
}
hipError_t launch_embed_train(const float* E, const float* pe, const int64_t* tok, float* x, int rows, int L, int D,
                              float scale, hipStream_t s) {
  hipLaunchKernelGGL(embed_train_kernel, dim3(rows), dim3(256), 0, s, E, pe, tok, x, rows, L, D, scale);
  return hipGetLastError();
}
// One block per vocabulary row v (deterministic: rows are added in ascending order).  The block first lists the rows whose
// token is v -- 256 rows per pass, positions by ballot prefix -- and then adds only those (a token occurs in a handful of
// the B*L rows; scanning every row for every column was 0.37 ms).  D <= 1024.
__global__ __launch_bounds__(256) void embed_bwd_kernel(const float* __restrict__ dx, const int64_t* __restrict__ tok,
                                                        float* __restrict__ dE, int rows, int D, float scale, int pad_id) {
  constexpr int CAP = 1024;
  __shared__ int list[CAP + 256];
  __shared__ int wcnt[4];
  const int v = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int n = 0;  // rows listed and not yet added (block-uniform)
  auto flush = [&]() {
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const float* src = dx + (size_t)list[k] * D;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = tid + j * 256;
        if (c < D) acc[j] += src[c];
      }
    }
    __syncthreads();
    n = 0;
  };
  if (v != pad_id) {
    for (int base = 0; base < rows; base += 256) {
      const int r = base + tid;
      const bool hit = r < rows && tok[r] == v;
      const unsigned long long m = __ballot(hit);
      if (lane == 0) wcnt[wave] = __popcll(m);
      __syncthreads();
      int off = n;
      for (int w = 0; w < wave; ++w) off += wcnt[w];
      if (hit) list[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
      const int add = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
      __syncthreads();
      n += add;
      if (n >= CAP) flush();
    }
    flush();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = tid + j * 256;
    if (c < D) dE[(size_t)v * D + c] = acc[j] * scale;
  }
}
hipError_t launch_embed_bwd(const float* dx, const int64_t* tok, float* dE, int rows, int V, int D, float scale, int pad_id,
                            hipStream_t s) {
  if (D > 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(V), dim3(256), 0, s, dx, tok, dE, rows, D, scale, pad_id);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Dropout: keep masks from Philox4x32-10 (counter-based, so forward and backward see the same mask without storing
// random state; masks are materialised as bytes because several kernels consume them)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32(unsigned long long counter, unsigned long long stream_id, unsigned k0, unsigned k1,
                                           unsigned (&out)[4]) {
  unsigned c0 = (unsigned)counter, c1 = (unsigned)(counter >> 32), c2 = (unsigned)stream_id, c3 = (unsigned)(stream_id >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__global__ void dropout_mask_kernel(uint8_t* __restrict__ mask, size_t n, unsigned thresh16, unsigned long long seed,
                                    unsigned long long stream_id) {
  const size_t groups = (n + 7) / 8;  // eight 16-bit draws per Philox call
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    unsigned r[4];
    philox4x32(g, stream_id, (unsigned)seed, (unsigned)(seed >> 32), r);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const size_t i = g * 8 + k;
      if (i < n) mask[i] = ((r[k >> 1] >> (16 * (k & 1))) & 0xFFFFu) >= thresh16 ? 1 : 0;
    }
  }
}
hipError_t launch_dropout_mask(uint8_t* mask, size_t n, float p, unsigned long long seed, unsigned long long stream_id,
                               hipStream_t s) {
  if (!n) return hipSuccess;
  const unsigned thresh = (unsigned)(p * 65536.0f + 0.5f);  // drop when the 16-bit draw is below p * 2^16
  const size_t groups = (n + 7) / 8;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)std::min<size_t>((groups + 255) / 256, 1u << 16)), dim3(256), 0, s, mask,
                     n, thresh, seed, stream_id);
  return hipGetLastError();
}
__global__ void apply_mask_kernel(const float* __restrict__ a, const uint8_t* __restrict__ m, float scale,
                                  float* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = m[i] ? a[i] * scale : 0.f;
}
hipError_t launch_apply_mask(const float* a, const uint8_t* mask, float scale, float* out, size_t n, hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(apply_mask_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1u << 20)), dim3(256), 0, s, a, mask,
                     scale, out, n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Data movement
// ---------------------------------------------------------------------------
// dst[r][0..Cd) = src[r][0..Cs) zero-padded on the right (Cd >= Cs)
__global__ void pad_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t rows, int Cs, int Cd) {
  const size_t total = rows * Cd;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cd);
    const size_t r = i / Cd;
    dst[i] = c < Cs ? src[r * Cs + c] : 0.f;
  }
}
hipError_t launch_pad_cols(const float* src, float* dst, size_t rows, int Cs, int Cd, hipStream_t s) {
  const size_t total = rows * Cd;
  hipLaunchKernelGGL(pad_cols_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1u << 20)), dim3(256), 0, s, src, dst,
                     rows, Cs, Cd);
  return hipGetLastError();
}
// dst[r][0..cols) = src[r][0..cols) between two row-major matrices of different leading dimensions
__global__ void copy2d_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd, size_t rows, int cols) {
  const size_t total = rows * cols;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % cols);
    const size_t r = i / cols;
    dst[r * ldd + c] = src[r * lds + c];
  }
}
hipError_t launch_copy2d(const float* src, int lds, float* dst, int ldd, size_t rows, int cols, hipStream_t s) {
  const size_t total = rows * cols;
  hipLaunchKernelGGL(copy2d_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1u << 20)), dim3(256), 0, s, src, lds,
                     dst, ldd, rows, cols);
  return hipGetLastError();
}
// Zero-dilated, zero-padded copy of an NHWC map: dst[b][oh*SH + OFFH][ow*SW + OFFW][c] = src[b][oh][ow][c], rest 0.
// (input of the stride-1 convolution that evaluates the data gradient of a strided convolution)
__global__ void dilate_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int OH, int OW, int C, int DH,
                              int DW, int SH, int SW, int offh, int offw) {
  const size_t total = (size_t)B * DH * DW * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int w = (int)((i / C) % DW), h = (int)((i / ((size_t)C * DW)) % DH), b = (int)(i / ((size_t)C * DW * DH));
    const int hh = h - offh, ww = w - offw;
    float v = 0.f;
    if (hh >= 0 && ww >= 0 && hh % SH == 0 && ww % SW == 0 && hh / SH < OH && ww / SW < OW)
      v = src[(((size_t)b * OH + hh / SH) * OW + ww / SW) * C + c];
    dst[i] = v;
  }
}
hipError_t launch_dilate(const float* src, float* dst, int B, int OH, int OW, int C, int DH, int DW, int SH, int SW, int offh,
                         int offw, hipStream_t s) {
  const size_t total = (size_t)B * DH * DW * C;
  hipLaunchKernelGGL(dilate_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1u << 20)), dim3(256), 0, s, src, dst, B,
                     OH, OW, C, DH, DW, SH, SW, offh, offw);
  return hipGetLastError();
}
// Weights of the data-gradient convolution: out[ci][co][kh][kw] = w[co][ci][KH-1-kh][KW-1-kw]  (OIHW -> flipped IOHW)
__global__ void flip_oihw_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin, int KH, int KW) {
  const size_t total = (size_t)Cout * Cin * KH * KW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int kw = (int)(i % KW), kh = (int)((i / KW) % KH), co = (int)((i / ((size_t)KW * KH)) % Cout);
    const int ci = (int)(i / ((size_t)KW * KH * Cout));
    out[i] = w[(((size_t)co * Cin + ci) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)];
  }
}
hipError_t launch_flip_oihw(const float* w, float* out, int Cout, int Cin, int KH, int KW, hipStream_t s) {
  const size_t total = (size_t)Cout * Cin * KH * KW;
  hipLaunchKernelGGL(flip_oihw_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, w, out, Cout,
                     Cin, KH, KW);
  return hipGetLastError();
}
// rows gather / scatter between a [B][n+skip] token layout and the compact [B][n] one:
// dst[b*n + i][:] = src[(b*(n+skip) + skip + i)][:]  (gather)  or the inverse with zero skip rows (scatter)
__global__ void token_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int n, int skip, int D,
                                  int scatter) {
  const size_t total = (size_t)B * (scatter ? n + skip : n) * D;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    const size_t row = i / D;
    if (!scatter) {
      const size_t b = row / n, t = row % n;
      dst[i] = src[((b * (n + skip)) + skip + t) * D + c];
    } else {
      const size_t b = row / (n + skip), t = row % (n + skip);
      dst[i] = t < (size_t)skip ? 0.f : src[(b * n + (t - skip)) * D + c];
    }
  }
}
hipError_t launch_token_rows(const float* src, float* dst, int B, int n, int skip, int D, int scatter, hipStream_t s) {
  const size_t total = (size_t)B * (scatter ? n + skip : n) * D;
  hipLaunchKernelGGL(token_rows_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1u << 20)), dim3(256), 0, s, src,
                     dst, B, n, skip, D, scatter);
  return hipGetLastError();
}
// out[c] = sum_b x[(b*stride_rows + row) * D + c]   (cls-token gradient)
__global__ void sum_rows_strided_kernel(const float* __restrict__ x, float* __restrict__ out, int B, long long stride_rows,
                                        int row, int D) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= D) return;
  float a = 0.f;
  for (int b = 0; b < B; ++b) a += x[((size_t)b * stride_rows + row) * D + c];
  out[c] = a;
}
hipError_t launch_sum_rows_strided(const float* x, float* out, int B, long long stride_rows, int row, int D, hipStream_t s) {
  hipLaunchKernelGGL(sum_rows_strided_kernel, dim3((D + 127) / 128), dim3(128), 0, s, x, out, B, stride_rows, row, D);
  return hipGetLastError();
}

// Stem convolution (Cin = 1 or 3, 3x3, pad 1) in training mode: raw weights, no bias / BN (z = conv(x)).  Its weight
// gradient is stem_wgrad_kernel in train_wgrad.hip.  The image is NCHW planar; a "tap" below is (ci * 3 + kh) * 3 + kw, the
// OIHW order of the raw weights.
template <int CIN>
__global__ __launch_bounds__(256) void stem_raw_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                       float* __restrict__ z, int B, int H, int W, int Cout) {
  // a thread owns four consecutive output channels of one pixel: 9 * CIN image loads serve all four, the filter comes
  // from LDS as [tap][co] float4s, the store is 16 bytes
  constexpr int K = 9 * CIN;
  __shared__ __attribute__((aligned(16))) float ws[K][64];
  for (int i = threadIdx.x; i < K * Cout; i += 256) ws[i % K][i / K] = w[i];  // w is [co][K]
  __syncthreads();
  const int C4 = Cout >> 2;
  const size_t total = (size_t)B * H * W * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % C4) * 4;
    const int x = (int)((i / C4) % W), y = (int)((i / ((size_t)C4 * W)) % H), b = (int)(i / ((size_t)C4 * W * H));
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ih = y + kh - 1, iw = x + kw - 1;
          if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
            const float v = img[(((size_t)b * CIN + ci) * H + ih) * W + iw];
            const float4 w4 = *reinterpret_cast<const float4*>(&ws[(ci * 3 + kh) * 3 + kw][co]);
            a[0] = fmaf(v, w4.x, a[0]); a[1] = fmaf(v, w4.y, a[1]); a[2] = fmaf(v, w4.z, a[2]); a[3] = fmaf(v, w4.w, a[3]);
          }
        }
    *reinterpret_cast<float4*>(z + i * 4) = make_float4(a[0], a[1], a[2], a[3]);
  }
}
hipError_t launch_stem_raw(const float* img, const float* w, float* z, int B, int Cin, int H, int W, int Cout, hipStream_t s) {
  if (Cout % 4 || Cout > 64) return hipErrorInvalidValue;
  const size_t total = (size_t)B * H * W * (Cout / 4);
  const dim3 grid((unsigned)std::min<size_t>((total + 255) / 256, 1u << 16));
  if (Cin == 1) hipLaunchKernelGGL(stem_raw_kernel<1>, grid, dim3(256), 0, s, img, w, z, B, H, W, Cout);
  else if (Cin == 3) hipLaunchKernelGGL(stem_raw_kernel<3>, grid, dim3(256), 0, s, img, w, z, B, H, W, Cout);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// GlobalContext block in the training step (addon_module/visual_attention.py:147-165): x [B][HW][C]
// ---------------------------------------------------------------------------
// partial[b][z][c] = sum over the z-th pixel chunk of (w[b][p]) x[b][p][c];  grid (B, GC_CHUNKS), thread = 4 channels x
// pixel phase
__global__ __launch_bounds__(256) void gc_wpool_kernel(const float* __restrict__ x, const float* __restrict__ wts,
                                                       float* __restrict__ part, int HW, int C) {
  __shared__ float4 red[256];
  const int b = blockIdx.x, z = blockIdx.y, tid = threadIdx.x;
  const int q4 = C / 4;                  // float4 per pixel row
  const int cq = tid % q4, ph = tid / q4, nph = 256 / q4;  // C <= 512 -> q4 <= 128 -> at least two pixel phases
  const int per = (HW + GC_CHUNKS - 1) / GC_CHUNKS, p0 = z * per, p1 = min(HW, p0 + per);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ph < nph)
    for (int p = p0 + ph; p < p1; p += nph) {
      const float w = wts ? wts[(size_t)b * HW + p] : 1.f;
      const float4 v = *reinterpret_cast<const float4*>(x + ((size_t)b * HW + p) * C + cq * 4);
      acc.x = fmaf(w, v.x, acc.x); acc.y = fmaf(w, v.y, acc.y); acc.z = fmaf(w, v.z, acc.z); acc.w = fmaf(w, v.w, acc.w);
    }
  red[tid] = acc;
  __syncthreads();
  if (tid < q4) {  // fixed order over the phases: deterministic
    float4 t = red[tid];
    for (int k = 1; k < nph; ++k) {
      const float4 u = red[k * q4 + tid];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    *reinterpret_cast<float4*>(part + ((size_t)b * GC_CHUNKS + z) * C + tid * 4) = t;
  }
}
__global__ void gc_wpool_final_kernel(const float* __restrict__ part, float* __restrict__ out, int B, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i % C;
  float t = 0.f;
  for (int z = 0; z < GC_CHUNKS; ++z) t += part[((size_t)b * GC_CHUNKS + z) * C + c];
  out[i] = t;
}
hipError_t launch_gc_wpool(const float* x, const float* wts, float* part, float* out, int B, int HW, int C, hipStream_t s) {
  if (C % 4 || C > 512 || 256 / (C / 4) < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gc_wpool_kernel, dim3(B, GC_CHUNKS), dim3(256), 0, s, x, wts, part, HW, C);
  hipLaunchKernelGGL(gc_wpool_final_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, part, out, B, C);
  return hipGetLastError();
}
__global__ void gc_bcast_add_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out, size_t n4,
                                    int HW, int C) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * 4;
    const int c = (int)(e % C);
    const size_t b = e / ((size_t)HW * C);
    float4 v = reinterpret_cast<const float4*>(x)[i];
    const float4 a = *reinterpret_cast<const float4*>(y + b * C + c);
    v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    reinterpret_cast<float4*>(out)[i] = v;
  }
}
hipError_t launch_gc_bcast_add(const float* x, const float* y, float* out, int B, int HW, int C, hipStream_t s) {
  const size_t n4 = (size_t)B * HW * C / 4;
  hipLaunchKernelGGL(gc_bcast_add_kernel, dim3(ew_grid(n4)), dim3(EW_THREADS), 0, s, x, y, out, n4, HW, C);
  return hipGetLastError();
}
// one block per image: softmax statistics of the logits, then per pixel a = softmax, da = dctx . x; then dl = a (da - s)
// (da is taken against the pooled vector, dctx . (x[p] - ctx): dl = a (da - sum a da) cancels dctx . ctx, which is three
// orders of magnitude larger than what is left when the positions of a map resemble each other)
__global__ __launch_bounds__(512) void gc_pool_bwd_weights_kernel(const float* __restrict__ x, const float* __restrict__ logits,
                                                                  const float* __restrict__ dctx, const float* __restrict__ ctx,
                                                                  float* __restrict__ a_out, float* __restrict__ dl,
                                                                  float* __restrict__ sum_dl, int HW, int C) {
  __shared__ float red[24], dc[512], cx[512];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* l = logits + (size_t)b * HW;
  float* av = a_out + (size_t)b * HW;
  float* dv = dl + (size_t)b * HW;
  if (tid < C) { dc[tid] = dctx[(size_t)b * C + tid]; cx[tid] = ctx[(size_t)b * C + tid]; }
  float m = -INFINITY;
  for (int p = tid; p < HW; p += 512) m = fmaxf(m, l[p]);
  m = wmax(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = red[0];
#pragma unroll
  for (int w = 1; w < 8; ++w) m = fmaxf(m, red[w]);
  float sum = 0.f;
  for (int p = tid; p < HW; p += 512) sum += expf(l[p] - m);
  sum = wsum(sum);
  if (lane == 0) red[8 + wave] = sum;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < 8; ++w) tot += red[8 + w];
  const float inv = 1.f / tot;
  // da per pixel: one wave per pixel, lanes over channels
  float sacc = 0.f;
  for (int p = wave; p < HW; p += 8) {
    const float* xr = x + ((size_t)b * HW + p) * C;
    float d = 0.f;
    for (int c = lane; c < C; c += 64) d = fmaf(dc[c], xr[c] - cx[c], d);
    d = wsum(d);
    const float a = expf(l[p] - m) * inv;
    if (lane == 0) { av[p] = a; dv[p] = d; }
    sacc = fmaf(a, d, sacc);  // identical in every lane of the wave
  }
  if (lane == 0) red[16 + wave] = sacc;
  __syncthreads();
  float sdot = 0.f;
#pragma unroll
  for (int w = 0; w < 8; ++w) sdot += red[16 + w];
  __syncthreads();
  float sd = 0.f;
  for (int p = tid; p < HW; p += 512) {
    const float v = av[p] * (dv[p] - sdot);
    dv[p] = v;
    sd += v;
  }
  sd = wsum(sd);
  if (lane == 0) red[wave] = sd;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < 8; ++w) t += red[w];
    sum_dl[b] = t;
  }
}
hipError_t launch_gc_pool_bwd_weights(const float* x, const float* logits, const float* dctx, const float* ctx, float* a,
                                      float* dl, float* sum_dl, int B, int HW, int C, hipStream_t s) {
  if (C > 512) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gc_pool_bwd_weights_kernel, dim3(B), dim3(512), 0, s, x, logits, dctx, ctx, a, dl, sum_dl, HW, C);
  return hipGetLastError();
}
__global__ void gc_pool_bwd_dx_kernel(const float* __restrict__ a, const float* __restrict__ dl, const float* __restrict__ dctx,
                                      const float* __restrict__ wg, float* __restrict__ dx, size_t n4, int HW, int C) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * 4;
    const int c = (int)(e % C);
    const size_t row = e / C, b = row / HW;
    const float av = a[row], dv = dl[row];
    const float4 d = *reinterpret_cast<const float4*>(dctx + b * C + c);
    const float4 w = *reinterpret_cast<const float4*>(wg + c);
    reinterpret_cast<float4*>(dx)[i] = make_float4(fmaf(av, d.x, dv * w.x), fmaf(av, d.y, dv * w.y), fmaf(av, d.z, dv * w.z),
                                                   fmaf(av, d.w, dv * w.w));
  }
}
__global__ __launch_bounds__(64) void sum_small_kernel(const float* __restrict__ a, int n, float* __restrict__ dst) {
  float t = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) t += a[i];
  t = wsum(t);
  if (threadIdx.x == 0) dst[0] = t;
}
hipError_t launch_sum_small(const float* a, int n, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(sum_small_kernel, dim3(1), dim3(64), 0, s, a, n, dst);
  return hipGetLastError();
}
hipError_t launch_gc_pool_bwd_dx(const float* a, const float* dl, const float* dctx, const float* wg, float* dx, int B, int HW,
                                 int C, hipStream_t s) {
  const size_t n4 = (size_t)B * HW * C / 4;
  hipLaunchKernelGGL(gc_pool_bwd_dx_kernel, dim3(ew_grid(n4)), dim3(EW_THREADS), 0, s, a, dl, dctx, wg, dx, n4, HW, C);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// VGG + BidirectionalLSTM encoder in the training step
// ---------------------------------------------------------------------------
__global__ void bias_add_kernel(float* __restrict__ z, const float* __restrict__ bias, size_t n4, int C) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)((i * 4) % C);
    float4 v = reinterpret_cast<float4*>(z)[i];
    const float4 b = *reinterpret_cast<const float4*>(bias + c);
    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    reinterpret_cast<float4*>(z)[i] = v;
  }
}
hipError_t launch_bias_add(float* z, const float* bias, long long rows, int C, hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  const size_t n4 = (size_t)rows * C / 4;
  hipLaunchKernelGGL(bias_add_kernel, dim3(ew_grid(n4)), dim3(EW_THREADS), 0, s, z, bias, n4, C);
  return hipGetLastError();
}
__global__ void scale_kernel(const float* __restrict__ a, float* __restrict__ out, size_t n, float alpha) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = alpha * a[i];
}
hipError_t launch_scale(const float* a, float* out, size_t n, float alpha, hipStream_t s) {
  hipLaunchKernelGGL(scale_kernel, dim3(ew_grid((n + 3) / 4)), dim3(EW_THREADS), 0, s, a, out, n, alpha);
  return hipGetLastError();
}
__global__ void mean_h_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, size_t total, int H, int W, int C, float inv) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C), w = (int)((i / C) % W);
    const size_t b = i / ((size_t)C * W * H);
    dx[i] = dy[(b * W + w) * C + c] * inv;
  }
}
hipError_t launch_mean_h_bwd(const float* dy, float* dx, int B, int H, int W, int C, hipStream_t s) {
  const size_t total = (size_t)B * H * W * C;
  hipLaunchKernelGGL(mean_h_bwd_kernel, dim3(ew_grid((total + 3) / 4)), dim3(EW_THREADS), 0, s, dy, dx, total, H, W, C, 1.f / H);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// many small device-to-device copies in one launch (d2t_train_gather)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void multi_copy_kernel(const CopyChunk* __restrict__ table) {
  const CopyChunk c = table[blockIdx.x];
  const bool vec = ((reinterpret_cast<uintptr_t>(c.src) | reinterpret_cast<uintptr_t>(c.dst)) & 15) == 0;
  long long i = threadIdx.x;
  if (vec) {
    const long long n4 = c.n >> 2;
    for (; i < n4; i += 256) reinterpret_cast<float4*>(c.dst)[i] = reinterpret_cast<const float4*>(c.src)[i];
    for (i = (n4 << 2) + threadIdx.x; i < c.n; i += 256) c.dst[i] = c.src[i];
  } else {
    for (; i < c.n; i += 256) c.dst[i] = c.src[i];
  }
}
hipError_t launch_multi_copy(const CopyChunk* table, int chunks, hipStream_t s) {
  if (chunks <= 0) return hipSuccess;
  hipLaunchKernelGGL(multi_copy_kernel, dim3(chunks), dim3(256), 0, s, table);
  return hipGetLastError();
}

}  // namespace d2t
