// Non-GEMM kernels of the recognizer path (gfx950, 64-wide wavefronts, fp32).
// Each kernel names the reference op sequence it replaces (paths relative to
// /root/reference/doc2tex/modules/component/).
#include "conv_common.h"
#include "recurrent_common.h"  // wsum / wmax, block_sum / block_max

namespace d2t {

// One step of a grid-stride sweep over an NHWC map in quads of channels: element idx of [B][H][W][C / 4] is channels
// 4 c4 .. 4 c4 + 3 of pixel (b, y, x), whose row in the map is pix.
struct Quad {
  int c4, x, y;
  long long b, pix;
};
__device__ __forceinline__ Quad quad_at(long long idx, int cq, int H, int W) {
  Quad q;
  q.c4 = (int)(idx % cq);
  q.pix = idx / cq;
  q.x = (int)(q.pix % W);
  q.y = (int)((q.pix / W) % H);
  q.b = q.pix / ((long long)W * H);
  return q;
}

// ---------------------------------------------------------------------------
// conv0_1 + bn0_1 + ReLU (feature_extractor/resnet.py:206-208): Cin = 1 (grey) or 3 (rgb: True), 3x3 pad 1.
// HBM-write-bound: one thread = one pixel x 4 output channels, 16-B coalesced stores.
// The image is NCHW planar [B][CIN][H][W]; the weights are pack_conv's [Cout][kh][kw][CIN] (for CIN = 1 that is [Cout][9]).
// Accumulation order inside a pixel: channel-major, then kh, kw -- a = fmaf(v[c][kh][kw], w[oc][kh][kw][c], a) -- so the
// fp32 path has one defined result; the CIN = 1 instantiation is the nine-tap chain it has always been.
// ---------------------------------------------------------------------------
// the 3x3 neighbourhood of pixel (y, x) in every plane of image `im`, zero outside the image
template <int CIN>
__device__ __forceinline__ void stem_taps(const float* im, int y, int x, int H, int W, float (&v)[CIN][9]) {
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int yy = y + kh - 1, xx = x + kw - 1;
        // (plane offset added to the row offset: the 64-bit row product is shared by the planes)
        v[ci][kh * 3 + kw] = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
                                 ? im[(long long)ci * H * W + ((long long)yy * W + xx)] : 0.f;
      }
}
// one output channel before bias and activation: the fmaf chain in the order above over the taps w(ci, t)
template <int CIN, class TapW>
__device__ __forceinline__ float stem_chain(const float (&v)[CIN][9], TapW w) {
  float a = 0.f;
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
    for (int t = 0; t < 9; ++t) a = fmaf(v[ci][t], w(ci, t), a);
  return a;
}

// fp32 NHWC rows, any Cout % 4 == 0 (64: VGG, 32: ResNet); the taps are read from memory
template <int CIN>
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ out, int B,
                                                   int H, int W, int Cout, int act) {
  const int cq = Cout >> 2;
  const long long total = (long long)B * H * W * cq;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const Quad q = quad_at(idx, cq, H, W);
    float v[CIN][9], o[4];
    stem_taps<CIN>(img + q.b * CIN * H * W, q.y, q.x, H, W, v);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int oc = q.c4 * 4 + c;
      const float a = stem_chain<CIN>(v, [&](int ci, int t) { return w[(oc * 9 + t) * CIN + ci]; }) + (bias ? bias[oc] : 0.f);
      o[c] = act == ACT_RELU ? fmaxf(a, 0.f) : a;
    }
    store_row<4>(o, out + q.pix * Cout + q.c4 * 4);
  }
}

// split records of format fmt, Cout == 32
template <int CIN>
__global__ __launch_bounds__(256) void stem_split_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                         const float* __restrict__ bias, uint16_t* __restrict__ out,
                                                         int B, int H, int W, int Cout, int act, int fmt) {
  const int cq = Cout >> 2;  // == 8: the stride of the loop below is a multiple of 8, so a thread keeps its 4 channels
  const int c4 = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) % cq);
  // this thread's filter taps, loaded once (36 loads per pixel otherwise; 108 with three channels).  Every index below is a
  // compile-time constant after unrolling, so the 4 x 9 x CIN taps and the 9 x CIN pixels live in registers
  float wr[4][CIN][9], br[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    br[c] = bias ? bias[c4 * 4 + c] : 0.f;
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
      for (int t = 0; t < 9; ++t) wr[c][ci][t] = w[((c4 * 4 + c) * 9 + t) * CIN + ci];
  }
  const long long total = (long long)B * H * W * cq;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const Quad q = quad_at(idx, cq, H, W);
    float v[CIN][9], o[4];
    stem_taps<CIN>(img + q.b * CIN * H * W, q.y, q.x, H, W, v);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float a = stem_chain<CIN>(v, [&](int ci, int t) { return wr[c][ci][t]; }) + br[c];
      o[c] = act == ACT_RELU ? fmaxf(a, 0.f) : a;
    }
    store_rec<4>(o, out + plane_idx((size_t)q.pix, c4 * 4, Cout), fmt);
  }
}

hipError_t launch_stem_split(const float* img, const float* w, const float* bias, uint16_t* out, int B, int Cin, int H, int W,
                             int Cout, int act, hipStream_t s, int fmt) {
  if (Cout != 32) return hipErrorInvalidValue;  // 8 channel quads per pixel: see the kernel's hoisted weights
  const dim3 grid = grid_1d((size_t)B * H * W * (Cout / 4), 8192);
  if (Cin == 1) hipLaunchKernelGGL(stem_split_kernel<1>, grid, dim3(256), 0, s, img, w, bias, out, B, H, W, Cout, act, fmt);
  else if (Cin == 3) hipLaunchKernelGGL(stem_split_kernel<3>, grid, dim3(256), 0, s, img, w, bias, out, B, H, W, Cout, act, fmt);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_stem(const float* img, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, int Cout,
                       int act, hipStream_t s) {
  if (Cout % 4) return hipErrorInvalidValue;
  const dim3 grid = grid_1d((size_t)B * H * W * (Cout / 4), 8192);
  if (Cin == 1) hipLaunchKernelGGL(stem_kernel<1>, grid, dim3(256), 0, s, img, w, bias, out, B, H, W, Cout, act);
  else if (Cin == 3) hipLaunchKernelGGL(stem_kernel<3>, grid, dim3(256), 0, s, img, w, bias, out, B, H, W, Cout, act);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// nn.MaxPool2d(kernel 2) NHWC (resnet.py:94,106,120); padding behaves as -inf.
// ---------------------------------------------------------------------------
// How a pool reads and writes the four channels from c on of map row `row`: fp32 rows, or split records of format fmt.
struct PoolF32 {
  using T = float;
  static __device__ __forceinline__ void load(float (&v)[4], const float* x, long long row, int c, int C, int) {
    load_tile<4>(x + row * C + c, v);
  }
  static __device__ __forceinline__ void store(const float (&v)[4], float* y, long long row, int c, int C, int) {
    store_row<4>(v, y + row * C + c);
  }
};
struct PoolRec {
  using T = uint16_t;
  static __device__ __forceinline__ void load(float (&v)[4], const uint16_t* x, long long row, int c, int C, int fmt) {
    v[0] = v[1] = v[2] = v[3] = -0.f;  // (-0 + x == x for every x, a -0 included; 0 + -0 would read back as +0)
    add_rec<4>(v, x + plane_idx((size_t)row, c, C), fmt);
  }
  static __device__ __forceinline__ void store(const float (&v)[4], uint16_t* y, long long row, int c, int C, int fmt) {
    store_rec<4>(v, y + plane_idx((size_t)row, c, C), fmt);
  }
};
// One thread = one output pixel x 4 channels.  K2: the constant 2x2 window (KH, KW unused), else any window.
// first, step: the thread's grid-stride sweep.  The kernels form them: blockDim read in here would be lowered without the
// kernel's uniform-work-group guarantee, as a dependent load in front of the loop.
template <bool K2, class IO>
__device__ __forceinline__ void maxpool_body(const typename IO::T* __restrict__ x, typename IO::T* __restrict__ y, int B,
                                             int H, int W, int C, int OH, int OW, int KH, int KW, int SH, int SW, int PH,
                                             int PW, int fmt, long long first, long long step) {
  const int cq = C >> 2, kh_n = K2 ? 2 : KH, kw_n = K2 ? 2 : KW;
  const long long total = (long long)B * OH * OW * cq;
  for (long long idx = first; idx < total; idx += step) {
    const Quad q = quad_at(idx, cq, OH, OW);
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int kh = 0; kh < kh_n; ++kh)
      for (int kw = 0; kw < kw_n; ++kw) {
        const int ih = q.y * SH - PH + kh, iw = q.x * SW - PW + kw;
        if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
          float v[4];
          IO::load(v, x, (q.b * H + ih) * W + iw, q.c4 * 4, C, fmt);
#pragma unroll
          for (int c = 0; c < 4; ++c) m[c] = fmaxf(m[c], v[c]);
        }
      }
    IO::store(m, y, q.pix, q.c4 * 4, C, fmt);
  }
}

__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H,
                                                      int W, int C, int OH, int OW, int SH, int SW, int PH, int PW) {
  maxpool_body<true, PoolF32>(x, y, B, H, W, C, OH, OW, 2, 2, SH, SW, PH, PW, 0, (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}
__global__ __launch_bounds__(256) void maxpool_split_kernel(const uint16_t* __restrict__ xp, uint16_t* __restrict__ yp,
                                                            int B, int H, int W, int C, int OH, int OW, int SH, int SW,
                                                            int PH, int PW, int fmt) {
  maxpool_body<true, PoolRec>(xp, yp, B, H, W, C, OH, OW, 2, 2, SH, SW, PH, PW, fmt, (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}
// any window and stride (the VGG extractor's pools), same layout and padding rule
__global__ __launch_bounds__(256) void maxpool_k_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H,
                                                        int W, int C, int OH, int OW, int KH, int KW, int SH, int SW,
                                                        int PH, int PW) {
  maxpool_body<false, PoolF32>(x, y, B, H, W, C, OH, OW, KH, KW, SH, SW, PH, PW, 0, (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}

hipError_t launch_maxpool_split(const uint16_t* x, uint16_t* y, int B, int H, int W, int C, int SH, int SW, int PH,
                                int PW, hipStream_t s, int fmt) {
  if (C % 32) return hipErrorInvalidValue;
  const int OH = (H + 2 * PH - 2) / SH + 1, OW = (W + 2 * PW - 2) / SW + 1;
  hipLaunchKernelGGL(maxpool_split_kernel, grid_1d((size_t)B * OH * OW * (C / 4), 8192), dim3(256), 0, s, x, y, B, H, W, C, OH,
                     OW, SH, SW, PH, PW, fmt);
  return hipGetLastError();
}

hipError_t launch_maxpool(const float* x, float* y, int B, int H, int W, int C, int SH, int SW, int PH, int PW,
                          hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  const int OH = (H + 2 * PH - 2) / SH + 1, OW = (W + 2 * PW - 2) / SW + 1;
  hipLaunchKernelGGL(maxpool_kernel, grid_1d((size_t)B * OH * OW * (C / 4), 8192), dim3(256), 0, s, x, y, B, H, W, C, OH, OW,
                     SH, SW, PH, PW);
  return hipGetLastError();
}

hipError_t launch_maxpool_k(const float* x, float* y, int B, int H, int W, int C, int KH, int KW, int SH, int SW,
                            int PH, int PW, hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  const int OH = (H + 2 * PH - KH) / SH + 1, OW = (W + 2 * PW - KW) / SW + 1;
  hipLaunchKernelGGL(maxpool_k_kernel, grid_1d((size_t)B * OH * OW * (C / 4), 8192), dim3(256), 0, s, x, y, B, H, W, C, OH, OW,
                     KH, KW, SH, SW, PH, PW);
  return hipGetLastError();
}

__global__ void mean_h_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int C) {
  const long long total = (long long)B * W * C;
  const float inv = 1.f / (float)H;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const int w = (int)((idx / C) % W);
    const long long b = idx / ((long long)C * W);
    float s = 0.f;
    for (int h = 0; h < H; ++h) s += x[((b * H + h) * W + w) * C + c];
    y[idx] = s * inv;
  }
}
hipError_t launch_mean_h(const float* x, float* y, int B, int H, int W, int C, hipStream_t s) {
  hipLaunchKernelGGL(mean_h_kernel, grid_1d((size_t)B * W * C, 4096), dim3(256), 0, s, x, y, B, H, W, C);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// LayerNorm over the last dim, one wave per row, row in registers
// (vision_transformer.py:119-122 eps 1e-6; nn.TransformerDecoderLayer norms eps 1e-5).
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ b, float* __restrict__ y, int rows,
                                                        float eps) {
  constexpr int V = D / 256;  // float4 per lane
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (size_t)row * D;
  float4 v[V];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    v[i] = *reinterpret_cast<const float4*>(xr + (i * 64 + lane) * 4);
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float mean = wsum(s) * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
    q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
  }
  const float rstd = 1.f / sqrtf(wsum(q) * (1.f / D) + eps);
  float* yr = y + (size_t)row * D;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = (i * 64 + lane) * 4;
    const float4 gg = *reinterpret_cast<const float4*>(g + c);
    const float4 bb = *reinterpret_cast<const float4*>(b + c);
    float4 o;
    o.x = v[i].x * rstd * gg.x + bb.x;
    o.y = v[i].y * rstd * gg.y + bb.y;
    o.z = v[i].z * rstd * gg.z + bb.z;
    o.w = v[i].w * rstd * gg.w + bb.w;
    *reinterpret_cast<float4*>(yr + c) = o;
  }
}

hipError_t launch_layernorm(const float* x, const float* g, const float* b, float* y, int rows, int D, float eps,
                            hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const dim3 grid((rows + 3) / 4);
  if (D == 256) hipLaunchKernelGGL(layernorm_kernel<256>, grid, dim3(256), 0, s, x, g, b, y, rows, eps);
  else if (D == 512) hipLaunchKernelGGL(layernorm_kernel<512>, grid, dim3(256), 0, s, x, g, b, y, rows, eps);
  else if (D == 1024) hipLaunchKernelGGL(layernorm_kernel<1024>, grid, dim3(256), 0, s, x, g, b, y, rows, eps);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Weight packing: OIHW -> OHWI with eval-BatchNorm folded
//   w'[o][kh][kw][c] = w[o][c][kh][kw] * s[o],  s = gamma / sqrt(var + eps)
//   b'[o] = beta - mean * s  (+ conv_bias * s)
// ---------------------------------------------------------------------------
__global__ void pack_conv_kernel(const float* __restrict__ w, const float* __restrict__ cb,
                                 const float* __restrict__ g, const float* __restrict__ be,
                                 const float* __restrict__ mu, const float* __restrict__ var, float eps,
                                 float* __restrict__ wo, float* __restrict__ bo, int Cout, int Cin, int KH, int KW) {
  const long long total = (long long)Cout * Cin * KH * KW;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % Cin);
    const int kw = (int)((idx / Cin) % KW);
    const int kh = (int)((idx / ((long long)Cin * KW)) % KH);
    const int o = (int)(idx / ((long long)Cin * KW * KH));
    const float s = g ? g[o] / sqrtf(var[o] + eps) : 1.f;
    // K order of the packed weights = the order the conv kernels sweep K: 32-channel chunk outermost,
    // filter tap inside it, channel within the chunk innermost (see conv_common.h: advance_k)
    const size_t kdst = ((size_t)(c >> 5) * KH * KW + (size_t)kh * KW + kw) * 32 + (c & 31);
    const size_t dst = Cin % 32 == 0 ? (size_t)o * Cin * KH * KW + kdst : (size_t)idx;
    wo[dst] = w[(((size_t)o * Cin + c) * KH + kh) * KW + kw] * s;
    if (c == 0 && kw == 0 && kh == 0) {
      float bias = cb ? cb[o] * s : 0.f;
      if (g) bias += be[o] - mu[o] * s;
      bo[o] = bias;
    }
  }
}

hipError_t launch_pack_conv(const float* w_oihw, const float* conv_bias, const float* bn_w, const float* bn_b,
                            const float* bn_mean, const float* bn_var, float eps, float* w_out, float* bias_out,
                            int Cout, int Cin, int KH, int KW, hipStream_t s) {
  hipLaunchKernelGGL(pack_conv_kernel, grid_1d((size_t)Cout * Cin * KH * KW, 4096), dim3(256), 0, s, w_oihw, conv_bias, bn_w,
                     bn_b, bn_mean, bn_var, eps, w_out, bias_out, Cout, Cin, KH, KW);
  return hipGetLastError();
}

__global__ void repack_ohwi_kernel(const float* __restrict__ w, float* __restrict__ wo, int Cout, int KH, int KW, int Cin) {
  const long long total = (long long)Cout * KH * KW * Cin;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % Cin);
    const int tap = (int)((idx / Cin) % (KH * KW));
    const long long o = idx / ((long long)Cin * KH * KW);
    wo[o * Cin * KH * KW + ((size_t)(c >> 5) * KH * KW + tap) * 32 + (c & 31)] = w[idx];
  }
}
hipError_t launch_repack_ohwi(const float* w_ohwi, float* w_out, int Cout, int KH, int KW, int Cin, hipStream_t s) {
  hipLaunchKernelGGL(repack_ohwi_kernel, grid_1d((size_t)Cout * KH * KW * Cin, 4096), dim3(256), 0, s, w_ohwi, w_out, Cout,
                     KH, KW, Cin);
  return hipGetLastError();
}

__global__ void transpose_into_kernel(const float* __restrict__ src, int rows, int cols, float* __restrict__ dst,
                                      int ld, int row_off) {
  const long long total = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i / rows), r = (int)(i % rows);
    dst[(size_t)(row_off + c) * ld + r] = src[(size_t)r * cols + c];
  }
}
hipError_t launch_transpose_into(const float* src, int rows, int cols, float* dst, int ld, int row_off,
                                 hipStream_t s) {
  hipLaunchKernelGGL(transpose_into_kernel, grid_1d((size_t)rows * cols, 2048), dim3(256), 0, s, src, rows, cols, dst, ld,
                     row_off);
  return hipGetLastError();
}

hipError_t launch_copy(const float* src, float* dst, size_t n, hipStream_t s) {
  return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s);
}

__global__ void add_rows_kernel(const float* a, const float* b, float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}
hipError_t launch_add_rows(const float* a, const float* b, float* out, int n, hipStream_t s) {
  hipLaunchKernelGGL(add_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, b, out, n);
  return hipGetLastError();
}

__global__ void fill_cls_kernel(const float* row, float* out, long long img_stride, int D) {
  for (int i = threadIdx.x; i < D; i += blockDim.x) out[(long long)blockIdx.x * img_stride + i] = row[i];
}
hipError_t launch_fill_cls(const float* row, float* out, int B, long long img_stride_floats, int D, hipStream_t s) {
  hipLaunchKernelGGL(fill_cls_kernel, dim3(B), dim3(256), 0, s, row, out, img_stride_floats, D);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// GlobalContext block (addon_module/visual_attention.py:105-165; gcb: True): per image a 1x1-conv attention map over
// the H*W positions, softmax, attention-pooled channel vector, ConvMLP (fc1 -> LayerNorm -> ReLU -> fc2), added to
// every position.  x is NHWC fp32 [B][HW][C], modified in place.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gc_logits_kernel(const float* __restrict__ x, const float* __restrict__ wg,
                                                        const float* __restrict__ bg, float* __restrict__ logits,
                                                        long long rows, int C) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float a = 0.f;
  for (int c = lane; c < C; c += 64) a = fmaf(x[row * C + c], wg[c], a);
  a = wsum(a);
  if (lane == 0) logits[row] = a + bg[0];
}
// ctx[b][c] = sum_p softmax_p(logits[b])[p] * x[b][p][c];  one block per image
__global__ __launch_bounds__(512) void gc_pool_kernel(const float* __restrict__ x, const float* __restrict__ logits,
                                                      float* __restrict__ ctx, int HW, int C) {
  __shared__ float red[16], wts[512];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* l = logits + (size_t)b * HW;
  float m = -INFINITY;
  for (int p = tid; p < HW; p += 512) m = fmaxf(m, l[p]);
  m = block_max<8>(m, red, wave, lane);
  __syncthreads();
  float sum = 0.f;
  for (int p = tid; p < HW; p += 512) sum += expf(l[p] - m);
  const float inv = 1.f / block_sum<8>(sum, red + 8, wave, lane);
  float acc = 0.f;  // thread = channel (C <= 512)
  for (int p0 = 0; p0 < HW; p0 += 512) {
    __syncthreads();
    if (p0 + tid < HW) wts[tid] = expf(l[p0 + tid] - m) * inv;
    __syncthreads();
    const int n = HW - p0 < 512 ? HW - p0 : 512;
    if (tid < C)
      for (int p = 0; p < n; ++p) acc = fmaf(wts[p], x[((size_t)b * HW + p0 + p) * C + tid], acc);
  }
  if (tid < C) ctx[(size_t)b * C + tid] = acc;
}
// y[b] = fc2(relu(LayerNorm(fc1(ctx[b]))));  one block per image, thread = output channel (C <= 512)
__global__ __launch_bounds__(512) void gc_mlp_kernel(const float* __restrict__ ctx, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, const float* __restrict__ g,
                                                     const float* __restrict__ be, const float* __restrict__ w2,
                                                     const float* __restrict__ b2, float* __restrict__ y, int C) {
  __shared__ float v[512], h[512], red[16];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < C) v[tid] = ctx[(size_t)b * C + tid];
  __syncthreads();
  float a = 0.f;
  if (tid < C) {
    a = b1[tid];
    for (int k = 0; k < C; ++k) a = fmaf(v[k], w1[(size_t)tid * C + k], a);
  }
  const float mean = block_sum<8>(tid < C ? a : 0.f, red, wave, lane) / C;
  const float d = tid < C ? a - mean : 0.f;
  const float var = block_sum<8>(d * d, red + 8, wave, lane);
  const float rstd = 1.f / sqrtf(var / C + 1e-5f);
  if (tid < C) h[tid] = fmaxf(d * rstd * g[tid] + be[tid], 0.f);
  __syncthreads();
  if (tid < C) {
    float o = b2[tid];
    for (int k = 0; k < C; ++k) o = fmaf(h[k], w2[(size_t)tid * C + k], o);
    y[(size_t)b * C + tid] = o;
  }
}
__global__ void gc_add_kernel(float* __restrict__ x, const float* __restrict__ y, size_t n4, int HW, int C) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * 4;
    const int c = (int)(e % C);
    const size_t b = e / ((size_t)HW * C);
    float4 v = reinterpret_cast<float4*>(x)[i];
    const float4 a = *reinterpret_cast<const float4*>(y + b * C + c);
    v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    reinterpret_cast<float4*>(x)[i] = v;
  }
}
hipError_t launch_gc_logits(const float* x, const float* wg, const float* bg, float* logits, long long rows, int C, hipStream_t s) {
  hipLaunchKernelGGL(gc_logits_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, wg, bg, logits, rows, C);
  return hipGetLastError();
}
hipError_t launch_gc_pool(const float* x, const float* logits, float* ctx, int B, int HW, int C, hipStream_t s) {
  if (C > 512) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gc_pool_kernel, dim3(B), dim3(512), 0, s, x, logits, ctx, HW, C);
  return hipGetLastError();
}
hipError_t launch_global_context(float* x, const GCParams& w, float* logits, float* ctx, float* y, int B, int HW, int C,
                                 hipStream_t s) {
  if (C > 512 || C % 4) return hipErrorInvalidValue;
  const long long rows = (long long)B * HW;
  hipError_t e = launch_gc_logits(x, w.wg, w.bg, logits, rows, C, s);
  if (e == hipSuccess) e = launch_gc_pool(x, logits, ctx, B, HW, C, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gc_mlp_kernel, dim3(B), dim3(512), 0, s, ctx, w.w1, w.b1, w.ln_g, w.ln_b, w.w2, w.b2, y, C);
  const size_t n4 = (size_t)rows * C / 4;
  hipLaunchKernelGGL(gc_add_kernel, grid_1d(n4, 1u << 20), dim3(256), 0, s, x, y, n4, HW, C);
  return hipGetLastError();
}

}  // namespace d2t
