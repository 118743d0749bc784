// Decode-step kernels (gfx950, fp32): everything the KV-cached greedy / beam loop
// launches once per generated token.  Replaces, for the newest position only, what
// nn.TransformerDecoder recomputes over the whole prefix at every step in the
// reference (prediction_head/tfm.py:125-140).  All position-dependent values are
// read from a device-side step counter so one captured hipGraph replays for every step.
#include <cstdlib>

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

// ---------------------------------------------------------------------------
// Skinny GEMM  y[M,N] = act(A @ w[N,K]^T + bias + res),  A = x or LayerNorm(x).
// M <= 64 rows per block row (the decode batch), weights streamed from L2 straight
// into registers.  Block tile 64 x 16; the K dimension is split over the NW waves
// of the block (each wave: all 64 rows x its K-slice, v_mfma_f32_16x16x4_f32, every
// load issued before the first MFMA), partial tiles are summed through LDS.
// The optional LayerNorm prologue (post-norm decoder: the previous sub-layer's
// LayerNorm) is evaluated on the register-resident rows: two-pass mean / variance
// with a cross-wave LDS reduction, so no standalone LayerNorm launch is needed.
// ---------------------------------------------------------------------------
template <int NW, int NCH, int MT>  // K == NW * NCH * 16; block tile (16*MT) rows x 16 columns
__global__ __launch_bounds__(NW * 64) void skinny_splitk_kernel(const SkinnyP p) {
  if (p.stop_at && *p.stop_at && *p.cur_step >= *p.stop_at) return;  // block-uniform
  decode_wave_priority();
  TraceScope trace_(p.trace);
  constexpr int KS = NCH * 16;
  constexpr int ROWS = 16 * MT;
  __shared__ float part[NW][ROWS][17];
  __shared__ float stat[NW][ROWS];
  __shared__ float s_mean[ROWS], s_rstd[ROWS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, q = lane >> 4;
  const int mbase = blockIdx.y * ROWS;
  const int n = blockIdx.x * 16 + r;
  const bool nok = n < p.N;
  const int k0 = wave * KS + q * 4;

  float4 a[MT][NCH], b[NCH];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = mbase + i * 16 + r;
    const bool mok = m < p.M;
    const float* src = p.x + (size_t)(mok ? m : 0) * p.ldx + k0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      a[i][c] = *reinterpret_cast<const float4*>(src + c * 16);
      if (!mok) a[i][c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  {
    const float* src = p.w + (size_t)(nok ? n : 0) * (p.wld ? p.wld : p.K) + k0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      b[c] = *reinterpret_cast<const float4*>(src + c * 16);
      if (!nok) b[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  if (p.ln_g) {
    const float invK = 1.f / (float)p.K;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) s += (a[i][c].x + a[i][c].y) + (a[i][c].z + a[i][c].w);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (q == 0) stat[wave][i * 16 + r] = s;
    }
    __syncthreads();
    if (tid < ROWS) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += stat[w][tid];
      s_mean[tid] = t * invK;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const float mu = s_mean[i * 16 + r];
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        a[i][c].x -= mu; a[i][c].y -= mu; a[i][c].z -= mu; a[i][c].w -= mu;
        s += (a[i][c].x * a[i][c].x + a[i][c].y * a[i][c].y) + (a[i][c].z * a[i][c].z + a[i][c].w * a[i][c].w);
      }
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (q == 0) stat[wave][i * 16 + r] = s;
    }
    __syncthreads();
    if (tid < ROWS) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += stat[w][tid];
      s_rstd[tid] = 1.f / sqrtf(t * invK + p.ln_eps);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float4 g4 = *reinterpret_cast<const float4*>(p.ln_g + k0 + c * 16);
      const float4 b4 = *reinterpret_cast<const float4*>(p.ln_b + k0 + c * 16);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const float rs = s_rstd[i * 16 + r];
        a[i][c].x = a[i][c].x * rs * g4.x + b4.x;
        a[i][c].y = a[i][c].y * rs * g4.y + b4.y;
        a[i][c].z = a[i][c].z * rs * g4.z + b4.z;
        a[i][c].w = a[i][c].w * rs * g4.w + b4.w;
      }
    }
  }

  f32x4 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][c].x, b[c].x, acc[i], 0, 0, 0);
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][c].y, b[c].y, acc[i], 0, 0, 0);
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][c].z, b[c].z, acc[i], 0, 0, 0);
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][c].w, b[c].w, acc[i], 0, 0, 0);
    }
  }
  // C/D map: col = lane&15 -> n, row = (lane>>4)*4 + reg -> m
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) part[wave][i * 16 + q * 4 + reg][r] = acc[i][reg];
  __syncthreads();

  float* y = p.y;
  if (p.step_ptr) y += (long long)(*p.step_ptr) * p.out_step_stride;
  for (int idx = tid; idx < ROWS * 16; idx += NW * 64) {
    const int row = idx >> 4, col = idx & 15;
    const int m = mbase + row, nn = blockIdx.x * 16 + col;
    if (m >= p.M || nn >= p.N) continue;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += part[w][row][col];
    v += p.bias ? p.bias[nn] : 0.f;
    if (p.res) v += p.res[(size_t)m * p.ldres + nn];
    y[(size_t)m * p.ldy + nn] = act_fn(v, p.act);
    if (p.ln_out && nn < p.K) {
      const float xv = p.x[(size_t)m * p.ldx + nn];
      p.ln_out[(size_t)m * p.K + nn] = (xv - s_mean[row]) * s_rstd[row] * p.ln_g[nn] + p.ln_b[nn];
    }
  }
}

// ---------------------------------------------------------------------------
// Wide form of the same GEMM for decode groups (M >= SKINNY_WIDE_MIN_M rows, where the kernel above is bound by the
// L2 traffic of its many small blocks): NWV waves own a block tile of (16*TM) rows x (16*TN) columns, so that every
// operand row is fetched by fewer blocks and the LayerNorm prologue runs once per 16*TN columns instead of once per 16.
// BITWISE the split-K kernel: a wave owns (16 x 16 sub-tile, K slice) units -- slice w = wave % NW, the row sub-tiles
// split over the NWV/NW waves of a slice -- each with its own accumulator (the same 16x16x4 chain over c and x, y, z, w)
// and its own LDS partial; the slices are summed in ascending w from zero, then bias, residual, activation.  The
// LayerNorm statistics keep the per-(row, slice) lane sums and the ascending-slice sums of the kernel above, and ln_out
// is the A operand itself, written from the registers.
// Every global operand is requested before the first wait, the small ones first (the vector-memory counter retires in
// order): step, bias, residual tile, ln_g / ln_b, then the rows, then the weight rows.
// ---------------------------------------------------------------------------
template <int NW, int NCH, int TM, int TN, int NWV>  // K == NW * NCH * 16; NWV waves
__global__ __launch_bounds__(NWV * 64) void skinny_wide_kernel(const SkinnyP p) {
  if (p.stop_at && *p.stop_at && *p.cur_step >= *p.stop_at) return;  // block-uniform
  decode_wave_priority();
  TraceScope trace_(p.trace);
  constexpr int KS = NCH * 16, ROWS = 16 * TM, COLS = 16 * TN;
  constexpr int G = NWV / NW;       // waves per K slice
  constexpr int TMW = TM / G;       // row sub-tiles of one wave
  constexpr int WG = NWV / 4;       // the epilogue: thread = sub-tile (wave >> 2) + WG e, accumulator register wave & 3, lane
  constexpr int NE = TM * TN / WG;  // output elements per thread
  static_assert(NW * G == NWV && TMW * G == TM && NE * WG == TM * TN && WG * 4 == NWV, "the waves share the units evenly");
  __shared__ float part[NW][TM * TN][4][64];  // [slice][sub-tile][accumulator register][lane]
  __shared__ float stat[NW][ROWS];
  __shared__ float s_mean[ROWS], s_rstd[ROWS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, q = lane >> 4;
  const int w = wave % NW, i0 = (wave / NW) * TMW;
  const int mbase = blockIdx.y * ROWS, nbase = blockIdx.x * COLS;
  const int k0 = w * KS + q * 4;

  // ---- the epilogue's operands ----
  const long long yoff = p.step_ptr ? (long long)(*p.step_ptr) * p.out_step_stride : 0;
  float bias_v[NE], res_v[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int st = (wave >> 2) + WG * e;
    const int m = mbase + (st / TN) * 16 + q * 4 + (wave & 3), nn = nbase + (st % TN) * 16 + r;
    const bool ok = m < p.M && nn < p.N;
    bias_v[e] = p.bias && ok ? p.bias[nn] : 0.f;
    res_v[e] = p.res && ok ? p.res[(size_t)m * p.ldres + nn] : 0.f;
  }
  float4 g4[NCH], b4[NCH];
  if (p.ln_g) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      g4[c] = *reinterpret_cast<const float4*>(p.ln_g + k0 + c * 16);
      b4[c] = *reinterpret_cast<const float4*>(p.ln_b + k0 + c * 16);
    }
  }
  // ---- this wave's rows and weight rows, K slice w ----
  float4 a[TMW][NCH], b[TN][NCH];
#pragma unroll
  for (int i = 0; i < TMW; ++i) {
    const int m = mbase + (i0 + i) * 16 + r;
    const bool mok = m < p.M;
    const float* src = p.x + (size_t)(mok ? m : 0) * p.ldx + k0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      a[i][c] = *reinterpret_cast<const float4*>(src + c * 16);
      if (!mok) a[i][c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = nbase + j * 16 + r;
      const bool nok = n < p.N;
      b[j][c] = *reinterpret_cast<const float4*>(p.w + (size_t)(nok ? n : 0) * (p.wld ? p.wld : p.K) + k0 + c * 16);
      if (!nok) b[j][c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  if (p.ln_g) {
    const float invK = 1.f / (float)p.K;
#pragma unroll
    for (int i = 0; i < TMW; ++i) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) s += (a[i][c].x + a[i][c].y) + (a[i][c].z + a[i][c].w);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (q == 0) stat[w][(i0 + i) * 16 + r] = s;
    }
    __syncthreads();
    if (tid < ROWS) {
      float t = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) t += stat[ww][tid];
      s_mean[tid] = t * invK;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TMW; ++i) {
      const float mu = s_mean[(i0 + i) * 16 + r];
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        a[i][c].x -= mu; a[i][c].y -= mu; a[i][c].z -= mu; a[i][c].w -= mu;
        s += (a[i][c].x * a[i][c].x + a[i][c].y * a[i][c].y) + (a[i][c].z * a[i][c].z + a[i][c].w * a[i][c].w);
      }
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (q == 0) stat[w][(i0 + i) * 16 + r] = s;
    }
    __syncthreads();
    if (tid < ROWS) {
      float t = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) t += stat[ww][tid];
      s_rstd[tid] = 1.f / sqrtf(t * invK + p.ln_eps);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TMW; ++i) {
      const float rs = s_rstd[(i0 + i) * 16 + r];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        a[i][c].x = a[i][c].x * rs * g4[c].x + b4[c].x;
        a[i][c].y = a[i][c].y * rs * g4[c].y + b4[c].y;
        a[i][c].z = a[i][c].z * rs * g4[c].z + b4[c].z;
        a[i][c].w = a[i][c].w * rs * g4[c].w + b4[c].w;
      }
    }
    // ln_out: the normalised rows are the A operand itself, (x - mean) * rstd * g + b; a (row, column) has one writer,
    // the block whose column tile holds that column (N >= K: launch_skinny)
    if (p.ln_out) {
#pragma unroll
      for (int i = 0; i < TMW; ++i) {
        const int m = mbase + (i0 + i) * 16 + r;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int k = k0 + c * 16;
          if (m < p.M && k / COLS == (int)blockIdx.x) *reinterpret_cast<float4*>(p.ln_out + (size_t)m * p.K + k) = a[i][c];
        }
      }
    }
  }

  f32x4 acc[TMW][TN];
#pragma unroll
  for (int i = 0; i < TMW; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // per accumulator the chain runs over c and x, y, z, w in that order; the TMW * TN independent chains are interleaved
#define D2T_WIDE_MFMA(f)                                                                                     \
  _Pragma("unroll") for (int i = 0; i < TMW; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j)             \
    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][c].f, b[j][c].f, acc[i][j], 0, 0, 0)
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    D2T_WIDE_MFMA(x);
    D2T_WIDE_MFMA(y);
    D2T_WIDE_MFMA(z);
    D2T_WIDE_MFMA(w);
  }
#undef D2T_WIDE_MFMA
#pragma unroll
  for (int i = 0; i < TMW; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) part[w][(i0 + i) * TN + j][reg][lane] = acc[i][j][reg];
  __syncthreads();

  // C/D map: col = lane&15 -> n, row = (lane>>4)*4 + reg -> m
  float* y = p.y + yoff;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int st = (wave >> 2) + WG * e;
    const int m = mbase + (st / TN) * 16 + q * 4 + (wave & 3), nn = nbase + (st % TN) * 16 + r;
    if (m >= p.M || nn >= p.N) continue;
    float v = 0.f;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) v += part[ww][st][wave & 3][lane];
    v += bias_v[e];
    if (p.res) v += res_v[e];
    y[(size_t)m * p.ldy + nn] = act_fn(v, p.act);
  }
}

// generic fallback (any K % 16 == 0, no LayerNorm prologue): one wave per 16 rows
__global__ __launch_bounds__(256) void skinny_generic_kernel(const SkinnyP p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int m = blockIdx.y * 64 + wave * 16 + r;
  const int n = blockIdx.x * 16 + r;
  const bool mok = m < p.M, nok = n < p.N;
  const float* xa = p.x + (size_t)(mok ? m : 0) * p.ldx + q * 4;
  const float* wb = p.w + (size_t)(nok ? n : 0) * p.K + q * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int KC = p.K >> 4;
  for (int c = 0; c < KC; ++c) {
    float4 a = *reinterpret_cast<const float4*>(xa + c * 16);
    float4 b = *reinterpret_cast<const float4*>(wb + c * 16);
    if (!mok) a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!nok) b = make_float4(0.f, 0.f, 0.f, 0.f);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  }
  const int nn = blockIdx.x * 16 + r;
  if (nn >= p.N) return;
  float* y = p.y;
  if (p.step_ptr) y += (long long)(*p.step_ptr) * p.out_step_stride;
  const float bias = p.bias ? p.bias[nn] : 0.f;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int mm = blockIdx.y * 64 + wave * 16 + q * 4 + reg;
    if (mm >= p.M) continue;
    float v = acc[reg] + bias;
    if (p.res) v += p.res[(size_t)mm * p.ldres + nn];
    y[(size_t)mm * p.ldy + nn] = act_fn(v, p.act);
  }
}

// small = 1: the 256-thread forms of the decode kernels (one wave per SIMD, <= 128 VGPRs), which fit on a CU beside the
// pipelined convolution kernel's three 128-register waves per SIMD; identical arithmetic per row, so identical results
static int decode_small() {
  static const int v = D2T_PROBE_ENV("D2T_DECODE_SMALL");
  return v;
}

template <int NW, int NCH, int TM, int TN, int NWV>
static void launch_skinny_wide(const SkinnyP& p, hipStream_t s) {
  const dim3 grid((p.N + 16 * TN - 1) / (16 * TN), (p.M + 16 * TM - 1) / (16 * TM));
  hipLaunchKernelGGL((skinny_wide_kernel<NW, NCH, TM, TN, NWV>), grid, dim3(NWV * 64), 0, s, p);
}

hipError_t launch_skinny(const SkinnyP& p, hipStream_t s) { return launch_skinny_form(p, SKINNY_FORM_AUTO, s); }

hipError_t launch_skinny_form(const SkinnyP& p, int form, hipStream_t s) {
  if (p.M <= 0 || p.N <= 0) return hipSuccess;
  if (p.K % 16 != 0 || p.ldx % 4 != 0) return hipErrorInvalidValue;
  // ln_out[m][nn] is written by the block that owns output column nn: all K columns exist only when N >= K
  if (p.ln_out && (!p.ln_g || p.N < p.K)) return hipErrorInvalidValue;
  const bool wide_k = p.K == 256 || p.K == 512 || p.K == 1024;
  // measured alone on the chip: from 384 rows on the wide form is the faster one at K = 256 and 1024
  if (form == SKINNY_FORM_AUTO)
    form = (p.K == 256 || p.K == 1024) && p.M >= SKINNY_WIDE_MIN_M && !decode_small() ? SKINNY_FORM_WIDE : SKINNY_FORM_SPLITK;
  if (form == SKINNY_FORM_WIDE) {
    if (!wide_k) return hipErrorInvalidValue;
    if (p.K == 256 && p.N > 512) launch_skinny_wide<4, 4, 2, 4, 4>(p, s);  // 32 x 64, four waves
    else if (p.K == 256) launch_skinny_wide<4, 4, 2, 2, 4>(p, s);          // narrow outputs: 32 x 32
    else if (p.K == 512) launch_skinny_wide<8, 4, 2, 2, 8>(p, s);          // 32 x 32, eight waves
    else launch_skinny_wide<8, 8, 2, 1, 8>(p, s);                          // 32 x 16
    return hipGetLastError();
  }
  if (form != SKINNY_FORM_SPLITK) return hipErrorInvalidValue;
  // narrow outputs (N <= 512) take 16-row tiles so that the few column tiles still fill >= 64 CUs
  const int mt = p.N <= 512 ? 1 : 2;
  const dim3 grid((p.N + 15) / 16, (p.M + 16 * mt - 1) / (16 * mt));
#define D2T_SK(NW, NCH)                                                                                  \
  do {                                                                                                   \
    if (mt == 1) hipLaunchKernelGGL((skinny_splitk_kernel<NW, NCH, 1>), grid, dim3(NW * 64), 0, s, p);   \
    else hipLaunchKernelGGL((skinny_splitk_kernel<NW, NCH, 2>), grid, dim3(NW * 64), 0, s, p);           \
  } while (0)
  if (p.K == 256) D2T_SK(4, 4);
  else if (p.K == 512) D2T_SK(8, 4);
  else if (p.K == 1024 && decode_small() && !p.ln_g && !p.step_ptr) {
    // two 256-thread passes over the halves of K (second pass accumulates onto the first through the residual input)
    SkinnyP a = p, b = p;
    a.K = 512; a.ldx = p.ldx; a.w = p.w; a.wld = p.K;
    b.K = 512; b.x = p.x + 512; b.w = p.w + 512; b.wld = p.K; b.bias = nullptr; b.res = p.y; b.ldres = p.ldy;
    a.act = ACT_NONE;
    if (p.act != ACT_NONE) return hipErrorInvalidValue;
    hipLaunchKernelGGL((skinny_splitk_kernel<4, 8, 1>), dim3((p.N + 15) / 16, (p.M + 15) / 16), dim3(256), 0, s, a);
    hipLaunchKernelGGL((skinny_splitk_kernel<4, 8, 1>), dim3((p.N + 15) / 16, (p.M + 15) / 16), dim3(256), 0, s, b);
  }
  else if (p.K == 1024) D2T_SK(8, 8);
  else {
    if (p.ln_g) return hipErrorInvalidValue;
    hipLaunchKernelGGL(skinny_generic_kernel, dim3((p.N + 15) / 16, (p.M + 63) / 64), dim3(256), 0, s, p);
  }
#undef D2T_SK
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Single-query multi-head attention for one decode step: one block (4 waves) per
// (row, head).  K and V rows of a head are contiguous, so a wave-wide 16-B load
// covers 64/(HD/4) whole keys: fully coalesced.  Each wave takes every 4th group of
// keys, keeps a wave-local (max, sum, weighted V) triple and the four triples are
// merged through LDS (log-sum-exp combine).  Self-attention mode appends this
// step's k,v to the cache.  Replaces nn.MultiheadAttention inside
// nn.TransformerDecoderLayer (tfm.py:130) for the newest position.
// ---------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256) void decode_attention_kernel(const DecAttnP p) {
  constexpr int LPK = HD / 4;          // lanes per key
  constexpr int KPI = 64 / LPK;        // keys per wave-iteration
  constexpr int MAXIT = 512 / (KPI * 4);
  __shared__ float w_m[4], w_s[4];
  __shared__ __attribute__((aligned(16))) float w_acc[4][HD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int kig = lane / LPK, ch = lane % LPK;
  const int b = blockIdx.x / p.heads, head = blockIdx.x % p.heads;
  int L = p.L, t = -1;
  if (p.step_ptr) { t = *p.step_ptr; L = t + 1; }
  float* Kc = p.k + (size_t)b * p.kv_batch_stride + (size_t)head * p.Lmax * HD;
  float* Vc = p.v + (size_t)b * p.kv_batch_stride + (size_t)head * p.Lmax * HD;
  const float* curk = p.cur_k ? p.cur_k + (size_t)b * p.cur_stride + head * HD : nullptr;
  const float* curv = p.cur_v ? p.cur_v + (size_t)b * p.cur_stride + head * HD : nullptr;
  if (curk && t >= 0 && tid < HD) {  // append this step's k,v to the cache
    Kc[(size_t)t * HD + tid] = curk[tid];
    Vc[(size_t)t * HD + tid] = curv[tid];
  }
  const float4 q4 = *reinterpret_cast<const float4*>(p.q + (size_t)b * p.q_stride + head * HD + ch * 4);
  const float scale = HD == 32 ? 0.17677669529663687f : 0.125f;
  const int nit = (L + KPI * 4 - 1) / (KPI * 4);  // iterations of this block (wave-uniform)

  float sc[MAXIT];
  float mloc = -INFINITY;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    sc[it] = -INFINITY;
    if (it < nit) {
      const int j = (it * 4 + wave) * KPI + kig;
      float d = 0.f;
      if (j < L) {
        const float* kr = (curk && j == t) ? curk : Kc + (size_t)j * HD;
        const float4 k4 = *reinterpret_cast<const float4*>(kr + ch * 4);
        d = (q4.x * k4.x + q4.y * k4.y) + (q4.z * k4.z + q4.w * k4.w);
      }
#pragma unroll
      for (int o = 1; o < LPK; o <<= 1) d += __shfl_xor(d, o, 64);
      if (j < L) {
        sc[it] = d * scale;
        mloc = fmaxf(mloc, sc[it]);
      }
    }
  }
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) mloc = fmaxf(mloc, __shfl_xor(mloc, o, 64));
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float ssum = 0.f;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    if (it < nit) {
      const int j = (it * 4 + wave) * KPI + kig;
      if (j < L) {
        const float pj = expf(sc[it] - mloc);
        const float* vr = (curv && j == t) ? curv : Vc + (size_t)j * HD;
        const float4 v4 = *reinterpret_cast<const float4*>(vr + ch * 4);
        ssum += pj;
        acc.x = fmaf(pj, v4.x, acc.x); acc.y = fmaf(pj, v4.y, acc.y);
        acc.z = fmaf(pj, v4.z, acc.z); acc.w = fmaf(pj, v4.w, acc.w);
      }
    }
  }
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) {
    ssum += __shfl_xor(ssum, o, 64);
    acc.x += __shfl_xor(acc.x, o, 64); acc.y += __shfl_xor(acc.y, o, 64);
    acc.z += __shfl_xor(acc.z, o, 64); acc.w += __shfl_xor(acc.w, o, 64);
  }
  if (kig == 0) *reinterpret_cast<float4*>(&w_acc[wave][ch * 4]) = acc;
  if (lane == 0) { w_m[wave] = mloc; w_s[wave] = ssum; }
  __syncthreads();
  if (tid < HD) {
    const float m = fmaxf(fmaxf(w_m[0], w_m[1]), fmaxf(w_m[2], w_m[3]));
    float tot = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = w_s[w] > 0.f ? expf(w_m[w] - m) : 0.f;  // waves without keys contribute nothing
      tot += w_s[w] * f;
      o += w_acc[w][tid] * f;
    }
    p.y[(size_t)b * p.y_stride + head * HD + tid] = o / tot;
  }
}

hipError_t launch_decode_attention(const DecAttnP& p, hipStream_t s) {
  const int Lcap = p.step_ptr ? p.Lmax : p.L;
  if (Lcap > 512 || Lcap < 1) return hipErrorInvalidValue;
  const dim3 grid(p.B * p.heads);
  if (p.hd == 32) hipLaunchKernelGGL(decode_attention_kernel<32>, grid, dim3(256), 0, s, p);
  else if (p.hd == 64) hipLaunchKernelGGL(decode_attention_kernel<64>, grid, dim3(256), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// _embedd_tgt (tfm.py:86-94) for the newest position: Embedding * sqrt(d) + WordPosEnc row t.
// ---------------------------------------------------------------------------
__global__ void embed_kernel(const float* __restrict__ emb, const float* __restrict__ pe,
                             const int64_t* __restrict__ start, const int64_t* __restrict__ tokens, int tok_stride,
                             const int* __restrict__ step_ptr, float* __restrict__ x, int d, float sqrt_d) {
  const int b = blockIdx.x, t = *step_ptr;
  const int64_t tok = t == 0 ? start[b] : tokens[(size_t)b * tok_stride + t - 1];
  for (int c = threadIdx.x; c < d; c += blockDim.x)
    x[(size_t)b * d + c] = emb[(size_t)tok * d + c] * sqrt_d + pe[(size_t)t * d + c];
}

hipError_t launch_embed(const float* emb, const float* pe, const int64_t* start, const int64_t* tokens,
                        int tok_stride, const int* step_ptr, float* x, int B, int d, hipStream_t s) {
  hipLaunchKernelGGL(embed_kernel, dim3(B), dim3(256), 0, s, emb, pe, start, tokens, tok_stride, step_ptr, x, d,
                     sqrtf((float)d));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Greedy next token (tfm.py:134-139) for every row + the next step's input
// embedding + step counter increment, one block.  First maximum wins ties;
// end-of-sequence bookkeeping stays on the device.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void argmax_embed_kernel(const ArgmaxP p) {
  const int t = *p.step_ptr;
  if (p.stop_at && *p.stop_at && t >= *p.stop_at) return;  // block-uniform; set by an EARLIER launch only (t + 1 > t)
  decode_wave_priority();
  TraceScope trace_(p.trace);
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* row = p.logits + (size_t)b * p.row_stride + (size_t)t * p.step_stride;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = lane; i < p.V; i += 64) {
    const float v = row[i];
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (bi >= p.V) bi = 0;  // all-NaN row: keep indexing in range
  if (p.x) {
    const float sqrt_d = sqrtf((float)p.d);
    const float* e = p.emb + (size_t)bi * p.d;
    const float* pe = p.pe + (size_t)(t + 1) * p.d;
    for (int c = lane; c < p.d; c += 64) p.x[(size_t)b * p.d + c] = e[c] * sqrt_d + pe[c];
  }
  if (lane == 0) {
    p.tokens[(size_t)b * p.tok_stride + t] = bi;
    if (bi == p.end_token && !p.ended[b]) {
      p.ended[b] = 1;
      const int c = atomicAdd(p.end_count, 1) + 1;
      if (c == p.B) *p.steps_done = t + 1;
      if (p.n_batches > 0) {  // decode group: this row's encoder batch may have finished (a ragged group passes ARGMAX_GROUPED
                              // here and its real batch count through n_batches_ptr)
        // uniform group: batch = b / rows_per_batch; ragged group (row_batch != nullptr): the layout comes from device tables, so
        // that one captured loop serves every layout with the same row total
        const int k = p.row_batch ? p.row_batch[b] : b / p.rows_per_batch;
        const int rows_k = p.batch_rows ? p.batch_rows[k] : p.rows_per_batch;
        const int nb = p.n_batches_ptr ? *p.n_batches_ptr : p.n_batches;
        if (atomicAdd(p.batch_end_count + k, 1) + 1 == rows_k) {
          p.batch_steps_done[k] = t + 1;
          // every block of THIS launch read step t before the stop takes effect (t < t + 1); the kernels of step t + 1 see it
          if (atomicAdd(p.batches_done, 1) + 1 == nb && p.stop_at) *p.stop_at = t + 1;
        }
      }
    }
    // every block has read the step counter before it arrives here, so the
    // last arriver may advance it (the kernel boundary publishes the store)
    __threadfence();
    if (atomicAdd(p.done_count, 1) == p.B - 1) {
      *p.done_count = 0;
      *p.step_ptr = t + 1;
    }
  }
}

hipError_t launch_argmax_embed(const ArgmaxP& p, hipStream_t s) {
  hipLaunchKernelGGL(argmax_embed_kernel, dim3(p.B), dim3(64), 0, s, p);
  return hipGetLastError();
}

// Ragged decode group with the device-side early exit: the loop runs until the LAST batch has ended, so the rows of a batch
// that ended earlier were decoded past their batch's exit.  One block per row clears tokens (PAD = 0) and logits of the steps
// [batch_steps_done[batch of the row], S): every batch comes back as its single-batch is_test decode leaves its buffers.
__global__ __launch_bounds__(256) void ragged_finalize_kernel(int64_t* __restrict__ tokens, float* __restrict__ logits,
                                                              const int* __restrict__ row_batch, const int* __restrict__ batch_steps_done,
                                                              int S, int V) {
  const int b = blockIdx.x;
  const int n = batch_steps_done[row_batch[b]];
  if (n <= 0 || n >= S) return;  // the batch never ended: all S steps are its result
  for (int t = n + threadIdx.x; t < S; t += 256) tokens[(size_t)b * S + t] = 0;
  float* l = logits + ((size_t)b * S + n) * V;
  const size_t cnt = (size_t)(S - n) * V;
  for (size_t i = threadIdx.x; i < cnt; i += 256) l[i] = 0.f;
}

hipError_t launch_ragged_finalize(int64_t* tokens, float* logits, const int* row_batch, const int* batch_steps_done, int B, int S,
                                  int V, hipStream_t s) {
  if (B < 1) return hipSuccess;
  hipLaunchKernelGGL(ragged_finalize_kernel, dim3(B), dim3(256), 0, s, tokens, logits, row_batch, batch_steps_done, S, V);
  return hipGetLastError();
}

// The online-softmax arithmetic of the d_model 512 row kernels' attention loops (head dim 64), spelled with explicit fmaf.
// decoder_row2_kernel promises the one-row kernel's bits per row; written as a * b + c * d the compiler's contraction may fuse
// either product, and chose differently in the two loops (tests/test_decode_ops_gpu.py: the builds differed by 1-3 ulp).
// Head dim 32 keeps the plain expressions below: its results are pinned bit for bit by arrays dumped from earlier builds
// (tests/golden/rgb_grey_baseline.npz), and no two builds of it promise each other's bits.
__device__ __forceinline__ float att_dot4(const float4& q, const float4& k) {
  return fmaf(q.x, k.x, q.y * k.y) + fmaf(q.z, k.z, q.w * k.w);
}
__device__ __forceinline__ void att_update(float sj, const float4& v, float& m, float& l, float4& acc) {
  const float mn = fmaxf(m, sj);
  const float f = expf(m - mn);  // exp(-inf) = 0 on the first key
  const float pj = expf(sj - mn);
  l = fmaf(l, f, pj);
  acc.x = fmaf(pj, v.x, acc.x * f); acc.y = fmaf(pj, v.y, acc.y * f);
  acc.z = fmaf(pj, v.z, acc.z * f); acc.w = fmaf(pj, v.w, acc.w * f);
  m = mn;
}
// (m, l, acc) += lane ^ o's triple (log-sum-exp combine of two key groups)
__device__ __forceinline__ void att_merge(int o, float& m, float& l, float4& acc) {
  const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
  const float ax = __shfl_xor(acc.x, o, 64), ay = __shfl_xor(acc.y, o, 64);
  const float az = __shfl_xor(acc.z, o, 64), aw = __shfl_xor(acc.w, o, 64);
  const float mn = fmaxf(m, mo);
  const float f1 = l > 0.f ? expf(m - mn) : 0.f, f2 = lo > 0.f ? expf(mo - mn) : 0.f;
  l = fmaf(lo, f2, l * f1);
  acc.x = fmaf(ax, f2, acc.x * f1); acc.y = fmaf(ay, f2, acc.y * f1);
  acc.z = fmaf(az, f2, acc.z * f1); acc.w = fmaf(aw, f2, acc.w * f1);
  m = mn;
}

template <int HD, int U>  // U key groups fetched together: 2*U 16-B loads in flight per lane
__device__ __forceinline__ void row_attention(const float* q, const float* Kc, const float* Vc, const float* curk,
                                              const float* curv, int t, int L, float* out, int lane,
                                              const int* anc = nullptr, long long anc_stride = 0) {
  // anc != nullptr (beam search, DecRowP::anc): position j < t of this hypothesis lives in cache row anc[j]; Kc / Vc then
  // point at cache row 0 of the head and anc_stride is the cache's row stride
  constexpr int LPK = HD / 4, KPI = 64 / LPK;
  const int kig = lane / LPK, ch = lane % LPK;
  const float4 q4 = *reinterpret_cast<const float4*>(q + ch * 4);
  const float scale = HD == 32 ? 0.17677669529663687f : 0.125f;
  float m = -INFINITY, l = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int nit = (L + KPI - 1) / KPI;
  for (int it0 = 0; it0 < nit; it0 += U) {
    float4 k4[U], v4[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = (it0 + u) * KPI + kig;
      const int jj = j < L ? j : 0;
      const size_t ro = (anc && jj != t) ? (size_t)anc[jj] * (size_t)anc_stride : 0;
      const float* kr = (curk && jj == t) ? curk : Kc + ro + (size_t)jj * HD;
      const float* vr = (curv && jj == t) ? curv : Vc + ro + (size_t)jj * HD;
      k4[u] = *reinterpret_cast<const float4*>(kr + ch * 4);
      v4[u] = *reinterpret_cast<const float4*>(vr + ch * 4);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = (it0 + u) * KPI + kig;
      float d = HD == 64 ? att_dot4(q4, k4[u]) : (q4.x * k4[u].x + q4.y * k4[u].y) + (q4.z * k4[u].z + q4.w * k4[u].w);
#pragma unroll
      for (int o = 1; o < LPK; o <<= 1) d += __shfl_xor(d, o, 64);
      if (j < L) {
        if constexpr (HD == 64) {
          att_update(d * scale, v4[u], m, l, acc);
        } else {
          const float sj = d * scale;
          const float mn = fmaxf(m, sj);
          const float f = expf(m - mn);  // exp(-inf) = 0 on the first key
          const float pj = expf(sj - mn);
          l = l * f + pj;
          acc.x = acc.x * f + pj * v4[u].x; acc.y = acc.y * f + pj * v4[u].y;
          acc.z = acc.z * f + pj * v4[u].z; acc.w = acc.w * f + pj * v4[u].w;
          m = mn;
        }
      }
    }
  }
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) {  // merge the key groups (log-sum-exp combine)
    if constexpr (HD == 64) {
      att_merge(o, m, l, acc);
    } else {
      const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
      const float ax = __shfl_xor(acc.x, o, 64), ay = __shfl_xor(acc.y, o, 64);
      const float az = __shfl_xor(acc.z, o, 64), aw = __shfl_xor(acc.w, o, 64);
      const float mn = fmaxf(m, mo);
      const float f1 = l > 0.f ? expf(m - mn) : 0.f, f2 = lo > 0.f ? expf(mo - mn) : 0.f;
      l = l * f1 + lo * f2;
      acc.x = acc.x * f1 + ax * f2; acc.y = acc.y * f1 + ay * f2;
      acc.z = acc.z * f1 + az * f2; acc.w = acc.w * f1 + aw * f2;
      m = mn;
    }
  }
  if (kig == 0) {
    const float inv = 1.f / l;
    *reinterpret_cast<float4*>(out + ch * 4) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The phases of the per-row decoder step, one copy each.  Every row kernel below is a sequence of these calls and barriers:
// self-attention over the cache, W_o + residual, LN1, W_q, cross-attention, W_co + residual.
// ---------------------------------------------------------------------------------------------------------------------
// Entry of a row kernel.  A finished step loop (stop_at: set by an EARLIER launch only) and a dead row slot return at once, both
// block-uniform; the rest runs at the decode priority inside the launch's trace record.
#define ROW_KERNEL_ENTRY(p, dead_row)                                       \
  if ((p).stop_at && *(p).stop_at && *(p).step_ptr >= *(p).stop_at) return; \
  if (dead_row) return;                                                     \
  decode_wave_priority();                                                   \
  TraceScope trace_((p).trace)

__device__ __forceinline__ void fma4(float a, const float4& w, float4& acc) {
  acc.x = fmaf(a, w.x, acc.x); acc.y = fmaf(a, w.y, acc.y); acc.z = fmaf(a, w.z, acc.z); acc.w = fmaf(a, w.w, acc.w);
}
__device__ __forceinline__ float4 scale4(const float4& a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

// out_part[g][n] = sum_{k in group g} in[k] * Wt[k][n]; caller reduces over g after a barrier (sum_parts).
// CTX_HD != 0: in_s holds [heads][D] context rows and column n reads the row of ITS head n / CTX_HD (the value projection behind
// the absorbed cross-attention)
template <int D, int NTH, int CTX_HD = 0>
__device__ __forceinline__ void row_gemv(const float* in_s, const float* __restrict__ Wt, float* part_s, int tid) {
  constexpr int LPR = D / 4, G = NTH / LPR, KG = D / G;
  const int lr = tid % LPR, g = tid / LPR;
  const float* w = Wt + (size_t)(g * KG) * D + lr * 4;
  const float* in = in_s + (CTX_HD ? ((lr * 4) / CTX_HD) * D : 0) + g * KG;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < KG; ++k) fma4(in[k], *reinterpret_cast<const float4*>(w + (size_t)k * D), acc);
  *reinterpret_cast<float4*>(part_s + g * D + lr * 4) = acc;
}
// one GEMV for two rows: every weight element is fetched once and applied to both inputs.  Thread (lr, g) -> columns
// 4 lr .. 4 lr + 3, k in [g KG, (g + 1) KG): per row the products and their order are row_gemv's
template <int D, int NTH, int UNROLL>
__device__ __forceinline__ void gemv2(const float* in0, const float* in1, const float* __restrict__ Wt, float* part0, float* part1,
                                      int tid) {
  constexpr int LPR = D / 4, G = NTH / LPR, KG = D / G;
  const int lr = tid % LPR, g = tid / LPR;
  const float* w = Wt + (size_t)(g * KG) * D + lr * 4;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
#pragma unroll UNROLL
  for (int k = 0; k < KG; ++k) {
    const float4 w4 = *reinterpret_cast<const float4*>(w + (size_t)k * D);
    const float x0 = in0[g * KG + k], x1 = in1[g * KG + k];
    fma4(x0, w4, a0);
    fma4(x1, w4, a1);
  }
  *reinterpret_cast<float4*>(part0 + g * D + lr * 4) = a0;
  *reinterpret_cast<float4*>(part1 + g * D + lr * 4) = a1;
}

// v0 + the G partial sums of column c, in ascending g
template <int G, int D>
__device__ __forceinline__ float sum_parts(const float* part, int c, float v) {
#pragma unroll
  for (int g = 0; g < G; ++g) v += part[g * D + c];
  return v;
}

// LN1 of one row by one wave, two-pass; gamma / beta: (i, c) -> the scale / shift of channel c = 64 i + lane
template <int D, class Gamma, class Beta>
__device__ __forceinline__ void row_ln1(const float* y_row, float* x1_row, int lane, float eps, Gamma gamma, Beta beta) {
  constexpr int V = D / 64;
  float v[V], s = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i) { v[i] = y_row[i * 64 + lane]; s += v[i]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i) { v[i] -= mean; q += v[i] * v[i]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = 1.f / sqrtf(q * (1.f / D) + eps);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = i * 64 + lane;
    x1_row[c] = v[i] * rstd * gamma(i, c) + beta(i, c);
  }
}
template <int D>
__device__ __forceinline__ void row_ln1(const float* y_row, float* x1_row, int lane, const DecRowP& p) {
  row_ln1<D>(y_row, x1_row, lane, p.eps, [&](int, int c) { return p.ln1_g[c]; }, [&](int, int c) { return p.ln1_b[c]; });
}

// Head `head` of row b in front of the self-attention: this step's K / V go into the cache at position t (store == false: the
// repeated last row of an odd row count keeps its stores to itself); returns the head's operands for row_attention[_2h]
struct HeadPtrs { const float *q, *K, *V, *curk, *curv; };
template <int D, int HD>
__device__ __forceinline__ HeadPtrs cache_append_and_heads(const DecRowP& p, int b, int head, int t, int lane, bool store) {
  const float* qkv = p.qkv + (size_t)b * p.qkv_stride;
  float* Kc = p.sk + (size_t)b * p.s_batch_stride + (size_t)head * p.s_Lmax * HD;
  float* Vc = p.sv + (size_t)b * p.s_batch_stride + (size_t)head * p.s_Lmax * HD;
  const float* curk = qkv + D + head * HD;
  const float* curv = qkv + 2 * D + head * HD;
  if (lane < HD && store) {
    Kc[(size_t)t * HD + lane] = curk[lane];
    Vc[(size_t)t * HD + lane] = curv[lane];
  }
  return {qkv + head * HD, Kc, Vc, curk, curv};
}
// the operands of row_attention_2h: two heads of one row, or one head of two rows
struct HeadPair {
  const float *q[2], *K[2], *V[2], *curk[2], *curv[2];
  float* out[2];
  __device__ __forceinline__ void set(int i, const HeadPtrs& h, float* o) {
    q[i] = h.q; K[i] = h.K; V[i] = h.V; curk[i] = h.curk; curv[i] = h.curv; out[i] = o;
  }
};
// one head of the one-row kernels: cache append + attention over positions 0 .. t.  ANC (beam search, DecRowP::anc): position
// j < t of this hypothesis lives in cache row anc_s[j] (no cache copy per step)
template <int D, int HD, bool ANC = false>
__device__ __forceinline__ void row_self_attention(const DecRowP& p, int b, int head, int t, int lane, float* out,
                                                   const int* anc_s = nullptr) {
  const HeadPtrs h = cache_append_and_heads<D, HD>(p, b, head, t, lane, true);
  if (ANC && p.anc)
    row_attention<HD, 4>(h.q, p.sk + (size_t)head * p.s_Lmax * HD, p.sv + (size_t)head * p.s_Lmax * HD, h.curk, h.curv, t, t + 1, out,
                         lane, anc_s, p.s_batch_stride);
  else
    row_attention<HD, 4>(h.q, h.K, h.V, h.curk, h.curv, t, t + 1, out, lane);
}

// ---------------------------------------------------------------------------
// Fused row kernel (see DecRowP).  512 threads = 8 waves = 8 heads.
// ---------------------------------------------------------------------------
template <int D, int HD, int NTH>  // NTH = 512: one wave per head; 256: four waves, two heads each (<= 128 VGPRs, so that a
                                    // block fits on a CU next to the pipelined convolution's three waves per SIMD)
__global__ __launch_bounds__(NTH, NTH == 256 ? 4 : 2) void decoder_row_kernel(const DecRowP p) {
  constexpr int G = NTH / (D / 4);
  constexpr int HPW = 8 * 64 / NTH;  // heads per wave
  ROW_KERNEL_ENTRY(p, false);
  __shared__ __attribute__((aligned(16))) float a_s[D], y_s[D], x1_s[D], q2_s[D], part_s[G * D];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int t = *p.step_ptr;
  // ---- self-attention, one head per wave (and pass) ----
#pragma unroll
  for (int hp = 0; hp < HPW; ++hp) {
    const int head = wave + hp * (NTH / 64);
    row_self_attention<D, HD>(p, b, head, t, lane, a_s + head * HD);
  }
  __syncthreads();
  row_gemv<D, NTH>(a_s, p.wo_t, part_s, tid);
  __syncthreads();
  if (tid < D) y_s[tid] = sum_parts<G, D>(part_s, tid, p.bo[tid] + p.xres[(size_t)b * D + tid]);
  __syncthreads();
  if (wave == 0) row_ln1<D>(y_s, x1_s, lane, p);
  __syncthreads();
  row_gemv<D, NTH>(x1_s, p.wq_t, part_s, tid);
  __syncthreads();
  if (tid < D) q2_s[tid] = sum_parts<G, D>(part_s, tid, p.bq[tid]);
  __syncthreads();
  // ---- cross-attention over the memory K/V, one head per wave (and pass) ----
#pragma unroll
  for (int hp = 0; hp < HPW; ++hp) {
    const int head = wave + hp * (NTH / 64);
    const int cb = p.c_row_map ? p.c_row_map[b] : b;
    const float* Kc = p.ck + (size_t)cb * p.c_batch_stride + (size_t)head * p.T * HD;
    const float* Vc = p.cv + (size_t)cb * p.c_batch_stride + (size_t)head * p.T * HD;
    row_attention<HD, 8>(q2_s + head * HD, Kc, Vc, nullptr, nullptr, -1, p.T, a_s + head * HD, lane);
  }
  __syncthreads();
  row_gemv<D, NTH>(a_s, p.wco_t, part_s, tid);
  __syncthreads();
  if (tid < D) p.y2[(size_t)b * D + tid] = sum_parts<G, D>(part_s, tid, p.bco[tid] + x1_s[tid]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Row kernel, round 3: cross-attention over the encoder MEMORY itself ("absorbed" projections).
//
// The kernel above streams, per row and layer, the projected K and V of its sample: 2 * T * D floats (534 KB at T = 261,
// D = 256) that are different for every layer -- 1.23 GB per decode step at 384 rows, the whole cost of the step.  But
//     score_h[j] = q_h . (W_k,h m_j + b_k,h) = (W_k,h^T q_h) . m_j + const_h          (the constant cancels in the softmax)
//     out_h      = sum_j p_hj (W_v,h m_j + b_v,h) = W_v,h (sum_j p_hj m_j) + b_v,h     (sum_j p_hj = 1)
// so a head can attend over the D-wide memory rows directly with the absorbed query q'_h = W_k,h^T q_h (D floats per head),
// and project the attention-weighted memory row afterwards.  Per row and layer that reads T * D floats (267 KB) -- the SAME
// bytes for all six layers, 102 MB for 384 rows: resident in the 256 MB Infinity Cache for the whole step loop -- and the
// 2 x 205 MB projected-K/V buffers, their GEMM per batch and the per-layer streams disappear.  The price is arithmetic:
// 8 heads x T x D multiply-adds for the scores and again for the weighted sum (8 x the head-dim form).  It goes to the
// matrix cores in exact fp32 (v_mfma_f32_16x16x4_f32, an fp32 fma chain per output like the VALU code it replaces):
//     S^T [16 keys x 16 (8 heads + 8 idle)] = M_tile [16 x D] . Q'^T [D x 16]            64 MFMAs per 16-key tile
//     ctx [16 (8 heads + 8 idle) x D]      += P [16 x 16 keys] . M_tile [16 x D]          64 MFMAs per tile
// A wave owns the key tiles w, w + NW, ...: it copies a tile (16 rows x 1 KB) into its private 16 KB of LDS with LDS-DMA
// (the 16-byte chunks of row i XOR-ed with i on the source side, so that both fragment patterns -- 16 keys x 4 channel
// groups for the scores, 4 keys x 16 channel groups for the weighted sum -- read without bank conflicts:
// tools/probe/lds_swizzle_check.py), keeps an online softmax per head (running max and sum, flash-decoding), and the waves'
// partial (max, sum, ctx) triples are merged through LDS.  The S^T product is taken transposed on purpose: its result
// layout (lane = (key group g, head), registers = keys 4g..4g+3) IS the A-operand layout of the second product with
// k-step s <-> register s, so P never moves between lanes.
// Everything else (self-attention over the cache, the row GEMVs, LN1) is the phase helpers above.
// ---------------------------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_ptr_dec;

#ifdef D2T_PROBES
// probe builds: block 0 / thread 0 adds the time between consecutive marks (s_memrealtime, 10 ns ticks) to d2t_row_phase[k]
__device__ unsigned long long d2t_row_phase[32];
#define ROW_PHASE(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); \
    atomicAdd(&d2t_row_phase[k], now_ - phase_t_); phase_t_ = now_; } } while (0)
#define ROW_PHASE_INIT() unsigned long long phase_t_ = __builtin_amdgcn_s_memrealtime(); if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&d2t_row_phase[31], 1ull)
#define WAVE_PHASE(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); \
    atomicAdd(&d2t_row_phase[k], now_ - wave_t_); wave_t_ = now_; } } while (0)
#define WAVE_PHASE_INIT() unsigned long long wave_t_ = __builtin_amdgcn_s_memrealtime()
#define ROW_PROBE(bit) (p.probe & (bit))
#else
#define ROW_PHASE(k) do { } while (0)
#define ROW_PHASE_INIT() do { } while (0)
#define WAVE_PHASE(k) do { } while (0)
#define WAVE_PHASE_INIT() do { } while (0)
#define ROW_PROBE(bit) 0
#endif

// LDS-DMA of key tile `tile` of `mem` into a wave's 16 KB stage: row i -> stage + i * 1024, physical 16-byte chunk c holds
// logical chunk c ^ i
__device__ __forceinline__ void cross_tile_dma(const float* __restrict__ mem, int T, int tile, unsigned char* stage, int lane) {
  const int j0 = tile << 4;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = j0 + i < T ? j0 + i : T - 1;  // rows past the end: a valid row, its probability is forced to zero
    __builtin_amdgcn_global_load_lds(mem + (size_t)j * 256 + ((lane ^ i) << 2), (lds_ptr_dec)(stage + i * 1024), 16, 0, 0);
  }
}

// Online softmax of one 16-key score tile: this lane holds keys j0 + 4 g + reg of one query row (head) in sacc.  Updates the
// row's running max / sum; pv = the keys' probabilities against the new max, ar[reg] = the rescale of accumulator register reg
// (the accumulators hold ctx[row 4 g + reg][...]: their scale is the alpha of THAT row, lane 4 g + reg has it)
__device__ __forceinline__ void online_softmax_tile(const f32x4& sacc, int j0, int g, int T, float& m_run, float& l_run,
                                                    float (&pv)[4], float (&ar)[4]) {
  float sv[4], mx = -INFINITY;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    sv[reg] = (j0 + 4 * g + reg < T) ? sacc[reg] : -INFINITY;
    mx = fmaxf(mx, sv[reg]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // a tile holds at least one valid key: finite
  const float m_new = fmaxf(m_run, mx);
  const float alpha = expf(m_run - m_new);  // exp(-inf) = 0 for the first tile
  float ps = 0.f;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    pv[reg] = expf(sv[reg] - m_new);  // exp(-inf) = 0 for keys past the end
    ps += pv[reg];
  }
  l_run = l_run * alpha + ps;
  m_run = m_new;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) ar[reg] = __shfl(alpha, 4 * g + reg, 64);
}

// this wave's share of the cross-attention of ONE query row set: heads x T keys of `mem` [T][256].
// qp_s: LDS [8][256] absorbed queries (already scaled by 1/sqrt(head_dim); the 16-byte chunks of row h XOR-ed with h like
// the tile rows); stage: this wave's 16 KB; results: the wave's
// running max / sum per head (lanes with col < 8, reduced over the key groups) and ctx accumulators acc[w][e] (D layout).
// How a tile arrives: PF == false, by LDS-DMA in front of its arithmetic; PF == true, the wave's first tile was started with
// cross_tile_dma long before, and every following tile travels to registers during the arithmetic on the current one and moves
// to LDS when its reads are done.  Same products, same order.
template <int NW, bool PF>
__device__ __forceinline__ void cross_absorbed_wave(const float* __restrict__ mem, int T, const float* qp_s, unsigned char* stage,
                                                    int wave, int lane, float& m_run, float& l_run, f32x4 (&acc)[4][4]) {
  const int col = lane & 15, g = lane >> 4;
  // B operand of the score product: q'[head = col][16u + 4g + t], re-read from LDS per tile (16 reads against 128 MFMAs; in
  // registers it would cost 64 VGPRs and the second block per CU).  The idle half of the MFMA tile (columns 8..15) repeats
  // heads 0..7: its results are never stored, and identical addresses broadcast.
  const int hrow = col & 7;
  m_run = -INFINITY;
  l_run = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[w][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntiles = (T + 15) >> 4;
  if constexpr (PF) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the first tile (issued at kernel entry) has landed
  WAVE_PHASE_INIT();
  for (int tile = wave; tile < ntiles; tile += NW) {
    const int j0 = tile << 4;
    const int nxt = tile + NW;
    WAVE_PHASE(13);
    f32x4 pf[16];
    if constexpr (PF) {
      if (nxt < ntiles) {  // wave-uniform
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int j = (nxt << 4) + i < T ? (nxt << 4) + i : T - 1;
          pf[i] = *reinterpret_cast<const f32x4*>(mem + (size_t)j * 256 + ((lane ^ i) << 2));
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) pf[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the previous tile's fragment reads have returned
      cross_tile_dma(mem, T, tile, stage, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    WAVE_PHASE(14);
    // ---- S^T[key = 4g' + reg][head = col] = sum_c m[key][c] q'[head][c] ----
    f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      // A operand: lane (row = key col, k = g) -> m[key][16u + 4g + t]; logical chunk 4u + g of row `col`
      const float4 a4 = *reinterpret_cast<const float4*>(stage + col * 1024 + (((4 * u + g) ^ col) << 4));
      const float4 q4 = *reinterpret_cast<const float4*>(reinterpret_cast<const unsigned char*>(qp_s) + hrow * 1024 + (((4 * u + g) ^ hrow) << 4));
      sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, q4.x, sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, q4.y, sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, q4.z, sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, q4.w, sacc, 0, 0, 0);
    }
    WAVE_PHASE(15);
    float pv[4], ar[4];
    online_softmax_tile(sacc, j0, g, T, m_run, l_run, pv, ar);
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) acc[w][e][reg] *= ar[reg];
    WAVE_PHASE(16);
    // ---- ctx[head][64w + 4 col' + e] += sum_keys P[head][key] m[key][chan]; k-step s <-> keys 4g + s ----
#pragma unroll
    for (int sk = 0; sk < 4; ++sk) {
      const int key = 4 * g + sk;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        // B operand: lane (k = g, col) -> m[key][64w + 4 col + e]; logical chunk 16w + col of row `key`
        const float4 b4 = *reinterpret_cast<const float4*>(stage + key * 1024 + (((16 * w + col) ^ key) << 4));
        acc[w][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[sk], b4.x, acc[w][0], 0, 0, 0);
        acc[w][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[sk], b4.y, acc[w][1], 0, 0, 0);
        acc[w][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[sk], b4.z, acc[w][2], 0, 0, 0);
        acc[w][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[sk], b4.w, acc[w][3], 0, 0, 0);
      }
    }
    WAVE_PHASE(17);
    if constexpr (PF) {
      if (nxt < ntiles) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this tile's fragment reads have returned: the stage may be overwritten
#pragma unroll
        for (int i = 0; i < 16; ++i) *reinterpret_cast<f32x4*>(stage + i * 1024 + lane * 16) = pf[i];
      }
    }
    WAVE_PHASE(18);
  }
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
}

// ---------------------------------------------------------------------------------------------------------------------
// Cross-attention on split-bf16 MFMAs (round 4).  Inside the loop below the fp32-MFMA form is bound by the matrix pipe:
// 128 v_mfma_f32_16x16x4_f32 per tile at 32 cycles, two waves per SIMD, and only 8 of the 16 columns (heads) of every tile
// useful -- 15 of the loop's 28 us (probe build, tools/probe/row_phases.py).  The same products on the bf16 pipe, every fp32
// operand as hi + lo (three MFMAs per product, lo*hi + hi*lo + hi*hi: the arithmetic of the encoder's GEMMs):
//     S^T [16 keys x 16 (8 heads + 8 idle)] = M_tile [16 x 256] . Q'^T      8 K-steps x 3 v_mfma_f32_16x16x32_bf16   (24)
//     ctx [16 (8 heads + 8 idle) x 256]    += P [16 x 16 keys] . M_tile     16 column blocks x 3 v_mfma_f32_16x16x16_bf16 (48)
// 72 MFMAs of 16 cycles instead of 128 of 32.  The memory rows arrive as two bf16 planes (hi = bf16_rne(x), lo =
// bf16_rne(x - hi): x to 16 or more significant bits; launch_split_bf16 at cross_kv time); a tile = 16 rows x 512 B of hi | 16 x 512 B of lo in the wave's
// 16 KB stage, 16-byte chunk c of row r at position c ^ r (conflict-free ds_read_b128 of the score product's A operand; the
// weighted sum's B operand [keys x channels] comes out of the same image with ds_read_b64_tr_b16).  The absorbed queries
// and the probabilities are split in registers (split16 below: hi = upper 16 bits, lo = bf16_rne(x - hi)).  The score product's result layout (lane = (key group, head), registers =
// keys 4g..4g+3) is the A-operand layout of the 16x16x16 form, so P never moves between lanes, as before.
// ---------------------------------------------------------------------------------------------------------------------
typedef __bf16 dbf16x8 __attribute__((ext_vector_type(8)));
typedef short ds4 __attribute__((ext_vector_type(4)));
typedef unsigned du32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) ds4* lds_ds4_ptr;
__device__ __forceinline__ void split16(float x, unsigned& hi, unsigned& lo) {  // hi = upper 16 bits, lo = bf16_rne(x - hi)
  const unsigned u = __float_as_uint(x);
  hi = u >> 16;
  const __bf16 l = (__bf16)(x - __uint_as_float(u & 0xFFFF0000u));
  lo = *reinterpret_cast<const unsigned short*>(&l);
}
// global source of the 16 bytes lane `lane` holds of piece i (0..15) of tile `tile`: pieces 0-7 = two hi rows each, 8-15 = lo
__device__ __forceinline__ const uint16_t* bx3_piece_src(const uint16_t* __restrict__ mh, const uint16_t* __restrict__ ml, int T, int tile,
                                                         int i, int lane) {
  const int row = 2 * (i & 7) + (lane >> 5);
  const int jr = (tile << 4) + row, j = jr < T ? jr : T - 1;  // rows past the end: a valid row, its probability is forced to zero
  return (i < 8 ? mh : ml) + (size_t)j * 256 + (((lane & 31) ^ row) << 3);
}
__device__ __forceinline__ void bx3_tile_dma(const uint16_t* __restrict__ mh, const uint16_t* __restrict__ ml, int T, int tile,
                                             unsigned char* stage, int lane) {
#pragma unroll
  for (int i = 0; i < 16; ++i)
    __builtin_amdgcn_global_load_lds(bx3_piece_src(mh, ml, T, tile, i, lane), (lds_ptr_dec)(stage + i * 1024), 16, 0, 0);
}
// this wave's share of the cross-attention of one query row: acc[cb][reg] = ctx[head 4 g + reg][channel 16 cb + col] (unnormalised)
template <int NW>
__device__ __forceinline__ void cross_absorbed_wave_bx3(const uint16_t* __restrict__ mh, const uint16_t* __restrict__ ml, int T,
                                                        const unsigned char* qp_b, unsigned char* stage, int wave, int lane,
                                                        float& m_run, float& l_run, f32x4 (&acc)[16]) {
  const int col = lane & 15, g = lane >> 4, hrow = col & 7;
  m_run = -INFINITY;
  l_run = 0.f;
#pragma unroll
  for (int cb = 0; cb < 16; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntiles = (T + 15) >> 4;
  // transposing-read addresses of the weighted sum's B operand: lane 4 q' + p of a 16-lane group supplies row 4 g + q' of the
  // block, channels 4 p .. 4 p + 3 of the column block; with the row's chunk swizzle: chunk (2 cb + (p >> 1)) ^ row
  const int trow = 4 * g + ((lane & 15) >> 2), tp = lane & 3;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the first tile (issued at kernel entry) has landed
  WAVE_PHASE_INIT();
  for (int tile = wave; tile < ntiles; tile += NW) {
    const int j0 = tile << 4;
    const int nxt = tile + NW;
    WAVE_PHASE(13);
    du32x4 pf[16];
    if (nxt < ntiles) {  // wave-uniform: the next tile travels to registers during this tile's arithmetic
#pragma unroll
      for (int i = 0; i < 16; ++i) pf[i] = *reinterpret_cast<const du32x4*>(bx3_piece_src(mh, ml, T, nxt, i, lane));
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) pf[i] = du32x4{0u, 0u, 0u, 0u};
    }
    WAVE_PHASE(14);
    // ---- S^T[key = 4 g' + reg][head = col]: A = tile rows (key = col), B = absorbed queries (head = col & 7) ----
    f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int ch = 4 * ks + g;  // logical 16-byte chunk (8 channels) of this lane's k-group
      const dbf16x8 ah = *reinterpret_cast<const dbf16x8*>(stage + col * 512 + ((ch ^ col) << 4));
      const dbf16x8 al = *reinterpret_cast<const dbf16x8*>(stage + 8192 + col * 512 + ((ch ^ col) << 4));
      const dbf16x8 bh = *reinterpret_cast<const dbf16x8*>(qp_b + hrow * 512 + ((ch ^ hrow) << 4));
      const dbf16x8 bl = *reinterpret_cast<const dbf16x8*>(qp_b + 4096 + hrow * 512 + ((ch ^ hrow) << 4));
      sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, sacc, 0, 0, 0);
    }
    WAVE_PHASE(15);
    float pv[4], ar[4];
    online_softmax_tile(sacc, j0, g, T, m_run, l_run, pv, ar);
    unsigned ph[4], pl[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) split16(pv[reg], ph[reg], pl[reg]);
#pragma unroll
    for (int cb = 0; cb < 16; ++cb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) acc[cb][reg] *= ar[reg];
    const ds4 pah = {(short)ph[0], (short)ph[1], (short)ph[2], (short)ph[3]}, pal = {(short)pl[0], (short)pl[1], (short)pl[2], (short)pl[3]};
    WAVE_PHASE(16);
    // ---- ctx[head][16 cb + col] += sum_keys P[head][key] m[key][channel]: A = P (head = col, keys 4 g .. 4 g + 3), B by transposing reads ----
#pragma unroll
    for (int cb = 0; cb < 16; ++cb) {
      const int off = trow * 512 + (((2 * cb + (tp >> 1)) ^ trow) << 4) + (tp & 1) * 8;
      const ds4 bh = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ds4_ptr)(stage + off));
      const ds4 bl = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ds4_ptr)(stage + 8192 + off));
      acc[cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pal, bh, acc[cb], 0, 0, 0);
      acc[cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pah, bl, acc[cb], 0, 0, 0);
      acc[cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pah, bh, acc[cb], 0, 0, 0);
    }
    WAVE_PHASE(17);
    if (nxt < ntiles) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this tile's fragment reads have returned: the stage may be overwritten
#pragma unroll
      for (int i = 0; i < 16; ++i) *reinterpret_cast<du32x4*>(stage + i * 1024 + lane * 16) = pf[i];
    }
    WAVE_PHASE(18);
  }
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
}

// ---- what surrounds the key loop: the absorbed queries on their way in, the waves' partial results on their way out ----
// absorbed query q'[h][c4 .. c4 + 3] into the [8][256] fp32 image the fp32 MFMA form reads (16-byte chunks of row h XOR-ed with h)
__device__ __forceinline__ void store_absorbed_query(float* qp, int h, int c4, const float4& qv) {
  *reinterpret_cast<float4*>(qp + h * 256 + (((c4 >> 2) ^ h) << 2)) = qv;
}
// split16 of x = a * s.  The lo plane's x - hi is spelled out, not left to the compiler's contraction: FUSED_LO takes it as
// fma(a, s, -hi), from the unrounded product -- what contraction had made of the one-row kernel's copy of this code and not of
// the two-row body's.  The two kernels' results are pinned separately (they promise each other fp32 rounding only), so each
// keeps its form.
template <bool FUSED_LO>
__device__ __forceinline__ void split16_scaled(float a, float s, unsigned& hi, unsigned& lo) {
#pragma clang fp contract(off)
  const float x = a * s;
  const unsigned u = __float_as_uint(x);
  hi = u >> 16;
  const float h = __uint_as_float(u & 0xFFFF0000u);
  const __bf16 l = (__bf16)(FUSED_LO ? fmaf(a, s, -h) : x - h);
  lo = *reinterpret_cast<const unsigned short*>(&l);
}
// ... and q' = a * scale as hi / lo bf16 planes (cross_absorbed_wave_bx3): head h's row of 512 B, chunk (c4 >> 3) ^ h, half
// (c4 >> 2) & 1
template <bool FUSED_LO>
__device__ __forceinline__ void store_absorbed_query_bx3(float* qp, int h, int c4, const float4& a, float scale) {
  const float v[4] = {a.x, a.y, a.z, a.w};
  unsigned hi[4], lo[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) split16_scaled<FUSED_LO>(v[e], scale, hi[e], lo[e]);
  unsigned char* base = reinterpret_cast<unsigned char*>(qp) + h * 512 + (((c4 >> 3) ^ h) << 4) + ((c4 >> 2) & 1) * 8;
  *reinterpret_cast<uint2*>(base) = make_uint2(hi[0] | hi[1] << 16, hi[2] | hi[3] << 16);
  *reinterpret_cast<uint2*>(base + 4096) = make_uint2(lo[0] | lo[1] << 16, lo[2] | lo[3] << 16);
}
// a wave's running max / sum per head for the merge: the lanes that hold one (`holds`: g == 0 and col < 8, head = col) write
// element `slot` = 8 * wave + head of wm / wl [waves][8]; behind it the wave's LDS traffic has drained (its stage is idle)
__device__ __forceinline__ void store_wave_ml(float* wm, float* wl, int slot, bool holds, float m_run, float l_run) {
  if (holds) { wm[slot] = m_run; wl[slot] = l_run; }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// this wave's un-normalised ctx [8 heads][256] into its (now idle) staging area: lane (g, col) holds heads 4 g + reg.
// fp32 form: acc[w][e][reg] = ctx[head 4 g + reg][channel 64 w + 4 col + e]
__device__ __forceinline__ void store_wave_ctx(const f32x4 (&acc)[4][4], float* mine, int g, int col) {
  if (g < 2) {
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        *reinterpret_cast<float4*>(mine + (4 * g + reg) * 256 + 64 * w + 4 * col) =
            make_float4(acc[w][0][reg], acc[w][1][reg], acc[w][2][reg], acc[w][3][reg]);
  }
}
// split-bf16 form: acc[cb][reg] = ctx[head 4 g + reg][channel 16 cb + col]
__device__ __forceinline__ void store_wave_ctx(const f32x4 (&acc)[16], float* mine, int g, int col) {
  if (g < 2) {
#pragma unroll
    for (int cb = 0; cb < 16; ++cb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) mine[(4 * g + reg) * 256 + 16 * cb + col] = acc[cb][reg];
  }
}
// log-sum-exp combine of the NW waves' partial softmaxes of one query row: channels c4 .. c4 + 3 of head h.  wm / wl: [NW][8];
// stage_base: the first of the NW stages that hold the waves' ctx; the normalised context goes to ctx_out [8][256]
template <int NW>
__device__ __forceinline__ void merge_wave_softmax(const float (*wm)[8], const float (*wl)[8], const unsigned char* stage_base,
                                                   float* ctx_out, int h, int c4) {
  float M = -INFINITY;
#pragma unroll
  for (int w = 0; w < NW; ++w) M = fmaxf(M, wm[w][h]);
  float L = 0.f;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const float f = wl[w][h] > 0.f ? expf(wm[w][h] - M) : 0.f;  // waves without keys contribute nothing
    L += wl[w][h] * f;
    const float4 c = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(stage_base + w * 16384) + h * 256 + c4);
    o.x += c.x * f; o.y += c.y * f; o.z += c.z * f; o.w += c.w * f;
  }
  *reinterpret_cast<float4*>(ctx_out + h * 256 + c4) = scale4(o, 1.f / L);
}

struct DecRow2P {
  DecRowP r;            // as decoder_row_kernel (ck / cv unused)
  const float* mem;     // [samples][T][D] encoder memory (engine-owned copy)
  long long mem_stride; // floats per sample
  const float* wk;      // [D][D] cross-attention key projection as stored (rows = output feature h*hd + e)
  const float* wv_t;    // [D (c)][D (o)] value projection, transposed
  const float* bv;      // [D]
  // beam search (MODE 1 / 2): the row kernel split around the per-SAMPLE cross-attention kernel
  float* qp;            // [rows][8][D]: MODE 1 writes the absorbed queries, beam_cross_kernel replaces them with the context rows
  float* x1;            // [rows][D]: LN1 output (the residual of the cross-attention block), MODE 1 -> MODE 2
  // round 4: the memory rows as two bf16 planes (launch_split_bf16: hi = bf16_rne(x), lo = bf16_rne(x - hi)) for the greedy
  // two-row kernel's split-bf16 cross-attention (nullptr: the fp32 rows above on the fp32 MFMA)
  const uint16_t* mem_hi;   // [samples][T][D]
  const uint16_t* mem_lo;   // [samples][T][D]
  // ragged decode group (the RAGGED builds of the greedy kernels): `mem` / `mem_hi` / `mem_lo` are ONE packed [sum B_i T_i][D]
  // buffer, row b attends over the len[b] memory rows that start at row row0[b] (device tables; r.T, mem_stride, c_row_map unused).
  // Ragged beam search (RAGGED == 2 of the one-row kernel): the tables are indexed by SAMPLE, row b reads entry r.c_row_map[b]
  const int* row0;
  const int* len;
};

// MODE 0: the whole row step (greedy).  MODE 1: up to the absorbed queries, which go to q.qp (+ x1 to q.x1).  MODE 2: from
// the context rows in q.qp on (value projection, output projection, residual) -- the two halves around beam_cross_kernel.
constexpr int ANC_MAX = 512;  // longest ancestry row held in LDS (DecRowP::anc needs s_Lmax <= ANC_MAX)
// D = 256, 8 heads of 32; BX3 (MODE 0): the cross-attention on split-bf16 MFMAs; RAGGED (MODE 0): memory base and length from the
// device tables -- 1: indexed by ROW (greedy decode groups), 2: indexed by the row's SAMPLE c_row_map[b] (beam search over crops of
// different sizes: rows move as hypotheses complete and compact, the row map follows them, the tables stay put)
template <int NTH, int MODE, bool BX3 = false, int RAGGED = 0>
__global__ __launch_bounds__(NTH, 2) void decoder_row_absorbed_kernel(const DecRow2P q) {
  constexpr int D = 256, HD = 32, NW = NTH / 64, G = NTH / (D / 4), HPW = 8 / NW;
  const DecRowP& p = q.r;
  ROW_KERNEL_ENTRY(p, p.rows_ptr && (int)blockIdx.x >= *p.rows_ptr);  // (device-side beam search: a dead row slot)
  // 77 KB: two blocks per CU.  The GEMV partial sums live in the (then idle) tile staging area, the merged context rows
  // in the absorbed queries' place (the queries are in registers by then).
  __shared__ __attribute__((aligned(1024))) unsigned char stage_s[NW * 16384];
  __shared__ __attribute__((aligned(1024))) float qp_s[8 * D];
  __shared__ __attribute__((aligned(16))) float a_s[D], y_s[D], x1_s[D], q2_s[D];
  __shared__ float wm_s[NW][8], wl_s[NW][8];
  float* const part_s = reinterpret_cast<float*>(stage_s);
  float* const ctx_s = qp_s;
  static_assert(G * D * 4 <= 16384, "GEMV partial sums must fit into one wave's staging area");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int t = *p.step_ptr;
  if (MODE != 2) {
  // beam search: the hypothesis' earlier positions stay in the cache rows they were written to (no cache copy per step)
  __shared__ int anc_s[ANC_MAX];
  if (p.anc) {
    for (int j = tid; j < t; j += NTH) anc_s[j] = p.anc[(size_t)b * p.anc_stride + j];
    __syncthreads();
  }
  // ---- self-attention over the cache (as decoder_row_kernel) ----
#pragma unroll
  for (int hp = 0; hp < (ROW_PROBE(1) ? 0 : HPW); ++hp) {
    const int head = wave + hp * NW;
    row_self_attention<D, HD, true>(p, b, head, t, lane, a_s + head * HD, anc_s);
  }
  __syncthreads();
  if (!ROW_PROBE(2)) row_gemv<D, NTH>(a_s, p.wo_t, part_s, tid);
  __syncthreads();
  if (tid < D) y_s[tid] = sum_parts<G, D>(part_s, tid, p.bo[tid] + p.xres[(size_t)b * D + tid]);
  __syncthreads();
  if (wave == 0) row_ln1<D>(y_s, x1_s, lane, p);
  __syncthreads();
  if (!ROW_PROBE(2)) row_gemv<D, NTH>(x1_s, p.wq_t, part_s, tid);
  __syncthreads();
  if (tid < D) q2_s[tid] = sum_parts<G, D>(part_s, tid, p.bq[tid]);
  __syncthreads();
  // ---- absorbed queries: q'[h][c] = scale * sum_e q2[h*32 + e] * W_k[h*32 + e][c] ----
  if (!ROW_PROBE(2)) {
    const float scale = 0.17677669529663687f;  // 1 / sqrt(32)
    for (int idx = tid; idx < 8 * (D / 4); idx += NTH) {
      const int h = idx / (D / 4), c4 = (idx % (D / 4)) * 4;
      const float* w = q.wk + (size_t)(h * HD) * D + c4;
      float4 accq = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
      for (int e = 0; e < HD; ++e) fma4(q2_s[h * HD + e], *reinterpret_cast<const float4*>(w + (size_t)e * D), accq);
      const float4 qv = scale4(accq, scale);
      if (MODE == 1) *reinterpret_cast<float4*>(q.qp + ((size_t)b * 8 + h) * D + c4) = qv;
      else if (BX3) store_absorbed_query_bx3<true>(qp_s, h, c4, accq, scale);
      else store_absorbed_query(qp_s, h, c4, qv);
    }
  }
  __syncthreads();
  }
  if (MODE == 1) {
    if (tid < D) q.x1[(size_t)b * D + tid] = x1_s[tid];
    return;
  }
  if (MODE == 2) {  // the context rows of this hypothesis and its LN1 output come back from global memory
    for (int idx = tid; idx < 8 * (D / 4); idx += NTH)
      *reinterpret_cast<float4*>(ctx_s + idx * 4) = *reinterpret_cast<const float4*>(q.qp + (size_t)b * 8 * D + idx * 4);
    if (tid < D) x1_s[tid] = q.x1[(size_t)b * D + tid];
    __syncthreads();
  }
  // ---- cross-attention over the memory rows of this row's sample ----
  if (MODE == 0 && !ROW_PROBE(4)) {
    // the keys of this row: a sample of the uniform [samples][T][D] memory, or (RAGGED) its own slice of the packed rows.  A wave
    // that owns no tile of a short row skips the key loop (no block barrier inside) and hands (-inf, 0) to the merge below
    int Tb;
    size_t moff;
    if constexpr (RAGGED == 1) {
      Tb = q.len[b];
      moff = (size_t)q.row0[b] * D;
    } else if constexpr (RAGGED == 2) {  // (the launcher guarantees a row map)
      const int cb = p.c_row_map[b];
      Tb = q.len[cb];
      moff = (size_t)q.row0[cb] * D;
    } else {
      const int cb = p.c_row_map ? p.c_row_map[b] : b;
      Tb = p.T;
      moff = (size_t)cb * q.mem_stride;
    }
    float m_run, l_run;
    unsigned char* stage = stage_s + wave * 16384;
    const int col = lane & 15, g = lane >> 4;
    float* mine = reinterpret_cast<float*>(stage);
    if constexpr (BX3) {
      const uint16_t* mh = q.mem_hi + moff;
      const uint16_t* ml = q.mem_lo + moff;
      f32x4 acc[16];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (wave < ((Tb + 15) >> 4)) bx3_tile_dma(mh, ml, Tb, wave, stage, lane);  // (the stage held GEMV partials until now)
      cross_absorbed_wave_bx3<NW>(mh, ml, Tb, reinterpret_cast<const unsigned char*>(qp_s), stage, wave, lane, m_run, l_run, acc);
      store_wave_ml(&wm_s[0][0], &wl_s[0][0], wave * 8 + col, g == 0 && col < 8, m_run, l_run);
      store_wave_ctx(acc, mine, g, col);
    } else {
      f32x4 acc[4][4];
      cross_absorbed_wave<NW, false>(q.mem + moff, Tb, qp_s, stage, wave, lane, m_run, l_run, acc);
      store_wave_ml(&wm_s[0][0], &wl_s[0][0], wave * 8 + col, g == 0 && col < 8, m_run, l_run);
      store_wave_ctx(acc, mine, g, col);
    }
  }
  __syncthreads();
  for (int idx = tid; idx < (MODE != 0 || ROW_PROBE(4) ? 0 : 8 * (D / 4)); idx += NTH)  // merge the waves' partial softmaxes
    merge_wave_softmax<NW>(wm_s, wl_s, stage_s, ctx_s, idx / (D / 4), (idx % (D / 4)) * 4);
  __syncthreads();
  // ---- a2[o] = b_v[o] + sum_c ctx[head(o)][c] * W_v^T[c][o] ----
  if (!ROW_PROBE(2)) row_gemv<D, NTH, HD>(ctx_s, q.wv_t, part_s, tid);
  __syncthreads();
  if (tid < D) a_s[tid] = sum_parts<G, D>(part_s, tid, q.bv[tid]);
  __syncthreads();
  if (!ROW_PROBE(2)) row_gemv<D, NTH>(a_s, p.wco_t, part_s, tid);
  __syncthreads();
  if (tid < D) p.y2[(size_t)b * D + tid] = sum_parts<G, D>(part_s, tid, p.bco[tid] + x1_s[tid]);
}

// ---------------------------------------------------------------------------------------------------------------------
// The row step for TWO rows per block (greedy decode; the shipped form).
//
// Two rows per block: the five row GEMVs read 5 x 256 KB of weights per row through the CU's 64 B/clk L2 path; the block's 512
// threads fetch every weight element ONCE and apply it to both rows' inputs (two accumulators, eight K groups of 32), the
// absorbed-query product shares W_k the same way, and the attention phases run per row: waves 0-3 on row 2b, waves 4-7 on row
// 2b + 1, each wave its own key tiles and 16 KB stage.  Per row the arithmetic and its order are those of
// decoder_row_absorbed_kernel (K groups of 32 instead of 64 change the association: equal to fp32 rounding).  An odd row
// count: the last block's second half repeats the last row and keeps its stores to itself -- the same kernel for EVERY row, so
// a row's result never depends on how many rows share the launch.  156 KB of LDS: one block per CU.
//
// Issue order.  Run as a serial chain of phases that each begin with an exposed round trip, the step keeps the matrix pipes
// 12 % busy with SQ_WAIT_ANY at 49 % of the wave cycles (PMC at 384 rows, profiles/r04_pmc_decode.txt).  So
//   * a wave's FIRST memory tile is on its way (LDS-DMA) from the kernel's first instruction -- the staging area is idle until
//     the cross-attention (the GEMV partials of the first two projections live in the absorbed queries' LDS instead);
//   * inside the cross-attention the NEXT tile travels to registers (16 x 16 bytes per lane) while the matrix cores work on the
//     current one, and moves to LDS when its reads are done: a tile costs max(arithmetic, round trip), not their sum;
//   * a GEMV's weight rows (32 x 16 bytes per thread) are requested one phase early: W_o before the self-attention, W_q behind
//     the W_o products, W_k behind the W_q products, W_v behind the cross-attention loop, W_co behind the W_v products; the
//     element-wise phases' few global operands even earlier (the vector-memory counter retires in order);
//   * the self-attention runs a wave's two heads in ONE loop (twice the K / V groups in flight per round trip);
//   * block barriers are raw s_barrier behind lgkmcnt(0) (LDS only): a __syncthreads() fence would drain the prefetches.
// Phase timeline at 384 rows, alone on the chip (probe build, tools/probe/row_phases.py; us per launch), with the cross-attention
// on split-bf16 MFMAs (cross_absorbed_wave_bx3): entry .. self-attention 21.9, five GEMVs 10.6, cross-attention 18.9, element-wise
// 3.9 -- 55.3 in all (the serial chain of phases, same arithmetic: 64.4; this issue order on the fp32 MFMA: 62.7).
// ---------------------------------------------------------------------------------------------------------------------
#define ROW_SYNC() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)

// weight rows of one two-row GEMV: thread (lr = tid % 64, g = tid / 64) holds Wt[32 g + k][4 lr .. 4 lr + 3], k = 0 .. 31
__device__ __forceinline__ void gemv2_load(const float* __restrict__ Wt, int g, int lr, float4 (&w)[32]) {
  const float* src = Wt + (size_t)(g * 32) * 256 + lr * 4;
#pragma unroll
  for (int k = 0; k < 32; ++k) w[k] = *reinterpret_cast<const float4*>(src + (size_t)k * 256);
}
// gemv2<256, 512>'s products in its order on rows loaded earlier; in0 / in1 = the two rows' inputs at k = 32 g
__device__ __forceinline__ void gemv2_fma(const float4 (&w)[32], const float* in0, const float* in1, float4& a0, float4& a1) {
  a0 = make_float4(0.f, 0.f, 0.f, 0.f);
  a1 = a0;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const float4 w4 = w[k];
    const float x0 = in0[k], x1 = in1[k];
    fma4(x0, w4, a0);
    fma4(x1, w4, a1);
  }
}
// the two rows' partial sums of thread (lr, g) into part[row][g][n]
__device__ __forceinline__ void gemv2_store(float* part, int g, int lr, const float4& a0, const float4& a1) {
  *reinterpret_cast<float4*>(part + (0 * 8 + g) * 256 + lr * 4) = a0;
  *reinterpret_cast<float4*>(part + (1 * 8 + g) * 256 + lr * 4) = a1;
}

// row_attention<32, U> for TWO heads of one row in one loop (per head the same keys per lane in the same order)
struct NoHook { __device__ __forceinline__ void operator()() const {} };
// `after_first_issue` runs once, right behind the first iteration's K / V loads: the caller's own prefetches (first memory tile,
// first GEMV's weight rows) then queue BEHIND those loads instead of in front of them, and their issue time is covered by the
// first round trip (the vector-memory counter retires in order: what is issued first is awaited first)
template <int U, int HD = 32, class Hook = NoHook>
__device__ __forceinline__ void row_attention_2h(const float* const (&q)[2], const float* const (&Kc)[2], const float* const (&Vc)[2],
                                                 const float* const (&curk)[2], const float* const (&curv)[2], int t, int L,
                                                 float* const (&out)[2], int lane, Hook after_first_issue = Hook()) {
  constexpr int LPK = HD / 4, KPI = 64 / LPK;
  const int kig = lane / LPK, ch = lane % LPK;
  float4 q4[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) q4[h] = *reinterpret_cast<const float4*>(q[h] + ch * 4);
  const float scale = HD == 32 ? 0.17677669529663687f : 0.125f;
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  const int nit = (L + KPI - 1) / KPI;
  float4 k4[2][U], v4[2][U];
  auto issue = [&](int it0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = (it0 + u) * KPI + kig;
      const int jj = j < L ? j : 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float* kr = (curk[h] && jj == t) ? curk[h] : Kc[h] + (size_t)jj * HD;
        const float* vr = (curv[h] && jj == t) ? curv[h] : Vc[h] + (size_t)jj * HD;
        k4[h][u] = *reinterpret_cast<const float4*>(kr + ch * 4);
        v4[h][u] = *reinterpret_cast<const float4*>(vr + ch * 4);
      }
    }
  };
  WAVE_PHASE_INIT();
  issue(0);
  __builtin_amdgcn_sched_barrier(0);
  WAVE_PHASE(21);  // first K / V groups issued
  after_first_issue();
  __builtin_amdgcn_sched_barrier(0);
  WAVE_PHASE(22);  // the caller's prefetches issued
  for (int it0 = 0; it0 < nit; it0 += U) {
    if (it0 > 0) issue(it0);
    WAVE_PHASE(23);  // (further groups issued)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = (it0 + u) * KPI + kig;
        float d = HD == 64 ? att_dot4(q4[h], k4[h][u])
                           : (q4[h].x * k4[h][u].x + q4[h].y * k4[h][u].y) + (q4[h].z * k4[h][u].z + q4[h].w * k4[h][u].w);
#pragma unroll
        for (int o = 1; o < LPK; o <<= 1) d += __shfl_xor(d, o, 64);
        if (j < L) {
          if constexpr (HD == 64) {
            att_update(d * scale, v4[h][u], m[h], l[h], acc[h]);
          } else {
            const float sj = d * scale;
            const float mn = fmaxf(m[h], sj);
            const float f = expf(m[h] - mn);
            const float pj = expf(sj - mn);
            l[h] = l[h] * f + pj;
            acc[h].x = acc[h].x * f + pj * v4[h][u].x; acc[h].y = acc[h].y * f + pj * v4[h][u].y;
            acc[h].z = acc[h].z * f + pj * v4[h][u].z; acc[h].w = acc[h].w * f + pj * v4[h][u].w;
            m[h] = mn;
          }
        }
      }
    WAVE_PHASE(24);  // groups awaited + scored
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int o = LPK; o < 64; o <<= 1) {
      if constexpr (HD == 64) {
        att_merge(o, m[h], l[h], acc[h]);
      } else {
        const float mo = __shfl_xor(m[h], o, 64), lo = __shfl_xor(l[h], o, 64);
        const float ax = __shfl_xor(acc[h].x, o, 64), ay = __shfl_xor(acc[h].y, o, 64);
        const float az = __shfl_xor(acc[h].z, o, 64), aw = __shfl_xor(acc[h].w, o, 64);
        const float mn = fmaxf(m[h], mo);
        const float f1 = l[h] > 0.f ? expf(m[h] - mn) : 0.f, f2 = lo > 0.f ? expf(mo - mn) : 0.f;
        l[h] = l[h] * f1 + lo * f2;
        acc[h].x = acc[h].x * f1 + ax * f2; acc[h].y = acc[h].y * f1 + ay * f2;
        acc[h].z = acc[h].z * f1 + az * f2; acc[h].w = acc[h].w * f1 + aw * f2;
        m[h] = mn;
      }
    }
    if (kig == 0) {
      const float inv = 1.f / l[h];
      *reinterpret_cast<float4*>(out[h] + ch * 4) = make_float4(acc[h].x * inv, acc[h].y * inv, acc[h].z * inv, acc[h].w * inv);
    }
  }
}

// RAGGED (decode groups of batches with different row counts and memory lengths): row b reads its keys from the packed memory
// rows [row0[b], row0[b] + len[b]); the two halves of a block get independent lengths.  Every block barrier (ROW_SYNC) and every
// s_waitcnt of the body lies OUTSIDE the key loop and is reached by all eight waves whatever the two lengths are: the first-tile
// LDS-DMA is a wave-uniform `if` without a barrier, the key loop is private to a wave, and a wave that owns no tile hands
// (-inf, 0) and zero accumulators to the merge.  A row's arithmetic depends on its own length alone (tile -> wave assignment),
// so it is bit-identical to the uniform kernel's on the same memory.  A template parameter, not a branch: the uniform builds
// compile to the code they were.
template <bool BX3, bool RAGGED = false>  // BX3: the cross-attention on split-bf16 MFMAs over DecRow2P::mem_hi / mem_lo (cross_absorbed_wave_bx3)
__device__ __forceinline__ void decoder_row2_absorbed_pf_body(const DecRow2P& q) {
  constexpr int D = 256, HD = 32, G = 8;
  const DecRowP& p = q.r;
  ROW_KERNEL_ENTRY(p, false);
  ROW_PHASE_INIT();
  __shared__ __attribute__((aligned(1024))) unsigned char stage_s[8 * 16384];
  __shared__ __attribute__((aligned(1024))) float qp_s[2][8 * D];
  __shared__ __attribute__((aligned(16))) float a_s[2][D], y_s[2][D], x1_s[2][D], q2_s[2][D];
  __shared__ float wm_s[2][4][8], wl_s[2][4][8];
  float* const part_late = reinterpret_cast<float*>(stage_s);   // [2][G][D]: the GEMVs behind the cross-attention (stages idle again)
  float* const part_early = &qp_s[0][0];                        // [2][G][D]: the GEMVs in front of it (the first tiles are landing in the stages)
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;  // (wave-uniform values in SGPRs)
  const int half = wave >> 2, w4i = wave & 3;
  const bool valid = 2 * (int)blockIdx.x + half < p.M;
  const int b = valid ? 2 * blockIdx.x + half : p.M - 1;
  const int trow = wave >> 2, tcol = tid & 255;
  const bool tvalid = valid;
  const int brow = b;
  const int t = *p.step_ptr;
  const int lr = lane, gg = wave;  // GEMV thread coordinates: columns 4 lr .. 4 lr + 3, K group gg
  // ---- this wave's first memory tile, and the first GEMV's weight rows, are requested before anything else ----
  int Tb;        // keys of this wave's row (wave-uniform: b is)
  size_t moff;   // its first memory row, in elements
  if constexpr (RAGGED) {
    Tb = q.len[b];
    moff = (size_t)q.row0[b] * D;
  } else {
    const int cb = p.c_row_map ? p.c_row_map[b] : b;
    Tb = p.T;
    moff = (size_t)cb * q.mem_stride;
  }
  const float* const mem = q.mem + moff;
  unsigned char* const stage = stage_s + wave * 16384;
  const uint16_t* const mh = BX3 ? q.mem_hi + moff : nullptr;
  const uint16_t* const ml = BX3 ? q.mem_lo + moff : nullptr;
  // the element-wise phases' few global operands, requested BEFORE the weight prefetches: the vector-memory counter retires in
  // order, so a small load issued behind a 256 KB prefetch would wait for all of it
  const float bo_v = p.bo[tcol] + p.xres[(size_t)brow * D + tcol], bq_v = p.bq[tcol], bv_v = q.bv[tcol], bco_v = p.bco[tcol];
  float ln_g[4], ln_b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { ln_g[i] = p.ln1_g[i * 64 + lane]; ln_b[i] = p.ln1_b[i * 64 + lane]; }
  float4 W[32];
  // this wave's first memory tile (LDS-DMA) and the first GEMV's weight rows: issued from inside the self-attention, right
  // behind its first K / V loads (their 48 instructions' issue time -- ~100 ns each with the CU's vector-memory path busy --
  // then passes under that first round trip instead of in front of it)
  auto prefetch = [&]() {
    if (w4i < ((Tb + 15) >> 4)) {
      if constexpr (BX3) bx3_tile_dma(mh, ml, Tb, w4i, stage, lane);
      else cross_tile_dma(mem, Tb, w4i, stage, lane);
    }
    gemv2_load(p.wo_t, gg, lr, W);
  };
  ROW_PHASE(19);  // kernel entry: scalar state, small operands
  // ---- self-attention over the cache, this wave's two heads in one loop ----
  {
    // (cache_append_and_heads spelled out: through the helper the split-bf16 builds' scratch changes, 36 -> 24 bytes per lane)
    const float* qkv = p.qkv + (size_t)b * p.qkv_stride;
    const float *qh[2], *Kh[2], *Vh[2], *ck[2], *cv[2];
    float* oh[2];
#pragma unroll
    for (int hp = 0; hp < 2; ++hp) {
      const int head = w4i + hp * 4;
      float* Kc = p.sk + (size_t)b * p.s_batch_stride + (size_t)head * p.s_Lmax * HD;
      float* Vc = p.sv + (size_t)b * p.s_batch_stride + (size_t)head * p.s_Lmax * HD;
      ck[hp] = qkv + D + head * HD;
      cv[hp] = qkv + 2 * D + head * HD;
      if (lane < HD && valid) {
        Kc[(size_t)t * HD + lane] = ck[hp][lane];
        Vc[(size_t)t * HD + lane] = cv[hp][lane];
      }
      qh[hp] = qkv + head * HD; Kh[hp] = Kc; Vh[hp] = Vc; oh[hp] = a_s[half] + head * HD;
    }
    row_attention_2h<4, 32>(qh, Kh, Vh, ck, cv, t, t + 1, oh, lane, prefetch);
  }
  ROW_SYNC();
  ROW_PHASE(0);
  {
    float4 a0, a1;
    gemv2_fma(W, a_s[0] + gg * 32, a_s[1] + gg * 32, a0, a1);
    gemv2_load(p.wq_t, gg, lr, W);  // next projection's rows: on their way during the reduction and LN1
    gemv2_store(part_early, gg, lr, a0, a1);
  }
  ROW_SYNC();
  ROW_PHASE(1);
  y_s[trow][tcol] = sum_parts<G, D>(part_early + trow * G * D, tcol, bo_v);
  ROW_SYNC();
  ROW_PHASE(2);
  if (w4i == 0)  // one wave per row
    row_ln1<D>(y_s[half], x1_s[half], lane, p.eps, [&](int i, int) { return ln_g[i]; }, [&](int i, int) { return ln_b[i]; });
  ROW_SYNC();
  ROW_PHASE(3);
  {
    float4 a0, a1;
    gemv2_fma(W, x1_s[0] + gg * 32, x1_s[1] + gg * 32, a0, a1);
    gemv2_load(q.wk, gg, lr, W);  // W_k rows of head gg (= tid / 64), columns 4 lr ..: the absorbed-query product's operand
    gemv2_store(part_early, gg, lr, a0, a1);
  }
  ROW_SYNC();
  ROW_PHASE(4);
  q2_s[trow][tcol] = sum_parts<G, D>(part_early + trow * G * D, tcol, bq_v);
  ROW_SYNC();
  ROW_PHASE(5);
  // ---- absorbed queries of both rows: q'[h][c] = scale * sum_e q2[h*32 + e] * W_k[h*32 + e][c]; thread -> (head gg, 4 channels) ----
  {
    const float scale = 0.17677669529663687f;  // 1 / sqrt(32)
    float4 a0, a1;
    gemv2_fma(W, q2_s[0] + gg * HD, q2_s[1] + gg * HD, a0, a1);
    if constexpr (BX3) {
      store_absorbed_query_bx3<false>(qp_s[0], gg, lr * 4, a0, scale);
      store_absorbed_query_bx3<false>(qp_s[1], gg, lr * 4, a1, scale);
    } else {
      store_absorbed_query(qp_s[0], gg, lr * 4, scale4(a0, scale));
      store_absorbed_query(qp_s[1], gg, lr * 4, scale4(a1, scale));
    }
  }
  ROW_SYNC();
  ROW_PHASE(6);
  // ---- cross-attention over the memory rows of each row's sample: four waves per row ----
  {
    float m_run, l_run;
    const int col = lane & 15, g = lane >> 4;
    float* mine = reinterpret_cast<float*>(stage);
    if constexpr (BX3) {
      f32x4 acc[16];
      cross_absorbed_wave_bx3<4>(mh, ml, Tb, reinterpret_cast<const unsigned char*>(qp_s[half]), stage, w4i, lane, m_run, l_run, acc);
      ROW_PHASE(12);
      store_wave_ml(&wm_s[half][0][0], &wl_s[half][0][0], w4i * 8 + col, g == 0 && col < 8, m_run, l_run);
      store_wave_ctx(acc, mine, g, col);
    } else {
      f32x4 acc[4][4];
      cross_absorbed_wave<4, true>(mem, Tb, qp_s[half], stage, w4i, lane, m_run, l_run, acc);
      ROW_PHASE(12);
      store_wave_ml(&wm_s[half][0][0], &wl_s[half][0][0], w4i * 8 + col, g == 0 && col < 8, m_run, l_run);
      store_wave_ctx(acc, mine, g, col);
    }
  }
  gemv2_load(q.wv_t, gg, lr, W);  // value projection's rows: on their way during the merge
  ROW_SYNC();
  ROW_PHASE(7);
  for (int idx = tid; idx < 2 * 8 * (D / 4); idx += 512) {  // merge each row's four partial softmaxes; ctx in the queries' place
    const int row = idx / (8 * (D / 4)), rem = idx % (8 * (D / 4));
    merge_wave_softmax<4>(wm_s[row], wl_s[row], stage_s + row * 4 * 16384, qp_s[row], rem / (D / 4), (rem % (D / 4)) * 4);
  }
  ROW_SYNC();
  ROW_PHASE(8);
  // ---- a2[o] = b_v[o] + sum_c ctx[head(o)][c] * W_v^T[c][o], both rows ----
  {
    const int hoff = ((lr * 4) / HD) * D + gg * 32;
    float4 a0, a1;
    gemv2_fma(W, qp_s[0] + hoff, qp_s[1] + hoff, a0, a1);
    gemv2_load(p.wco_t, gg, lr, W);
    gemv2_store(part_late, gg, lr, a0, a1);
  }
  ROW_SYNC();
  ROW_PHASE(9);
  a_s[trow][tcol] = sum_parts<G, D>(part_late + trow * G * D, tcol, bv_v);
  ROW_SYNC();
  ROW_PHASE(10);
  {
    float4 a0, a1;
    gemv2_fma(W, a_s[0] + gg * 32, a_s[1] + gg * 32, a0, a1);
    ROW_SYNC();  // (every thread has read part_late's previous contents)
    gemv2_store(part_late, gg, lr, a0, a1);
  }
  ROW_SYNC();
  ROW_PHASE(11);
  {
    const float v = sum_parts<G, D>(part_late + trow * G * D, tcol, bco_v + x1_s[trow][tcol]);
    if (tvalid) p.y2[(size_t)brow * D + tcol] = v;
  }
  ROW_PHASE(20);
}

__global__ __launch_bounds__(512, 1) void decoder_row2_absorbed_pf_kernel(const DecRow2P q) { decoder_row2_absorbed_pf_body<false>(q); }
__global__ __launch_bounds__(512, 1) void decoder_row2_absorbed_bx3_kernel(const DecRow2P q) { decoder_row2_absorbed_pf_body<true>(q); }
__global__ __launch_bounds__(512, 1) void decoder_row2_absorbed_pf_ragged_kernel(const DecRow2P q) { decoder_row2_absorbed_pf_body<false, true>(q); }
__global__ __launch_bounds__(512, 1) void decoder_row2_absorbed_bx3_ragged_kernel(const DecRow2P q) { decoder_row2_absorbed_pf_body<true, true>(q); }

#ifdef D2T_PROBES
}  // namespace d2t
extern "C" int d2t_debug_row_phases(unsigned long long* out, int reset) {  // probe builds: read (and clear) d2t_row_phase
  hipDeviceSynchronize();
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(d2t::d2t_row_phase), 32 * 8) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[32] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(d2t::d2t_row_phase), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
namespace d2t {
#endif
hipError_t launch_decoder_row_absorbed(const DecRowP& r, const float* mem, long long mem_stride, const float* wk, const float* wv_t,
                                       const float* bv, hipStream_t s, const uint16_t* mem_hi, const uint16_t* mem_lo,
                                       const int* row0, const int* len) {
  // ---- what is refused ----
  const bool ragged = row0 != nullptr;
  if (r.heads != 8 || r.D != 256 || (!ragged && r.T < 1)) return hipErrorInvalidValue;
  const bool by_sample = ragged && r.c_row_map;  // beam rows: tables per sample, reached through the row map
  if (ragged && !len) return hipErrorInvalidValue;
  if (ragged && !by_sample && (r.anc || r.rows_ptr)) return hipErrorInvalidValue;  // tables per row: greedy rows only
  if (by_sample && !r.one_row) return hipErrorInvalidValue;  // the two-row builds know neither row map nor ancestry
  if (r.anc && (!r.one_row || r.s_Lmax > ANC_MAX)) return hipErrorInvalidValue;  // the two-row kernel reads the cache directly
  DecRow2P q{r, mem, mem_stride, wk, wv_t, bv, nullptr, nullptr, mem_hi, mem_lo, row0, len};
  static const int probe = D2T_PROBE_ENV("D2T_ROW_PROBE");  // probe builds only: skip phases (results are garbage by construction)
  q.r.probe = probe;
  // ---- which kernel: [cross-attention on split-bf16 MFMAs][memory tables: none, per row, per sample] ----
  using Kernel = void (*)(const DecRow2P);
  static const Kernel one_row_kernels[2][3] = {
      {decoder_row_absorbed_kernel<256, 0, false, 0>, decoder_row_absorbed_kernel<256, 0, false, 1>, decoder_row_absorbed_kernel<256, 0, false, 2>},
      {decoder_row_absorbed_kernel<256, 0, true, 0>, decoder_row_absorbed_kernel<256, 0, true, 1>, decoder_row_absorbed_kernel<256, 0, true, 2>}};
  static const Kernel two_row_kernels[2][2] = {{decoder_row2_absorbed_pf_kernel, decoder_row2_absorbed_pf_ragged_kernel},
                                               {decoder_row2_absorbed_bx3_kernel, decoder_row2_absorbed_bx3_ragged_kernel}};
  static const bool one_row = D2T_PROBE_ENV_STR("D2T_DECODE_ONE_ROW_BLOCKS") != nullptr;  // A/B: the one-row-per-block form for every row
  const int bx3 = mem_hi && mem_lo;
  if (r.one_row || (one_row && !ragged)) hipLaunchKernelGGL(one_row_kernels[bx3][by_sample ? 2 : ragged], dim3(r.M), dim3(256), 0, s, q);
  else hipLaunchKernelGGL(two_row_kernels[bx3][ragged], dim3((r.M + 1) / 2), dim3(512), 0, s, q);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Beam search: ONE block per SAMPLE runs the cross-attention of all its live hypotheses (north_star's "K/V resident in LDS
// per wavefront", in the absorbed form: the sample's memory rows are staged in LDS ONCE per layer and step and serve every
// hypothesis and head; the reference repeats the memory per hypothesis, tfm.py:163, and the per-row kernel re-read it per
// hypothesis).  M <= 6 hypotheses x 8 heads = up to 48 query rows = three 16-row MFMA tiles (83 % filled at beam 5 against
// 50 % for a single row).  The four waves work through the key tiles TOGETHER: a ring of four 16 KB tile buffers with the
// LDS-DMA three tiles ahead; per tile wave w multiplies channel quarter w of the tile with the same slice of every q' row
// (the A fragment is read once for all row tiles), the partial score tiles are summed through LDS, each wave runs the online
// softmax of all rows and accumulates channel quarter w of the weighted memory rows.  (For ONE row this cooperative form
// lost to independent waves -- two block barriers per tile; with three row tiles per barrier pair it is the better split,
// and it needs no merge.)  In: q.qp = absorbed queries [rows][8][256] (from decoder_row_absorbed_kernel MODE 1); out: the
// normalised context rows in their place.
struct BeamCrossP {
  const float* mem; long long mem_stride; int T;
  float* qp;            // [rows][8][256]
  const int* seg;       // [samples][3]: first row, live hypotheses, (unused) per sample; nullptr: one sample, rows [0, M)
  int M;                // seg == nullptr: live hypotheses
  const int* step_ptr; const int* stop_at;
};

__global__ __launch_bounds__(256, 1) void beam_cross_kernel(const BeamCrossP p) {
  if (p.stop_at && *p.stop_at && *p.step_ptr >= *p.stop_at) return;
  constexpr int NR = 3, D = 256;
  int off = 0, M = p.M;
  if (p.seg) { off = p.seg[blockIdx.x * 3]; M = p.seg[blockIdx.x * 3 + 1]; }
  if (M <= 0) return;  // block-uniform (a finished sample)
  decode_wave_priority();
  __shared__ __attribute__((aligned(1024))) unsigned char stage[4 * 16384];
  __shared__ __attribute__((aligned(1024))) float qp_s[NR * 16 * D];
  __shared__ __attribute__((aligned(16))) float part[4 * 16 * NR * 16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, g = lane >> 4;
  const int R = 8 * M, nrt = (R + 15) >> 4;
  const float* mem = p.mem + (size_t)blockIdx.x * p.mem_stride;
  float* qrows = p.qp + (size_t)off * 8 * D;
  for (int idx = tid; idx < nrt * 16 * (D / 4); idx += 256) {  // q' rows, 16-byte chunks of row r XOR-ed with r & 15; rows >= R zero
    const int row = idx / (D / 4), c4 = idx % (D / 4);
    const float4 v = row < R ? *reinterpret_cast<const float4*>(qrows + (size_t)row * D + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(qp_s + row * D + ((c4 ^ (row & 15)) << 2)) = v;
  }
  float m_run[NR], l_run[NR];
  f32x4 acc[NR][4];
#pragma unroll
  for (int rt = 0; rt < NR; ++rt) {
    m_run[rt] = -INFINITY;
    l_run[rt] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[rt][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int T = p.T, ntiles = (T + 15) >> 4;
  auto issue = [&](int tile) {  // this wave's four rows of the tile: row i -> buffer + i * 1024, physical chunk c holds logical c ^ i
    unsigned char* buf = stage + (tile & 3) * 16384;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = wave * 4 + k;
      const int j = (tile << 4) + i < T ? (tile << 4) + i : T - 1;  // rows past the end: a valid row, its probability is forced to zero
      __builtin_amdgcn_global_load_lds(mem + (size_t)j * D + ((lane ^ i) << 2), (lds_ptr_dec)(buf + i * 1024), 16, 0, 0);
    }
  };
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the q' loads above are done: from here on vmcnt counts tile pieces only
  issue(0);
  if (ntiles > 1) issue(1);
  if (ntiles > 2) issue(2);
  for (int tile = 0; tile < ntiles; ++tile) {
    const int j0 = tile << 4;
    const int ahead = ntiles - 1 - tile;  // block-uniform
    if (ahead >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // the tile has landed for everyone (and, at tile 0, the q' rows are in LDS); nobody reads tile - 1 any more
    if (tile + 3 < ntiles) issue(tile + 3);
    const unsigned char* buf = stage + (tile & 3) * 16384;
    // ---- partial S^T[key = 4g' + reg][row = 16 rt + col] over this wave's channel quarter ----
    f32x4 sacc[NR];
#pragma unroll
    for (int rt = 0; rt < NR; ++rt) sacc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
      const int u = wave * 4 + uu;
      const float4 a4 = *reinterpret_cast<const float4*>(buf + col * 1024 + (((4 * u + g) ^ col) << 4));
#pragma unroll
      for (int rt = 0; rt < NR; ++rt) {
        if (rt < nrt) {
          const float4 q4 = *reinterpret_cast<const float4*>(reinterpret_cast<const unsigned char*>(qp_s) + (rt * 16 + col) * 1024 +
                                                              (((4 * u + g) ^ col) << 4));
          sacc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, q4.x, sacc[rt], 0, 0, 0);
          sacc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, q4.y, sacc[rt], 0, 0, 0);
          sacc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, q4.z, sacc[rt], 0, 0, 0);
          sacc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, q4.w, sacc[rt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int rt = 0; rt < NR; ++rt)
      if (rt < nrt) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) part[(wave * 16 + 4 * g + reg) * (NR * 16) + rt * 16 + col] = sacc[rt][reg];
      }
    __syncthreads();
    // ---- online softmax of every row (all waves, identically): this lane holds keys j0 + 4g + reg of row 16 rt + col ----
    float pv[NR][4];
#pragma unroll
    for (int rt = 0; rt < NR; ++rt) {
      if (rt < nrt) {
        f32x4 sc;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int o = (4 * g + reg) * (NR * 16) + rt * 16 + col;
          sc[reg] = (part[o] + part[16 * NR * 16 + o]) + (part[2 * 16 * NR * 16 + o] + part[3 * 16 * NR * 16 + o]);
        }
        float ar[4];  // the accumulators hold ctx[row 16 rt + 4g + reg]: lane 4g + reg has that row's alpha
        online_softmax_tile(sc, j0, g, T, m_run[rt], l_run[rt], pv[rt], ar);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[rt][e][reg] *= ar[reg];
      } else {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) pv[rt][reg] = 0.f;
      }
    }
    // ---- ctx[row][64 wave + 4 col + e] += sum_keys P[row][key] m[key][chan]; k-step sk <-> keys 4g + sk ----
#pragma unroll
    for (int sk = 0; sk < 4; ++sk) {
      const int key = 4 * g + sk;
      const float4 b4 = *reinterpret_cast<const float4*>(buf + key * 1024 + (((16 * wave + col) ^ key) << 4));
#pragma unroll
      for (int rt = 0; rt < NR; ++rt)
        if (rt < nrt) {
          acc[rt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[rt][sk], b4.x, acc[rt][0], 0, 0, 0);
          acc[rt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[rt][sk], b4.y, acc[rt][1], 0, 0, 0);
          acc[rt][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[rt][sk], b4.z, acc[rt][2], 0, 0, 0);
          acc[rt][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[rt][sk], b4.w, acc[rt][3], 0, 0, 0);
        }
    }
  }
  // ---- normalise and hand the context rows back in the queries' place ----
#pragma unroll
  for (int rt = 0; rt < NR; ++rt) {
    if (rt < nrt) {
      float l = l_run[rt];
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float inv = 1.f / __shfl(l, 4 * g + reg, 64);  // lane 4g + reg holds the denominator of row 16 rt + 4g + reg
        const int row = rt * 16 + 4 * g + reg;
        if (row < R)
          *reinterpret_cast<float4*>(qrows + (size_t)row * D + 64 * wave + 4 * col) =
              make_float4(acc[rt][0][reg] * inv, acc[rt][1][reg] * inv, acc[rt][2][reg] * inv, acc[rt][3][reg] * inv);
      }
    }
  }
}

// one beam step of a layer's row work: pre (per hypothesis) -> cross (per sample) -> post (per hypothesis).
// seg / nsamples: the samples' row segments (batched beam), or nullptr / 1 for a single sample whose rows are [0, r.M).
hipError_t launch_decoder_row_beam(const DecRowP& r, const float* mem, long long mem_stride, const float* wk, const float* wv_t,
                                   const float* bv, float* qp, float* x1, const int* seg, int nsamples, hipStream_t s) {
  if (r.heads != 8 || r.D != 256 || r.T < 1 || !qp || !x1 || nsamples < 1) return hipErrorInvalidValue;
  DecRow2P q{r, mem, mem_stride, wk, wv_t, bv, qp, x1, nullptr, nullptr};
  hipLaunchKernelGGL((decoder_row_absorbed_kernel<256, 1>), dim3(r.M), dim3(256), 0, s, q);
  BeamCrossP c{mem, mem_stride, r.T, qp, seg, r.M, r.step_ptr, r.stop_at};
  hipLaunchKernelGGL(beam_cross_kernel, dim3(nsamples), dim3(256), 0, s, c);
  hipLaunchKernelGGL((decoder_row_absorbed_kernel<256, 2>), dim3(r.M), dim3(256), 0, s, q);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// decoder_row_kernel for TWO rows per block (round 4; d_model 512 = config C1's decoder).  rocprofv3 of C1's serving run: the
// one-row kernel is 43 % of the kernel time at 62.8 us per launch, and a third of that is the three row GEMVs pulling 3 x 1 MB
// of weights through the CU's 64 B/clk L2 path for ONE row.  Here the block's 512 threads fetch every weight element once and
// apply it to both rows' inputs (two accumulators; the same K groups of D / 4 in the same order: per row bit-identical to the
// one-row kernel), and each wave runs ITS head of both rows in one attention loop (twice the K / V groups in flight per round
// trip, row_attention_2h).  An odd row count: the last block's second half repeats the last row and keeps its stores to itself.
// ---------------------------------------------------------------------------------------------------------------------
template <int D, int HD>
__global__ __launch_bounds__(512, 1) void decoder_row2_kernel(const DecRowP p) {
  constexpr int NTH = 512, G = NTH / (D / 4);
  static_assert(D / HD == 8 && NTH / 64 == 8, "one wave per head");
  ROW_KERNEL_ENTRY(p, false);
  __shared__ __attribute__((aligned(16))) float a_s[2][D], y_s[2][D], x1_s[2][D], q2_s[2][D], part_s[2][G * D];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int t = *p.step_ptr;
  int b[2];
  bool valid[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    valid[r] = 2 * (int)blockIdx.x + r < p.M;
    b[r] = valid[r] ? 2 * blockIdx.x + r : p.M - 1;
  }
  // ---- self-attention: wave = head, both rows in one loop ----
  {
    HeadPair h2;
#pragma unroll
    for (int r = 0; r < 2; ++r) h2.set(r, cache_append_and_heads<D, HD>(p, b[r], wave, t, lane, valid[r]), a_s[r] + wave * HD);
    row_attention_2h<4, HD>(h2.q, h2.K, h2.V, h2.curk, h2.curv, t, t + 1, h2.out, lane);
  }
  __syncthreads();
  gemv2<D, NTH, 16>(a_s[0], a_s[1], p.wo_t, part_s[0], part_s[1], tid);
  __syncthreads();
  for (int i = tid; i < 2 * D; i += NTH) {
    const int r = i / D, c = i % D;
    y_s[r][c] = sum_parts<G, D>(part_s[r], c, p.bo[c] + p.xres[(size_t)(r ? b[1] : b[0]) * D + c]);
  }
  __syncthreads();
  if (wave < 2) row_ln1<D>(y_s[wave], x1_s[wave], lane, p);  // one wave per row
  __syncthreads();
  gemv2<D, NTH, 16>(x1_s[0], x1_s[1], p.wq_t, part_s[0], part_s[1], tid);
  __syncthreads();
  for (int i = tid; i < 2 * D; i += NTH) {
    const int r = i / D, c = i % D;
    q2_s[r][c] = sum_parts<G, D>(part_s[r], c, p.bq[c]);
  }
  __syncthreads();
  // ---- cross-attention over the projected memory K / V: wave = head, both rows in one loop ----
  {
    const int head = wave;
    const float *qh[2], *Kh[2], *Vh[2];
    const float* none[2] = {nullptr, nullptr};
    float* oh[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int cb = p.c_row_map ? p.c_row_map[b[r]] : b[r];
      Kh[r] = p.ck + (size_t)cb * p.c_batch_stride + (size_t)head * p.T * HD;
      Vh[r] = p.cv + (size_t)cb * p.c_batch_stride + (size_t)head * p.T * HD;
      qh[r] = q2_s[r] + head * HD; oh[r] = a_s[r] + head * HD;
    }
    row_attention_2h<8, HD>(qh, Kh, Vh, none, none, -1, p.T, oh, lane);
  }
  __syncthreads();
  gemv2<D, NTH, 16>(a_s[0], a_s[1], p.wco_t, part_s[0], part_s[1], tid);
  __syncthreads();
  for (int i = tid; i < 2 * D; i += NTH) {
    const int r = i / D, c = i % D;
    const float v = sum_parts<G, D>(part_s[r], c, p.bco[c] + x1_s[r][c]);
    if (r ? valid[1] : valid[0]) p.y2[(size_t)(r ? b[1] : b[0]) * D + c] = v;
  }
}

hipError_t launch_decoder_row(const DecRowP& p, hipStream_t s) {
  if (p.heads != 8) return hipErrorInvalidValue;
  const bool small = decode_small() != 0;
  if (p.D == 256 && small) hipLaunchKernelGGL((decoder_row_kernel<256, 32, 256>), dim3(p.M), dim3(256), 0, s, p);
  else if (p.D == 256) hipLaunchKernelGGL((decoder_row_kernel<256, 32, 512>), dim3(p.M), dim3(512), 0, s, p);
  else if (p.D == 512 && !p.anc && !p.one_row && !D2T_PROBE_ENV_STR("D2T_DECODE_ONE_ROW_BLOCKS"))
    hipLaunchKernelGGL((decoder_row2_kernel<512, 64>), dim3((p.M + 1) / 2), dim3(512), 0, s, p);
  else if (p.D == 512) hipLaunchKernelGGL((decoder_row_kernel<512, 64, 512>), dim3(p.M), dim3(512), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Beam search device side (reference: tfm.py:145-186 runs the model, tools/beam.py:68-105
// does log_softmax + flat top-k on the host).
// ---------------------------------------------------------------------------
__global__ void embed_tokens_kernel(const float* __restrict__ emb, const float* __restrict__ pe,
                                    const int64_t* __restrict__ tok, const int* __restrict__ step_ptr,
                                    float* __restrict__ x, int d, float sqrt_d, const int* __restrict__ rows_ptr,
                                    const int* __restrict__ stop) {
  const int b = blockIdx.x, t = *step_ptr;
  if ((rows_ptr && b >= *rows_ptr) || (stop && *stop && t >= *stop)) return;
  const int64_t tk = tok[b];
  for (int c = threadIdx.x; c < d; c += blockDim.x)
    x[(size_t)b * d + c] = emb[(size_t)tk * d + c] * sqrt_d + pe[(size_t)t * d + c];
}
hipError_t launch_embed_tokens(const float* emb, const float* pe, const int64_t* tok, const int* step_ptr, float* x,
                               int M, int d, hipStream_t s, const int* rows_ptr, const int* stop) {
  hipLaunchKernelGGL(embed_tokens_kernel, dim3(M), dim3(256), 0, s, emb, pe, tok, step_ptr, x, d, sqrtf((float)d), rows_ptr, stop);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void beam_topk_kernel(const float* __restrict__ logits,
                                                        const float* __restrict__ scores, int V,
                                                        float* __restrict__ topv, int* __restrict__ topi,
                                                        const int* __restrict__ seg, int kmax,
                                                        const int* __restrict__ step, const int* __restrict__ stop) {
  if (stop && *stop && *step >= *stop) return;  // device-side beam loop: every sample has finished
  // this block's segment of rows
  const int off = seg[blockIdx.x * 3], M = seg[blockIdx.x * 3 + 1], k = seg[blockIdx.x * 3 + 2];
  if (M <= 0 || k <= 0) return;  // block-uniform
  logits += (size_t)off * V;
  scores += off;
  topv += (size_t)blockIdx.x * kmax;
  topi += (size_t)blockIdx.x * kmax;
  __shared__ float s_lse[16];
  __shared__ float r_v[4];
  __shared__ int r_i[4];
  __shared__ float sel_v;
  __shared__ int sel_i;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // log-sum-exp of every row (F.log_softmax, tfm.py:169)
  for (int i = wave; i < M; i += 4) {
    const float* row = logits + (size_t)i * V;
    float mx = -INFINITY;
    for (int v = lane; v < V; v += 64) mx = fmaxf(mx, row[v]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += expf(row[v] - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) s_lse[i] = mx + logf(sum);
  }
  __syncthreads();
  const int total = M * V;
  float last_v = INFINITY;
  int last_i = -1;
  for (int sel = 0; sel < k; ++sel) {
    // best candidate strictly after (last_v, last_i) in (value desc, index asc) order
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int idx = tid; idx < total; idx += 256) {
      const int i = idx / V;
      const float c = scores[i] + (logits[idx] - s_lse[i]);
      const bool after = c < last_v || (c == last_v && idx > last_i);
      if (after && (c > bv || (c == bv && idx < bi))) { bv = c; bi = idx; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { r_v[wave] = bv; r_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w)
        if (r_v[w] > bv || (r_v[w] == bv && r_i[w] < bi)) { bv = r_v[w]; bi = r_i[w]; }
      sel_v = bv; sel_i = bi;
      topv[sel] = bv; topi[sel] = bi;
    }
    __syncthreads();
    last_v = sel_v; last_i = sel_i;
    __syncthreads();
  }
}
hipError_t launch_beam_topk_batch(const float* logits, const float* scores, const int* seg, int N, int V, int kmax,
                                  float* topv, int* topi, hipStream_t s, const int* step, const int* stop) {
  if (N < 1 || kmax < 1 || kmax > 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_topk_kernel, dim3(N), dim3(256), 0, s, logits, scores, V, topv, topi, seg, kmax, step, stop);
  return hipGetLastError();
}

__global__ void cache_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                    const int* __restrict__ prev, int cap, int M, int heads, int Lmax, int hd,
                                    int rows) {
  // grid: (slab, i, head); copies rows*hd contiguous floats
  const int slab = blockIdx.x, i = blockIdx.y, h = blockIdx.z;
  const size_t per_row = (size_t)heads * Lmax * hd;
  const float* s = src + ((size_t)slab * cap + prev[i]) * per_row + (size_t)h * Lmax * hd;
  float* d = dst + ((size_t)slab * cap + i) * per_row + (size_t)h * Lmax * hd;
  const int n4 = rows * hd / 4;
  for (int c = threadIdx.x; c < n4; c += blockDim.x)
    reinterpret_cast<float4*>(d)[c] = reinterpret_cast<const float4*>(s)[c];
}
hipError_t launch_cache_gather(const float* src, float* dst, const int* prev, int slabs, int cap, int M, int heads,
                               int Lmax, int hd, int rows, hipStream_t s) {
  hipLaunchKernelGGL(cache_gather_kernel, dim3(slabs, M, heads), dim3(256), 0, s, src, dst, prev, cap, M, heads, Lmax,
                     hd, rows);
  return hipGetLastError();
}

// Beam search without the cache copy: anc[row][j] = cache row that holds position j of hypothesis `row`.  Before step t
// (read from the host's step pack) the survivors inherit their parent's ancestry and add the parent's row for position
// t - 1; the kernel also publishes t in the engine's step counter.  One block per row.
__global__ void beam_ancestry_kernel(const int* __restrict__ anc_old, int* __restrict__ anc_new, const int* __restrict__ prev,
                                     int stride, const int* __restrict__ step_in, int* __restrict__ step_out,
                                     const int* __restrict__ rows_ptr, const int* __restrict__ stop) {
  const int t = *step_in, row = blockIdx.x;
  if (row == 0 && threadIdx.x == 0) *step_out = t;
  if (!anc_new || t < 1) return;
  if ((rows_ptr && row >= *rows_ptr) || (stop && *stop && t >= *stop)) return;
  const int p = prev[row];
  const int* src = anc_old + (size_t)p * stride;
  int* dst = anc_new + (size_t)row * stride;
  for (int j = threadIdx.x; j < t - 1; j += blockDim.x) dst[j] = src[j];
  if (threadIdx.x == 0) dst[t - 1] = p;
}
hipError_t launch_beam_ancestry(const int* anc_old, int* anc_new, const int* prev, int rows, int stride, const int* step_in,
                                int* step_out, hipStream_t s, const int* rows_ptr, const int* stop) {
  if (rows < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_ancestry_kernel, dim3(rows), dim3(64), 0, s, anc_old, anc_new, prev, stride, step_in, step_out, rows_ptr, stop);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Device-side beam bookkeeping (round 4): Beam.advance (tools/beam.py:68-105) for every sample of a batched beam search in ONE
// single-block launch per step, so that the step loop needs no host round trip and can be captured as a graph.
// Thread i owns sample i (i, i + 256, ...).  Pass 1: its `live` candidates in order -- prev = idx / V, word = idx % V; a
// candidate ending in [s] joins the sample's completed set (step, parent row, score), the others become next step's
// hypotheses; a sample with `beam` completed hypotheses is finished (Beam.done) and its rows drop out.  Pass 2: the samples'
// new row counts are prefix-summed (rows stay compact, in sample order, as the host version kept them).  Pass 3: the new rows'
// token / score / sample / parent, and the (parent, token) history record the host walks back through at the end.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_dev_init_kernel(const BeamDev b, long long go_token) {
  for (int i = threadIdx.x; i < b.N; i += 256) {
    b.seg[3 * i] = i; b.seg[3 * i + 1] = 1; b.seg[3 * i + 2] = b.beam;
    b.tok[i] = go_token; b.scores[i] = 0.f; b.map[i] = i; b.prev[i] = i;
    b.comp_n[i] = 0; b.fin[i] = 0;
  }
  if (threadIdx.x == 0) { b.ctrl[0] = 0; b.ctrl[1] = b.N; b.ctrl[2] = 0; b.ctrl[3] = 0; }
}
hipError_t launch_beam_dev_init(const BeamDev& b, int64_t go_token, hipStream_t s) {
  hipLaunchKernelGGL(beam_dev_init_kernel, dim3(1), dim3(256), 0, s, b, (long long)go_token);
  return hipGetLastError();
}
__global__ __launch_bounds__(256) void beam_dev_advance_kernel(const BeamDev b) {
  constexpr int KMAX = 16, SPT = 4;  // beam <= 16; up to 4 samples per thread (N <= 1024)
  __shared__ int s_new[1024], s_off[1024];
  const int t = b.ctrl[0];
  if (b.ctrl[2] && t >= b.ctrl[2]) return;  // every sample finished at an earlier step
  int n_par[SPT][KMAX], n_word[SPT][KMAX];
  float n_val[SPT][KMAX];
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int i = threadIdx.x + 256 * q;
    if (i >= b.N) break;
    int newM = 0;
    if (!b.fin[i] && b.seg[3 * i + 1] > 0) {
      const int off = b.seg[3 * i], live = b.seg[3 * i + 2];
      int cn = b.comp_n[i];
      for (int r = 0; r < live; ++r) {
        const int idx = b.topi[(size_t)i * b.beam + r], prev = idx / b.V, word = idx - prev * b.V;
        const float val = b.topv[(size_t)i * b.beam + r];
        if (word == b.end_token) {
          b.comp_t[(size_t)i * b.beam + cn] = t; b.comp_par[(size_t)i * b.beam + cn] = off + prev; b.comp_score[(size_t)i * b.beam + cn] = val;
          ++cn;
        } else {
          n_par[q][newM] = off + prev; n_word[q][newM] = word; n_val[q][newM] = val;
          ++newM;
        }
      }
      b.comp_n[i] = cn;
      if (cn == b.beam) { b.fin[i] = 1; newM = 0; }
    }
    s_new[i] = newM;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // (N <= 1024 small integers: a serial scan is a microsecond)
    int run = 0;
    for (int i = 0; i < b.N; ++i) { s_off[i] = run; run += s_new[i]; }
    b.ctrl[0] = t + 1;
    b.ctrl[1] = run;
    b.ctrl[3] = t + 1;
    if (run == 0) b.ctrl[2] = t + 1;  // nothing left to extend: the remaining steps of the loop return at once
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int i = threadIdx.x + 256 * q;
    if (i >= b.N) break;
    const int off = s_off[i], newM = s_new[i];
    for (int j = 0; j < newM; ++j) {
      const int row = off + j;
      b.tok[row] = n_word[q][j]; b.scores[row] = n_val[q][j]; b.map[row] = i; b.prev[row] = n_par[q][j];
      b.hist_par[(size_t)t * b.cap + row] = n_par[q][j];
      b.hist_tok[(size_t)t * b.cap + row] = n_word[q][j];
    }
    b.seg[3 * i] = off; b.seg[3 * i + 1] = newM; b.seg[3 * i + 2] = b.fin[i] ? 0 : b.beam - b.comp_n[i];
  }
}
hipError_t launch_beam_dev_advance(const BeamDev& b, hipStream_t s) {
  if (b.N < 1 || b.N > 1024 || b.beam < 1 || b.beam > 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_dev_advance_kernel, dim3(1), dim3(256), 0, s, b);
  return hipGetLastError();
}

__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
  const long long total = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i / rows), r = (int)(i % rows);
    dst[i] = src[(size_t)r * cols + c];
  }
}
hipError_t launch_transpose(const float* src, float* dst, int rows, int cols, hipStream_t s) {
  const long long total = (long long)rows * cols;
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048)), dim3(256),
                     0, s, src, dst, rows, cols);
  return hipGetLastError();
}

}  // namespace d2t
