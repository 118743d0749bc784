// The decode step's skinny GEMM (gfx950, fp32):  y[M,N] = act(A @ w[N,K]^T + bias + res),  A = x or LayerNorm(x), in two
// block shapes with bitwise equal results plus a generic fallback.  The two shapes are two kernels, but every phase the bits
// depend on -- operand fetch, LayerNorm prologue, MFMA chain, epilogue value -- has ONE definition below.
// ln_out (the normalised rows as a side output) is where the two differ: the split-K kernel recomputes it in its epilogue
// loop from a second read of x and the rows' statistics, the wide kernel stores its A registers; both evaluate
// (x - mean) * rstd * g + b with the same association.
#include "decode_common.h"

namespace d2t {

// A finished step loop (stop_at: set by an EARLIER launch only) returns at once, block-uniform; the rest runs at the decode
// priority inside the launch's trace record.
#define SKINNY_KERNEL_ENTRY(p)                                              \
  if ((p).stop_at && *(p).stop_at && *(p).cur_step >= *(p).stop_at) return; \
  decode_wave_priority();                                                   \
  TraceScope trace_((p).trace)

__device__ __forceinline__ int skinny_wld(const SkinnyP& p) { return p.wld ? p.wld : p.K; }  // row stride of the weights

// NCH 16-byte chunks of row `row` of a row-major operand at column k0, 16 columns apart.  A row out of range (!ok) is
// fetched as row 0 and comes back as zeros.  (A chunk filled in place, not returned: up to 22 more VGPRs in the split-K builds.)
__device__ __forceinline__ float4 fetch_chunk(const float* src, bool ok) {
  float4 v = *reinterpret_cast<const float4*>(src);
  if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
  return v;
}
template <int NCH>
__device__ __forceinline__ void fetch_row(const float* base, int row, bool ok, int ld, int k0, float4* v) {
  const float* src = base + (size_t)(ok ? row : 0) * ld + k0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) v[c] = fetch_chunk(src + c * 16, ok);
}

// LayerNorm prologue on register-resident rows (post-norm decoder: the previous sub-layer's LayerNorm), two-pass.  A wave
// holds NT row sub-tiles of K slice `slice`: lane (r, q) has NCH chunks of block row row0 + 16 i (row0 includes r); the NW
// slices of a row meet in LDS.  Leaves s_mean / s_rstd filled and `a` normalised.  The association is the contract:
// (x + y) + (z + w) per chunk, chunks ascending, xor 16 then xor 32, slices ascending from zero.
// gamma / beta: c -> the scale / shift of chunk c (a load, or registers requested earlier).
template <int NT, int NCH, int NW, int ROWS, class Gamma, class Beta>
__device__ __forceinline__ void skinny_ln_prologue(float4 (&a)[NT][NCH], int slice, int row0, int q, int tid, int K, float eps,
                                                   float (&stat)[NW][ROWS], float (&s_mean)[ROWS], float (&s_rstd)[ROWS],
                                                   Gamma gamma, Beta beta) {
  const float invK = 1.f / (float)K;
  auto slice_sum = [&](int i, float s) {  // this slice's sum of sub-tile i's rows
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (q == 0) stat[slice][row0 + i * 16] = s;
  };
  auto row_sum = [&](int row) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += stat[w][row];
    return t;
  };
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) s += (a[i][c].x + a[i][c].y) + (a[i][c].z + a[i][c].w);
    slice_sum(i, s);
  }
  __syncthreads();
  if (tid < ROWS) s_mean[tid] = row_sum(tid) * invK;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const float mu = s_mean[row0 + i * 16];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      a[i][c].x -= mu; a[i][c].y -= mu; a[i][c].z -= mu; a[i][c].w -= mu;
      s += (a[i][c].x * a[i][c].x + a[i][c].y * a[i][c].y) + (a[i][c].z * a[i][c].z + a[i][c].w * a[i][c].w);
    }
    slice_sum(i, s);
  }
  __syncthreads();
  if (tid < ROWS) s_rstd[tid] = 1.f / sqrtf(row_sum(tid) * invK + eps);
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const float4 g4 = gamma(c), b4 = beta(c);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const float rs = s_rstd[row0 + i * 16];
      a[i][c].x = a[i][c].x * rs * g4.x + b4.x;
      a[i][c].y = a[i][c].y * rs * g4.y + b4.y;
      a[i][c].z = a[i][c].z * rs * g4.z + b4.z;
      a[i][c].w = a[i][c].w * rs * g4.w + b4.w;
    }
  }
}

// Chunk c of the K slice: four v_mfma_f32_16x16x4_f32 per accumulator, in the order x, y, z, w; the NI * NJ independent
// chains are interleaved.
template <int NI, int NJ, int NCH>
__device__ __forceinline__ void mfma_chunk(const float4 (&a)[NI][NCH], const float4 (&b)[NJ][NCH], int c, f32x4 (&acc)[NI][NJ]) {
#define D2T_MFMA_STEP(f)                                                                         \
  _Pragma("unroll") for (int i = 0; i < NI; ++i) _Pragma("unroll") for (int j = 0; j < NJ; ++j)  \
    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][c].f, b[j][c].f, acc[i][j], 0, 0, 0)
  D2T_MFMA_STEP(x);
  D2T_MFMA_STEP(y);
  D2T_MFMA_STEP(z);
  D2T_MFMA_STEP(w);
#undef D2T_MFMA_STEP
}

// The value of one output element from its sum over K: + bias, + residual only when the launch has one, activation.
__device__ __forceinline__ float skinny_tail(float v, float bias, bool has_res, float res, int act) {
  v += bias;
  if (has_res) v += res;
  return act_fn(v, act);
}
// ... whose sum over K is the NW slices' partials (part: w -> the partial of slice w), added in ascending w from zero
template <int NW, class Part>
__device__ __forceinline__ float skinny_out(Part part, float bias, bool has_res, float res, int act) {
  float v = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) v += part(w);
  return skinny_tail(v, bias, has_res, res, act);
}

// Split-K form.  M <= 64 rows per block row (the decode batch), weights streamed from L2 straight into registers.  Block
// tile (16 * MT) x 16; the K dimension is split over the NW waves of the block (each wave: all rows x its K-slice, every
// load issued before the first MFMA), partial tiles are summed through LDS.  The optional LayerNorm prologue runs on the
// register-resident rows with a cross-wave LDS reduction, so no standalone LayerNorm launch is needed.
template <int NW, int NCH, int MT>  // K == NW * NCH * 16; block tile (16*MT) rows x 16 columns
__global__ __launch_bounds__(NW * 64) void skinny_splitk_kernel(const SkinnyP p) {
  SKINNY_KERNEL_ENTRY(p);
  constexpr int KS = NCH * 16, ROWS = 16 * MT;
  __shared__ float part[NW][ROWS][17];
  __shared__ float stat[NW][ROWS];
  __shared__ float s_mean[ROWS], s_rstd[ROWS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, q = lane >> 4;
  const int mbase = blockIdx.y * ROWS;
  const int n = blockIdx.x * 16 + r;
  const int k0 = wave * KS + q * 4;

  float4 a[MT][NCH], b[1][NCH];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = mbase + i * 16 + r;
    fetch_row<NCH>(p.x, m, m < p.M, p.ldx, k0, a[i]);
  }
  fetch_row<NCH>(p.w, n, n < p.N, skinny_wld(p), k0, b[0]);

  if (p.ln_g)
    skinny_ln_prologue(a, wave, r, q, tid, p.K, p.ln_eps, stat, s_mean, s_rstd,
                       [g = p.ln_g + k0](int c) { return *reinterpret_cast<const float4*>(g + c * 16); },
                       [b = p.ln_b + k0](int c) { return *reinterpret_cast<const float4*>(b + c * 16); });

  f32x4 acc[MT][1] = {};
#pragma unroll
  for (int c = 0; c < NCH; ++c) mfma_chunk(a, b, c, acc);
  // C/D map: col = lane&15 -> n, row = (lane>>4)*4 + reg -> m
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) part[wave][i * 16 + q * 4 + reg][r] = acc[i][0][reg];
  __syncthreads();

  float* y = p.y;
  if (p.step_ptr) y += (long long)(*p.step_ptr) * p.out_step_stride;
  for (int idx = tid; idx < ROWS * 16; idx += NW * 64) {
    const int row = idx >> 4, col = idx & 15;
    const int m = mbase + row, nn = blockIdx.x * 16 + col;
    if (m >= p.M || nn >= p.N) continue;
    y[(size_t)m * p.ldy + nn] = skinny_out<NW>([&](int w) { return part[w][row][col]; }, p.bias ? p.bias[nn] : 0.f, p.res != nullptr,
                                               p.res ? p.res[(size_t)m * p.ldres + nn] : 0.f, p.act);
    if (p.ln_out && nn < p.K) {
      const float xv = p.x[(size_t)m * p.ldx + nn];
      p.ln_out[(size_t)m * p.K + nn] = (xv - s_mean[row]) * s_rstd[row] * p.ln_g[nn] + p.ln_b[nn];
    }
  }
}

// Wide form of the same GEMM for decode groups (M >= SKINNY_WIDE_MIN_M rows, where the kernel above is bound by the
// L2 traffic of its many small blocks): NWV waves own a block tile of (16*TM) rows x (16*TN) columns, so that every
// operand row is fetched by fewer blocks and the LayerNorm prologue runs once per 16*TN columns instead of once per 16.
// BITWISE the split-K kernel: a wave owns (16 x 16 sub-tile, K slice) units -- slice w = wave % NW, the row sub-tiles
// split over the NWV/NW waves of a slice -- each with its own accumulator (mfma_chunk) and its own LDS partial, summed by
// skinny_out; the LayerNorm statistics are skinny_ln_prologue's per-(row, slice) sums.
// Every global operand is requested before the first wait, the small ones first (the vector-memory counter retires in
// order): step, bias, residual tile, ln_g / ln_b, then the rows, then the weight rows.
template <int NW, int NCH, int TM, int TN, int NWV>  // K == NW * NCH * 16; NWV waves
__global__ __launch_bounds__(NWV * 64) void skinny_wide_kernel(const SkinnyP p) {
  SKINNY_KERNEL_ENTRY(p);
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
    fetch_row<NCH>(p.x, m, m < p.M, p.ldx, k0, a[i]);
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = nbase + j * 16 + r;
      fetch_row<1>(p.w, n, n < p.N, skinny_wld(p), k0 + c * 16, &b[j][c]);
    }
  }

  if (p.ln_g) {
    skinny_ln_prologue(a, w, i0 * 16 + r, q, tid, p.K, p.ln_eps, stat, s_mean, s_rstd, [&](int c) { return g4[c]; },
                       [&](int c) { return b4[c]; });
    // ln_out: a (row, column) has one writer, the block whose column tile holds that column (N >= K: launch_skinny)
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

  f32x4 acc[TMW][TN] = {};
#pragma unroll
  for (int c = 0; c < NCH; ++c) mfma_chunk(a, b, c, acc);
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
    y[(size_t)m * p.ldy + nn] =
        skinny_out<NW>([&](int ww) { return part[ww][st][wave & 3][lane]; }, bias_v[e], p.res != nullptr, res_v[e], p.act);
  }
}

// generic fallback (any K % 16 == 0, no LayerNorm prologue): one wave per 16 rows.  Its weight rows are K apart (SkinnyP::wld
// is the split-K builds'), and its one partial is not added to zero (0.f + acc would turn a -0.0 into +0.0): skinny_tail.
__global__ __launch_bounds__(256) void skinny_generic_kernel(const SkinnyP p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int m = blockIdx.y * 64 + wave * 16 + r;
  const int n = blockIdx.x * 16 + r;
  f32x4 acc[1][1] = {};
  const int KC = p.K >> 4;
  for (int c = 0; c < KC; ++c) {
    float4 a[1][1], b[1][1];
    fetch_row<1>(p.x, m, m < p.M, p.ldx, q * 4 + c * 16, a[0]);
    fetch_row<1>(p.w, n, n < p.N, p.K, q * 4 + c * 16, b[0]);
    mfma_chunk(a, b, 0, acc);
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
    y[(size_t)mm * p.ldy + nn] =
        skinny_tail(acc[0][0][reg], bias, p.res != nullptr, p.res ? p.res[(size_t)mm * p.ldres + nn] : 0.f, p.act);
  }
}

template <int NW, int NCH, int MT>
static void launch_splitk_tile(const SkinnyP& p, hipStream_t s) {
  const dim3 grid((p.N + 15) / 16, (p.M + 16 * MT - 1) / (16 * MT));
  hipLaunchKernelGGL((skinny_splitk_kernel<NW, NCH, MT>), grid, dim3(NW * 64), 0, s, p);
}
// narrow outputs (N <= 512) take 16-row tiles so that the few column tiles still fill >= 64 CUs
template <int NW, int NCH>
static void launch_splitk(const SkinnyP& p, hipStream_t s) {
  if (p.N <= 512) launch_splitk_tile<NW, NCH, 1>(p, s);
  else launch_splitk_tile<NW, NCH, 2>(p, s);
}
template <int NW, int NCH, int TM, int TN, int NWV>
static void launch_wide(const SkinnyP& p, hipStream_t s) {
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
    if (p.K == 256 && p.N > 512) launch_wide<4, 4, 2, 4, 4>(p, s);  // 32 x 64, four waves
    else if (p.K == 256) launch_wide<4, 4, 2, 2, 4>(p, s);          // narrow outputs: 32 x 32
    else if (p.K == 512) launch_wide<8, 4, 2, 2, 8>(p, s);          // 32 x 32, eight waves
    else launch_wide<8, 8, 2, 1, 8>(p, s);                          // 32 x 16
    return hipGetLastError();
  }
  if (form != SKINNY_FORM_SPLITK) return hipErrorInvalidValue;
  if (p.K == 256) launch_splitk<4, 4>(p, s);
  else if (p.K == 512) launch_splitk<8, 4>(p, s);
  else if (p.K == 1024 && decode_small() && !p.ln_g && !p.step_ptr) {
    // two 256-thread passes over the halves of K (second pass accumulates onto the first through the residual input)
    SkinnyP a = p, b = p;
    a.K = 512; a.ldx = p.ldx; a.w = p.w; a.wld = p.K;
    b.K = 512; b.x = p.x + 512; b.w = p.w + 512; b.wld = p.K; b.bias = nullptr; b.res = p.y; b.ldres = p.ldy;
    a.act = ACT_NONE;
    if (p.act != ACT_NONE) return hipErrorInvalidValue;
    launch_splitk_tile<4, 8, 1>(a, s);
    launch_splitk_tile<4, 8, 1>(b, s);
  }
  else if (p.K == 1024) launch_splitk<8, 8>(p, s);
  else {
    if (p.ln_g) return hipErrorInvalidValue;
    hipLaunchKernelGGL(skinny_generic_kernel, dim3((p.N + 15) / 16, (p.M + 63) / 64), dim3(256), 0, s, p);
  }
  return hipGetLastError();
}

}  // namespace d2t
