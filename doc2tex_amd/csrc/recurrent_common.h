// Device helpers shared by the recurrent kernels: the BiLSTM and LSTM-attention decoder of inference (recurrent.hip) and
// their backward kernels (train_recurrent.hip); ops.hip takes the block reductions from here.  Each states the order of its
// floating-point operations: the kernels' results are compared bit for bit across builds.
#pragma once
#include <hip/hip_runtime.h>

#include "train_common.h"

namespace d2t {

constexpr int LSTM_RB = 4;   // batch rows per block of the BiLSTM kernels, forward and backward
constexpr int AD_MAXT = 4096;  // keys per row of the LSTM-attention kernels, forward and backward (alignment rows in LDS)

static __device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// One LSTM cell from its four pre-activation gates (order i, f, g, o) and the cell state before the step.
// c = fma(i, g, round(f * c_prev)): spelled out, because left to contraction `f * c_prev + i * g` fused either product,
// depending on the code around it.
struct LstmCell { float ig, fg, gg, og, c, h; };
static __device__ __forceinline__ LstmCell lstm_cell(float ai, float af, float ag, float ao, float c_prev) {
  LstmCell r;
  r.ig = sigmoidf_(ai); r.fg = sigmoidf_(af);
  r.gg = tanhf(ag); r.og = sigmoidf_(ao);
  r.c = fmaf(r.ig, r.gg, r.fg * c_prev);
  r.h = r.og * tanhf(r.c);
  return r;
}

// Its backward from the saved gates, c_prev, tanh(c) and the gradients of h and (from the step behind) c:
// the gradients of the pre-activation gates and of c_prev.
struct LstmCellGrad { float dai, daf, dag, dao, dc_prev; };
static __device__ __forceinline__ LstmCellGrad lstm_cell_bwd(float ig, float fg, float gg, float og, float c_prev,
                                                             float tc, float dh, float dc_in) {
  const float dc = dc_in + dh * og * (1.f - tc * tc);
  LstmCellGrad r;
  r.dai = dc * gg * ig * (1.f - ig); r.daf = dc * c_prev * fg * (1.f - fg);
  r.dag = dc * ig * (1.f - gg * gg); r.dao = dh * tc * og * (1.f - og);
  r.dc_prev = dc * fg;
  return r;
}

// Location term of key t for the lane's four channels n0..n0+3: bias + sum over taps of the folded filter wloc_s [tap][H]
// times the alignment memory mem_s around t (zero outside [0, Tk)), one fmaf per tap in tap order.
static __device__ __forceinline__ float4 loc_term(const float* mem_s, const float* wloc_s, float4 bl4, int t, int taps,
                                                  int half, int Tk, int n0) {
  constexpr int H = 256;
  float4 lc = bl4;
  for (int j = 0; j < taps; ++j) {
    const int tt = t + j - half;
    const float m = (tt >= 0 && tt < Tk) ? mem_s[tt] : 0.f;
    const float4 wl = *reinterpret_cast<const float4*>(wloc_s + j * H + n0);
    lc.x = fmaf(wl.x, m, lc.x); lc.y = fmaf(wl.y, m, lc.y);
    lc.z = fmaf(wl.z, m, lc.z); lc.w = fmaf(wl.w, m, lc.w);
  }
  return lc;
}

// part[0][i] + part[1][i] + ... + part[N-1][i], left to right from 0 (rows `stride` floats apart)
template <int N>
static __device__ __forceinline__ float sum_parts(const float* part, int stride, int i) {
  float a = 0.f;
#pragma unroll
  for (int q = 0; q < N; ++q) a += part[q * stride + i];
  return a;
}
// four parts, pairwise: (p0 + p1) + (p2 + p3)
static __device__ __forceinline__ float sum_parts4_paired(const float* part, int stride, int i) {
  return (part[i] + part[stride + i]) + (part[2 * stride + i] + part[3 * stride + i]);
}
// Sum of v over the block's WAVES waves, in every thread: wave butterfly, then the wave sums left to right from 0.  red:
// WAVES floats nobody else touches until the block's next barrier.
template <int WAVES = 16>
static __device__ __forceinline__ float block_sum(float v, float* red, int wave, int lane) {
  v = wsum(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return sum_parts<WAVES>(red, 1, 0);
}

// Maximum of v over the block's WAVES waves, in every thread; red as above.
template <int WAVES = 16>
static __device__ __forceinline__ float block_max(float v, float* red, int wave, int lane) {
  v = wmax(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) v = fmaxf(v, red[w]);
  return v;
}

// The argmax's total order (value descending, index ascending): does (v, i) come before (bv, bi)?
static __device__ __forceinline__ bool argmax_better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}
// every lane of the wave gets the wave's first element in that order
static __device__ __forceinline__ void wave_argmax_first(float& best, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (argmax_better(ov, oi, best, bi)) { best = ov; bi = oi; }
  }
}

}  // namespace d2t
