// Cross-attention maps of the TFM decode (gfx950, fp32): the probabilities the row kernels of decode_row.hip fold into their
// running softmax and never keep.  Launched only by the teacher-forced replay (engine_tfm.hip d2t_decode_cross_attention) and
// by the operator entry d2t_op_cross_attn_probs; no decode launches it.
#include "decode_common.h"

namespace d2t {

// One block per query row, one wave per head.  The head's T scores go to LDS (T <= 4096: 16 KB per head, 128 KB per block),
// then a two-pass softmax over them: the maximum first, exp and sum second.  Per-head form: every wave writes its own
// normalised row.  Mean form: the normalised rows stay in LDS and the block sums them per key in head order 0 .. 7 (torch's
// average_attn_weights).  The key walk is row_attention's: HD / 4 lanes per key, a 16-byte load each, so a wave-wide load
// covers whole keys; the key bias is constant per head and cancels in the softmax, so the projected keys may carry it or not.
template <int HD>
__global__ __launch_bounds__(512) void cross_attn_probs_kernel(const CrossProbsP p) {
  constexpr int LPK = HD / 4, KPI = 64 / LPK;
  extern __shared__ __attribute__((aligned(16))) float sc_s[];  // [8][T]
  const int tid = threadIdx.x, head = tid >> 6, lane = tid & 63;
  const int kig = lane / LPK, ch = lane % LPK;
  const int b = blockIdx.x, T = p.T;
  const int cb = p.c_row_map ? p.c_row_map[b] : b;
  const float* Kc = p.ck + (size_t)cb * p.c_batch_stride + (size_t)head * T * HD;
  const float4 q4 = *reinterpret_cast<const float4*>(p.q + (size_t)b * p.q_stride + head * HD + ch * 4);
  const float scale = HD == 32 ? 0.17677669529663687f : 0.125f;
  float* sc = sc_s + (size_t)head * T;
  float mx = -INFINITY;
#pragma unroll 4
  for (int j0 = 0; j0 < T; j0 += KPI) {
    const int j = j0 + kig;
    const float4 k4 = *reinterpret_cast<const float4*>(Kc + (size_t)(j < T ? j : T - 1) * HD + ch * 4);
    float d = (q4.x * k4.x + q4.y * k4.y) + (q4.z * k4.z + q4.w * k4.w);
#pragma unroll
    for (int o = 1; o < LPK; o <<= 1) d += __shfl_xor(d, o, 64);
    if (j < T) {
      const float sj = d * scale;
      if (ch == 0) sc[j] = sj;
      mx = fmaxf(mx, sj);
    }
  }
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));  // key 0 is valid: finite in every lane
  __syncthreads();
  float l = 0.f;
  for (int j = lane; j < T; j += 64) {
    const float e = expf(sc[j] - mx);
    sc[j] = e;
    l += e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o, 64);
  float* out = p.out + (size_t)b * p.out_row_stride + (p.step_ptr ? (size_t)*p.step_ptr * T : 0);
  if (p.out_head_stride) {  // block-uniform
    float* oh = out + (size_t)head * p.out_head_stride;
    for (int j = lane; j < T; j += 64) oh[j] = sc[j] / l;
    return;
  }
  for (int j = lane; j < T; j += 64) sc[j] = sc[j] / l;
  __syncthreads();
  for (int j = tid; j < T; j += 512) {
    float s = sc_s[j];
#pragma unroll
    for (int h = 1; h < 8; ++h) s += sc_s[(size_t)h * T + j];
    out[j] = s * 0.125f;
  }
}

hipError_t launch_cross_attn_probs(const CrossProbsP& p, hipStream_t s) {
  constexpr int LDS_MAX = 8 * 4096 * (int)sizeof(float);
  static_assert(LDS_MAX <= 160 * 1024, "eight heads' scores of the longest memory fit the CU's LDS");
  if (p.M < 1 || p.T < 1 || p.T > 4096 || (p.D != 256 && p.D != 512) || !p.q || !p.ck || !p.out) return hipErrorInvalidValue;
  using Kernel = void (*)(const CrossProbsP);
  const Kernel k = p.D == 256 ? cross_attn_probs_kernel<32> : cross_attn_probs_kernel<64>;
  static bool attr_set[2] = {false, false};
  if (!attr_set[p.D == 512]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    if (e != hipSuccess) return e;
    attr_set[p.D == 512] = true;
  }
  hipLaunchKernelGGL(k, dim3(p.M), dim3(512), (size_t)8 * p.T * sizeof(float), s, p);
  return hipGetLastError();
}

}  // namespace d2t
