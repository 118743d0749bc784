// What the per-row decoder kernels (decode_row.hip) and the beam search's per-sample cross-attention (decode_beam.hip) share:
// the online softmax of a 16-key score tile, and the hand-over between launch_decoder_row_beam and beam_cross_kernel.
#pragma once
#include "decode_common.h"

namespace d2t {

typedef __attribute__((address_space(3))) void* lds_ptr_dec;

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

// beam_cross_kernel's parameters (decode_beam.hip).  launch_decoder_row_beam lives with the row kernels whose MODE 1 / 2 builds
// it launches around this one, so that no __global__ template is instantiated in two objects; it reaches this kernel through
// launch_beam_cross.
struct BeamCrossP {
  const float* mem; long long mem_stride; int T;
  float* qp;            // [rows][8][256]
  const int* seg;       // [samples][3]: first row, live hypotheses, (unused) per sample; nullptr: one sample, rows [0, M)
  int M;                // seg == nullptr: live hypotheses
  const int* step_ptr; const int* stop_at;
};
#pragma GCC visibility push(hidden)
void launch_beam_cross(const BeamCrossP& p, int nsamples, hipStream_t s);  // one block per sample
#pragma GCC visibility pop

}  // namespace d2t
