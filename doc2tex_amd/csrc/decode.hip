// Decode-step kernels (gfx950, fp32): everything the KV-cached greedy / beam loop
// launches once per generated token.  Replaces, for the newest position only, what
// nn.TransformerDecoder recomputes over the whole prefix at every step in the
// reference (prediction_head/tfm.py:125-140).  All position-dependent values are
// read from a device-side step counter so one captured hipGraph replays for every step.
// This file: the small step kernels (attention of the unfused path, embedding, greedy argmax, ragged clean-up, transpose).
// The GEMMs are decode_gemm.hip's, the per-row decoder kernels decode_row.hip's, the beam search's device side decode_beam.hip's.
#include "decode_common.h"

namespace d2t {

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

__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
  const long long total = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i / rows), r = (int)(i % rows);
    dst[i] = src[(size_t)r * cols + c];
  }
}
hipError_t launch_transpose(const float* src, float* dst, int rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL(transpose_kernel, grid_1d((size_t)rows * cols, 2048), dim3(256), 0, s, src, dst, rows, cols);
  return hipGetLastError();
}

}  // namespace d2t
