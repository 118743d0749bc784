// Recurrent pieces of the recognizer path (gfx950, fp32): the bidirectional LSTM sequence model
// (seq_modeling/bilstm.py:6-24) and the LSTMCell attention decoder (prediction_head/seq2seq.py:224-331,
// seq2seq_v2.py:176-293, addon_module/attention1D.py:121-161,203-242).  These paths are sequential in time and
// row-local, so each is ONE launch that loops over all time steps inside the kernel.  Their backward kernels:
// train_recurrent.hip; the arithmetic both share: recurrent_common.h.
#include <algorithm>
#include <cstdint>

#include "../../include/d2t.h"
#include "kernels.h"
#include "recurrent_common.h"

namespace d2t {

// ---------------------------------------------------------------------------
// Bidirectional LSTM recurrence.  grid = (2 directions, ceil(B / LSTM_RB)); 1024 threads = the 4H gate rows (H = 256).
// W_hh^T [H][4H] is streamed from L2 each step with coalesced rows.  SAVE (the training forward): the gates after their
// nonlinearities and the cell state of every step are kept for the backward pass.
// ---------------------------------------------------------------------------
template <bool SAVE>
__global__ __launch_bounds__(1024) void bilstm_fwd_kernel(const float* __restrict__ g, const float* __restrict__ whh_t,
                                                          float* __restrict__ out, float* __restrict__ sv_gates,
                                                          float* __restrict__ sv_c, int B, int T, int H) {
  __shared__ float h_s[LSTM_RB][256], c_s[LSTM_RB][256], gate_s[LSTM_RB][1024];
  const int dir = blockIdx.x, b0 = blockIdx.y * LSTM_RB, r = threadIdx.x;
  const int G4 = 4 * H;
  const float* W = whh_t + (size_t)dir * H * G4;
  for (int i = r; i < LSTM_RB * H; i += 1024) { (&h_s[0][0])[i] = 0.f; (&c_s[0][0])[i] = 0.f; }
  __syncthreads();
  for (int step = 0; step < T; ++step) {
    const int t = dir == 0 ? step : T - 1 - step;
    float acc[LSTM_RB];
#pragma unroll
    for (int b = 0; b < LSTM_RB; ++b)
      acc[b] = (b0 + b < B) ? g[((size_t)(b0 + b) * T + t) * (2 * G4) + dir * G4 + r] : 0.f;
#pragma unroll 8
    for (int k = 0; k < H; ++k) {
      const float w = W[(size_t)k * G4 + r];
#pragma unroll
      for (int b = 0; b < LSTM_RB; ++b) acc[b] = fmaf(h_s[b][k], w, acc[b]);
    }
#pragma unroll
    for (int b = 0; b < LSTM_RB; ++b) gate_s[b][r] = acc[b];
    __syncthreads();
    {
      const int b = r >> 8, j = r & 255;  // 4 rows x 256 hidden units = 1024 threads
      if (b0 + b < B) {
        const LstmCell u = lstm_cell(gate_s[b][j], gate_s[b][H + j], gate_s[b][2 * H + j], gate_s[b][3 * H + j], c_s[b][j]);
        c_s[b][j] = u.c;
        h_s[b][j] = u.h;
        const size_t row = (size_t)(b0 + b) * T + t;
        out[row * (2 * H) + dir * H + j] = u.h;
        if constexpr (SAVE) {
          float* sg = sv_gates + row * (2 * G4) + dir * G4;
          sg[j] = u.ig; sg[H + j] = u.fg; sg[2 * H + j] = u.gg; sg[3 * H + j] = u.og;
          sv_c[row * (2 * H) + dir * H + j] = u.c;
        }
      }
    }
    __syncthreads();
  }
}

hipError_t launch_bilstm(const float* g, const float* whh_t, float* out, int B, int T, int H, hipStream_t s) {
  if (H != 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bilstm_fwd_kernel<false>, dim3(2, (B + LSTM_RB - 1) / LSTM_RB), dim3(1024), 0, s, g, whh_t, out,
                     (float*)nullptr, (float*)nullptr, B, T, H);
  return hipGetLastError();
}
hipError_t launch_bilstm_train_fwd(const float* gates, const float* whh_t, float* out, float* sv_gates, float* sv_c, int B, int T,
                                   int H, hipStream_t s) {
  if (H != 256 || B < 1 || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bilstm_fwd_kernel<true>, dim3(2, (B + LSTM_RB - 1) / LSTM_RB), dim3(1024), 0, s, gates, whh_t, out,
                     sv_gates, sv_c, B, T, H);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// LSTM-attention greedy decoder: one block (1024 threads) per batch row runs every step.
// D = E = H = 256, V <= D2T_ATTN_MAX_CLASSES, Tk <= 4096 keys (two alignment rows of that length in LDS: 32 of the block's
// 58 KB; the shipped max_dimension [800, 800] gives 2525).  The backward kernel of the training step keeps six such rows (96
// of its 134 KB).  WIDE = false: V <= 1024, one class per thread, logits staged in LDS for wave 0's argmax.  WIDE = true:
// any V, thread tid takes classes tid, tid + 1024, ... in order, keeps its first maximum, and the block reduces those.
// ---------------------------------------------------------------------------
// Early exit across blocks (AttnDecP::exit_state): a row that has just emitted [s] at `step` counts itself into the high
// half of the word and raises the low half to its end step, in ONE agent-scope compare-and-swap -- a reader on another
// XCD sees both halves of one update or neither, so no ordering between two words is needed.  Lock-free: a failed swap
// means another row's update went through.
__device__ __forceinline__ void attn_exit_publish(unsigned long long* w, int step) {
  unsigned long long old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    const unsigned cnt = (unsigned)(old >> 32) + 1u;
    const unsigned mx = (unsigned)old > (unsigned)step ? (unsigned)old : (unsigned)step;
    if (__hip_atomic_compare_exchange_strong(w, &old, ((unsigned long long)cnt << 32) | mx, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return;
  }
}
// thread 0, end of `step`, with the word as it read it at the start of the step: stop before step + 1?
__device__ __forceinline__ int attn_exit_reached(unsigned long long seen, int B, int step) {
  return (unsigned)(seen >> 32) == (unsigned)B && (unsigned)(step + 1) > (unsigned)seen;
}

// The generator's logit of class cls at (row b, step): bias + h . column, the output dropout of the training forward;
// stored to probs and returned.  (p by value here and in attn_end_step: by reference the kernel took 9 more VGPRs.)
__device__ __forceinline__ float attn_logit(const AttnDecP p, const float* h_s, int b, int step, int cls) {
  float v = p.bg[cls];
#pragma unroll 8
  for (int k = 0; k < 256; ++k) v = fmaf(h_s[k], p.wg_t[(size_t)k * p.V + cls], v);
  if (p.out_dropmask) v = p.out_dropmask[((size_t)b * p.S + step) * p.V + cls] ? v * p.out_dropscale : 0.f;
  p.probs[((size_t)b * p.S + step) * p.V + cls] = v;
  return v;
}

// The electing thread (thread 0) ends the step with the winning class: the next input token, the output token, the row's
// end step, and (EXIT) the row's end published to the other blocks and this block's decision to stop.
// GROUP: the row's batch has its own exit word `gword` and counts `grows` rows (AttnDecP::grp_*).
template <bool EXIT, bool GROUP = false>
__device__ __forceinline__ void attn_end_step(const AttnDecP p, int b, int step, int bi, int& ended,
                                              unsigned long long seen, int* tok_s, int* stop_s,
                                              [[maybe_unused]] unsigned long long* gword = nullptr,
                                              [[maybe_unused]] int grows = 0) {
  if (bi >= p.V) bi = 0;
  *tok_s = bi;
  p.tokens[(size_t)b * p.S + step] = bi;
  if (bi == p.end_token && !ended) {
    ended = 1;
    p.end_step[b] = step;
    if constexpr (EXIT) attn_exit_publish(GROUP ? gword : p.exit_state, step);
  }
  if constexpr (EXIT) *stop_s = attn_exit_reached(seen, GROUP ? grows : p.B, step);
}

// RAGGED (step mode only): the row's sample has its own memory length and its own place in ONE packed memory
// (AttnDecP::smp_row0 / smp_T), and the state / history rows have the stride st_ld.  The length is uniform within a block,
// so every barrier is still reached by all of its threads; no shared array is added.
// GUARD (RAGGED builds of the device-side beam loop, launched for every row slot): a block whose row is not live, or whose
// search has reached its stop step, returns here -- before any barrier, on words every thread of the block reads alike.
// GROUP (loop mode only: a greedy decode group, AttnDecP::grp_*): the row's memory length and first packed row come from
// the per-row tables, and (EXIT) the exit word and row count are those of the row's batch.  The table entries are read
// into scalar registers once, in front of the loop: everything derived from them is uniform in the block, as the uniform
// builds' kernel arguments are.
template <bool WIDE, bool EXIT, bool RAGGED = false, bool GUARD = false, bool GROUP = false>
__global__ __launch_bounds__(1024) void attn_decode_kernel(const AttnDecP p) {
  constexpr int H = 256;
  if constexpr (GUARD)
    if ((int)blockIdx.x >= p.guard[1] || (p.guard[2] && p.guard[0] >= p.guard[2])) return;
  __shared__ float x_s[3 * H];  // [context | embedding | h]  = LSTMCell input
  __shared__ float c_s[H], hq_s[H];
  __shared__ float mem_s[AD_MAXT + 16], alpha_s[AD_MAXT], red_s[32];
  __shared__ float gate_s[4 * H];
  __shared__ float logit_s[WIDE ? 16 : 1024];  // WIDE: each wave's best value
  __shared__ int besti_s[16];                  // WIDE: and its index
  __shared__ int tok_s;
  [[maybe_unused]] __shared__ int stop_s;  // EXIT: thread 0's decision, read by the block behind the step's last barrier
  __shared__ __attribute__((aligned(16))) float wloc_s[11 * H];  // folded location filter, [tap][n]
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // beam search: every hypothesis attends over its sample's keys (sample 0 unless a row map is given)
  const int bm = p.step_mode ? (p.row_sample ? p.row_sample[b] : 0) : b;
  // T: the sample's memory length, mrow: its first memory row, ld: the stride of the state and history rows.  RAGGED: Tk is
  // held to st_ld <= AD_MAXT here as well, whatever the tables say (the hosts refuse such tables before the launch)
  // GROUP: Tk is held to AD_MAXT, likewise
  const int T = GROUP ? __builtin_amdgcn_readfirstlane(p.grp_len[b]) : RAGGED ? p.smp_T[bm] : p.T;
  const int Tk = GROUP ? min(T - p.key_off, AD_MAXT) : RAGGED ? min(T - p.key_off, p.st_ld) : T - p.key_off;
  const int ld = RAGGED ? p.st_ld : Tk;
  const size_t mrow = GROUP ? (size_t)__builtin_amdgcn_readfirstlane(p.grp_row0[b]) : RAGGED ? (size_t)p.smp_row0[bm] : (size_t)bm * T;
  [[maybe_unused]] unsigned long long* gword = nullptr;  // GROUP, EXIT: the exit word of the row's batch and that batch's rows
  [[maybe_unused]] int grows = 0;
  if constexpr (GROUP && EXIT) {
    const int k = __builtin_amdgcn_readfirstlane(p.grp_row_batch[b]);
    gword = p.exit_state + k;
    grows = __builtin_amdgcn_readfirstlane(p.grp_batch_rows[k]);
  }
  const float* keys = p.mem + (mrow + p.key_off) * p.D;
  const float* kp = p.kp + (mrow + p.key_off) * H;
  float* ctx_s = x_s;
  float* emb_s = x_s + H;
  float* h_s = x_s + 2 * H;
  const int half = p.taps / 2;

  // ---- initial state (seq2seq.py:229-238) ----
  if (tid < H) {
    float init = 0.f;
    if (p.init_mode == 1) {
      for (int t = 0; t < T; ++t) init += p.mem[(mrow + t) * p.D + tid];
      init /= (float)T;
    } else if (p.init_mode == 2) {
      init = p.mem[mrow * p.D + tid];
    }
    hq_s[tid] = init;  // scratch
  }
  for (int i = tid; i < AD_MAXT + 16; i += 1024) mem_s[i] = 0.f;
  for (int i = tid; i < p.taps * H; i += 1024) wloc_s[i] = p.wloc[(i % H) * p.taps + i / H];
  __syncthreads();
  if (tid < H) {
    float hh = 0.f, cc = 0.f;
    if (p.init_mode != 0) {
      hh = p.bih[tid]; cc = p.bic[tid];
      for (int k = 0; k < p.D; ++k) {
        const float v = hq_s[k];
        hh = fmaf(v, p.wih_t[(size_t)k * H + tid], hh);
        cc = fmaf(v, p.wic_t[(size_t)k * H + tid], cc);
      }
    }
    h_s[tid] = hh;
    c_s[tid] = cc;
  }
  if (tid == 0) tok_s = 0;  // [GO]
  if constexpr (EXIT)
    if (tid == 0) stop_s = 0;
  int ended = 0;
  [[maybe_unused]] unsigned long long seen = 0;  // EXIT, thread 0: the exit word as of the start of the current step
  __syncthreads();
  if (p.step_mode && !p.first) {  // resume a hypothesis from its stored state
    if (tid < H) { h_s[tid] = p.st_h_in[(size_t)b * H + tid]; c_s[tid] = p.st_c_in[(size_t)b * H + tid]; }
    for (int t = tid; t < Tk; t += 1024) mem_s[t] = p.st_mem_in[(size_t)b * ld + t];
    if (tid == 0) tok_s = (int)p.tok_in[b];
    __syncthreads();
  }

  for (int step = 0; step < p.S; ++step) {
    // early exit: ONE lane looks at the word now (a load that bypasses the L1; nothing waits for it here) and the block
    // acts on it behind the step's last barrier
    if constexpr (EXIT)
      if (tid == 0) seen = __hip_atomic_load(GROUP ? gword : p.exit_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p.teacher && tid == 0) {
      if (step == 0 || !p.use_teacher || p.use_teacher[step]) tok_s = (int)p.teacher[(size_t)b * p.S + step];
      if (p.sv_tok) p.sv_tok[(size_t)b * p.S + step] = tok_s;  // otherwise: the argmax of the previous step
    }
    if (p.sv_hprev && tid < H) {
      p.sv_hprev[((size_t)b * p.S + step) * H + tid] = h_s[tid];
      p.sv_cprev[((size_t)b * p.S + step) * H + tid] = c_s[tid];
    }
    if (p.teacher) __syncthreads();
    // (1) query projection and target embedding
    if (tid < H) {
      float a = p.bq[tid];
#pragma unroll 8
      for (int k = 0; k < H; ++k) a = fmaf(h_s[k], p.wq_t[(size_t)k * H + tid], a);
      hq_s[tid] = a;
      emb_s[tid] = p.emb ? p.emb[(size_t)tok_s * p.E + tid] : 0.f;  // one-hot targets: see tokgate below
      if (p.sv_hq) p.sv_hq[((size_t)b * p.S + step) * H + tid] = a;
    }
    __syncthreads();
    // (2) scores: e[t] = w . tanh(key_proj[t] + query_proj + loc(mem)[t]) + b ; one wave per key
    {
      const int n0 = lane * 4;
      const float4 hq4 = *reinterpret_cast<const float4*>(hq_s + n0);
      const float4 ws4 = *reinterpret_cast<const float4*>(p.wscore + n0);
      const float4 bl4 = *reinterpret_cast<const float4*>(p.bloc + n0);
      for (int t = wave; t < Tk; t += 16) {
        const float4 k4 = *reinterpret_cast<const float4*>(kp + (size_t)t * H + n0);
        const float4 lc = loc_term(mem_s, wloc_s, bl4, t, p.taps, half, Tk, n0);
        const float e = wsum(ws4.x * tanhf(k4.x + hq4.x + lc.x) + ws4.y * tanhf(k4.y + hq4.y + lc.y) +
                             ws4.z * tanhf(k4.z + hq4.z + lc.z) + ws4.w * tanhf(k4.w + hq4.w + lc.w));
        if (lane == 0) alpha_s[t] = e + p.bscore;
      }
    }
    __syncthreads();
    // (3) softmax over the keys
    {
      float m = -INFINITY;
      for (int t = tid; t < Tk; t += 1024) m = fmaxf(m, alpha_s[t]);
      m = block_max(m, red_s, wave, lane);
      __syncthreads();
      float sum = 0.f;
      for (int t = tid; t < Tk; t += 1024) {
        const float ex = expf(alpha_s[t] - m);
        alpha_s[t] = ex;
        sum += ex;
      }
      const float inv = 1.f / block_sum(sum, red_s + 16, wave, lane);
      for (int t = tid; t < Tk; t += 1024) {
        const float a = alpha_s[t] * inv;
        alpha_s[t] = a;
        if (p.sv_alpha) p.sv_alpha[((size_t)b * p.S + step) * ld + t] = a;
        mem_s[t] = p.coverage ? mem_s[t] + a : a;  // coverage: accumulated alignment (seq2seq.py:302-304)
      }
      if constexpr (RAGGED)  // the history row beyond the sample's keys: zeros, so that a gathered map is defined there
        if (p.sv_alpha)
          for (int t = Tk + tid; t < ld; t += 1024) p.sv_alpha[((size_t)b * p.S + step) * ld + t] = 0.f;
    }
    __syncthreads();
    // (4) context = alpha^T keys : 4 key groups x 256 channels, reduced through LDS
    {
      const int c = tid & 255, gq = tid >> 8;
      float a = 0.f;
#pragma unroll 8
      for (int t = gq; t < Tk; t += 4) a = fmaf(alpha_s[t], keys[(size_t)t * p.D + c], a);
      gate_s[gq * H + c] = a;
    }
    __syncthreads();
    if (tid < H) {
      ctx_s[tid] = sum_parts4_paired(gate_s, H, tid);
      if (p.sv_x) {
        p.sv_x[((size_t)b * p.S + step) * (p.D + p.E) + tid] = ctx_s[tid];
        p.sv_x[((size_t)b * p.S + step) * (p.D + p.E) + p.D + tid] = emb_s[tid];
      }
    }
    __syncthreads();
    // (5) LSTMCell gates: thread = gate row, [ctx ; emb ; h] . W^T (coalesced transposed weights)
    {
      float a = p.bx[tid];
      if (p.tokgate) a += p.tokgate[(size_t)tok_s * 4 * H + tid];  // W_ih . onehot(token) = one column of W_ih
      const float* w = p.wx_t + tid;
      if constexpr (GROUP && WIDE && EXIT) {
        // the same sums in the same order, eight weight loads issued in front of their eight FMAs: left to the loop below,
        // the compiler waited for every load in this one build (s_waitcnt vmcnt(0) in front of each FMA);
        // the other three group builds keep eight loads in flight as they are
        for (int k = 0; k < 3 * H; k += 8) {
          float wv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) wv[u] = w[(size_t)(k + u) * 4 * H];
#pragma unroll
          for (int u = 0; u < 8; ++u) a = fmaf(x_s[k + u], wv[u], a);
        }
      } else {
#pragma unroll 8
        for (int k = 0; k < 3 * H; ++k) a = fmaf(x_s[k], w[(size_t)k * 4 * H], a);
      }
      gate_s[tid] = a;
    }
    __syncthreads();
    if (tid < H) {
      const LstmCell u = lstm_cell(gate_s[tid], gate_s[H + tid], gate_s[2 * H + tid], gate_s[3 * H + tid], c_s[tid]);
      c_s[tid] = u.c;
      h_s[tid] = u.h;
      if (p.sv_gates) {
        float* gs = p.sv_gates + ((size_t)b * p.S + step) * 4 * H;
        gs[tid] = u.ig; gs[H + tid] = u.fg; gs[2 * H + tid] = u.gg; gs[3 * H + tid] = u.og;
        p.sv_hafter[((size_t)b * p.S + step) * H + tid] = h_s[tid];
        p.sv_cafter[((size_t)b * p.S + step) * H + tid] = u.c;
      }
    }
    __syncthreads();
    // (6) generator logits + argmax: the first class in the order (value descending, index ascending), in thread 0
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if constexpr (WIDE) {  // each thread's classes, then the lanes, then the waves
      for (int cls = tid; cls < p.V; cls += 1024) {
        const float v = attn_logit(p, h_s, b, step, cls);
        if (argmax_better(v, cls, best, bi)) { best = v; bi = cls; }
      }
      wave_argmax_first(best, bi);
      if (lane == 0) { logit_s[wave] = best; besti_s[wave] = bi; }
      __syncthreads();
      if (tid == 0)
        for (int w = 1; w < 16; ++w)
          if (argmax_better(logit_s[w], besti_s[w], best, bi)) { best = logit_s[w]; bi = besti_s[w]; }
    } else {  // one class per thread, staged in LDS; wave 0 picks
      logit_s[tid] = tid < p.V ? attn_logit(p, h_s, b, step, tid) : -INFINITY;
      __syncthreads();
      if (wave == 0) {
        for (int i = lane; i < p.V; i += 64)
          if (argmax_better(logit_s[i], i, best, bi)) { best = logit_s[i]; bi = i; }
        wave_argmax_first(best, bi);
      }
    }
    if (tid == 0) attn_end_step<EXIT, GROUP>(p, b, step, bi, ended, seen, &tok_s, &stop_s, gword, grows);
    __syncthreads();
    if constexpr (EXIT)
      if (stop_s) break;
  }
  if (p.step_mode) {
    if (tid < H) { p.st_h_out[(size_t)b * H + tid] = h_s[tid]; p.st_c_out[(size_t)b * H + tid] = c_s[tid]; }
    for (int t = tid; t < Tk; t += 1024) p.st_mem_out[(size_t)b * ld + t] = mem_s[t];
  }
}

hipError_t launch_attn_decode(const AttnDecP& p, hipStream_t s) {
  if (p.H != 256 || p.D != 256 || p.E != 256 || p.V > D2T_ATTN_MAX_CLASSES || p.T - p.key_off > AD_MAXT ||
      p.taps > 11 || p.T - p.key_off < 1)
    return hipErrorInvalidValue;
  // the ragged build: step mode only, both per-sample tables, and a stride the two LDS rows can hold
  const bool ragged = p.smp_row0 || p.smp_T || p.st_ld;
  if (ragged && (!p.step_mode || p.S != 1 || p.teacher || p.exit_state || !p.smp_row0 || !p.smp_T || p.st_ld < 1 || p.st_ld > AD_MAXT))
    return hipErrorInvalidValue;
  if (p.guard && !ragged) return hipErrorInvalidValue;
  // the group builds: loop mode only, all four tables, no alignment history; one exit word per batch or none
  const bool group = p.grp_row0 || p.grp_len || p.grp_row_batch || p.grp_batch_rows;
  if (group) {
    if (ragged || p.step_mode || p.teacher || p.sv_alpha || !p.grp_row0 || !p.grp_len || !p.grp_row_batch || !p.grp_batch_rows)
      return hipErrorInvalidValue;
    auto k = p.V <= 1024 ? (p.exit_state ? attn_decode_kernel<false, true, false, false, true> : attn_decode_kernel<false, false, false, false, true>)
                         : (p.exit_state ? attn_decode_kernel<true, true, false, false, true> : attn_decode_kernel<true, false, false, false, true>);
    hipLaunchKernelGGL(k, dim3(p.B), dim3(1024), 0, s, p);
    return hipGetLastError();
  }
  if (p.guard) {
    hipLaunchKernelGGL((p.V <= 1024 ? attn_decode_kernel<false, false, true, true> : attn_decode_kernel<true, false, true, true>),
                       dim3(p.B), dim3(1024), 0, s, p);
    return hipGetLastError();
  }
  if (ragged) {
    hipLaunchKernelGGL((p.V <= 1024 ? attn_decode_kernel<false, false, true> : attn_decode_kernel<true, false, true>), dim3(p.B),
                       dim3(1024), 0, s, p);
    return hipGetLastError();
  }
  // EXIT builds (an exit_state is given: greedy is_test) carry the early exit across blocks; the others are the loop without
  // it, instruction for instruction (beam search's step mode, the training forward, greedy without is_test)
  if (p.exit_state && (p.step_mode || p.teacher)) return hipErrorInvalidValue;
  auto k = p.V <= 1024 ? (p.exit_state ? attn_decode_kernel<false, true> : attn_decode_kernel<false, false>)
                       : (p.exit_state ? attn_decode_kernel<true, true> : attn_decode_kernel<true, false>);
  hipLaunchKernelGGL(k, dim3(p.B), dim3(1024), 0, s, p);
  return hipGetLastError();
}

// The 4-byte words [a, e) of a buffer := 0 by thread i of n: 16-byte stores on the aligned body, single words at its ends.
__device__ __forceinline__ void zero_words(uint32_t* a, uint32_t* e, size_t i, size_t n) {
  if (a >= e) return;
  uint32_t* body = reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(a) + 15) & ~(uintptr_t)15);
  if (body > e) body = e;
  uint32_t* bend = body + ((size_t)(e - body) & ~(size_t)3);
  for (uint32_t* q = a + i; q < body; q += n) *q = 0u;
  for (uint4* q = reinterpret_cast<uint4*>(body) + i; q < reinterpret_cast<uint4*>(bend); q += n) *q = make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t* q = bend + i; q < e; q += n) *q = 0u;
}

// grid (x, y): blockIdx.y strides over the rows, the threads of the x blocks over a row's tail
__global__ __launch_bounds__(256) void attn_decode_finalize_kernel(const unsigned long long* exit_state, int* steps_dev, int B, int S, int V, int Tk,
                                                                   int64_t* tokens, float* probs, float* alpha) {
  const unsigned long long w = __hip_atomic_load(exit_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned mx = (unsigned)w;
  const int steps = ((unsigned)(w >> 32) == (unsigned)B && mx + 1u < (unsigned)S) ? (int)mx + 1 : S;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *steps_dev = steps;
  if (steps >= S) return;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = (size_t)gridDim.x * blockDim.x;
  for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
    const size_t r0 = b * S + steps, r1 = (b + 1) * S;  // (row, step) pairs to clear
    zero_words(reinterpret_cast<uint32_t*>(tokens + r0), reinterpret_cast<uint32_t*>(tokens + r1), i, n);
    zero_words(reinterpret_cast<uint32_t*>(probs + r0 * V), reinterpret_cast<uint32_t*>(probs + r1 * V), i, n);
    if (alpha) zero_words(reinterpret_cast<uint32_t*>(alpha + r0 * Tk), reinterpret_cast<uint32_t*>(alpha + r1 * Tk), i, n);
  }
}

hipError_t launch_attn_decode_finalize(const unsigned long long* exit_state, int* steps_dev, int B, int S, int V, int Tk,
                                       int64_t* tokens, float* probs, float* alpha, hipStream_t s) {
  if (!exit_state || !steps_dev || !tokens || !probs || B < 1 || S < 1 || V < 1 || Tk < 1) return hipErrorInvalidValue;
  const size_t row_vec = ((size_t)S * (size_t)std::max(V, Tk) + 3) / 4;  // 16-byte stores of a whole row, at most
  const unsigned gx = (unsigned)std::min<size_t>(64, (row_vec + 255) / 256);
  hipLaunchKernelGGL(attn_decode_finalize_kernel, dim3(gx, (unsigned)std::min(B, 256)), dim3(256), 0, s, exit_state,
                     steps_dev, B, S, V, Tk, tokens, probs, alpha);
  return hipGetLastError();
}

// The finalize kernel behind a group launch: row b belongs to batch row_batch[b], whose word and row count give its steps.
// Rows lie in batch order, so the first row of a batch is the one whose predecessor belongs to another batch: it stores
// the batch's step count.  grid as above.
__global__ __launch_bounds__(256) void attn_decode_finalize_group_kernel(const unsigned long long* exit_state, int* steps_dev,
                                                                         const int* __restrict__ row_batch,
                                                                         const int* __restrict__ batch_rows, int batches, int B,
                                                                         int S, int V, int64_t* tokens, float* probs) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = (size_t)gridDim.x * blockDim.x;
  if (!exit_state) {  // no early exit: every batch ran all S steps
    if (blockIdx.y == 0)
      for (size_t k = i; k < (size_t)batches; k += n) steps_dev[k] = S;
    return;
  }
  for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
    const int k = row_batch[b];
    const unsigned long long w = __hip_atomic_load(exit_state + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned mx = (unsigned)w;
    const int steps = ((unsigned)(w >> 32) == (unsigned)batch_rows[k] && mx + 1u < (unsigned)S) ? (int)mx + 1 : S;
    if (i == 0 && (b == 0 || row_batch[b - 1] != k)) steps_dev[k] = steps;
    if (steps >= S) continue;
    const size_t r0 = b * S + steps, r1 = (b + 1) * S;  // (row, step) pairs to clear
    zero_words(reinterpret_cast<uint32_t*>(tokens + r0), reinterpret_cast<uint32_t*>(tokens + r1), i, n);
    zero_words(reinterpret_cast<uint32_t*>(probs + r0 * V), reinterpret_cast<uint32_t*>(probs + r1 * V), i, n);
  }
}

hipError_t launch_attn_decode_finalize_group(const unsigned long long* exit_state, int* steps_dev, const int* row_batch,
                                             const int* batch_rows, int batches, int B, int S, int V, int64_t* tokens,
                                             float* probs, hipStream_t s) {
  if (!steps_dev || !row_batch || !batch_rows || !tokens || !probs || batches < 1 || B < batches || S < 1 || V < 1)
    return hipErrorInvalidValue;
  const size_t row_vec = ((size_t)S * (size_t)V + 3) / 4;  // 16-byte stores of a whole row, at most
  const unsigned gx = (unsigned)std::min<size_t>(64, (row_vec + 255) / 256);
  hipLaunchKernelGGL(attn_decode_finalize_group_kernel, dim3(gx, (unsigned)std::min(B, 256)), dim3(256), 0, s, exit_state,
                     steps_dev, row_batch, batch_rows, batches, B, S, V, tokens, probs);
  return hipGetLastError();
}

// Beam-search alignment maps: out[i][j][:] = hist[j][path[i*S + j]][:] for j < len[i], zeros for len[i] <= j < S.
// The output is walked as flat float4 chunks, so every store is 16 bytes (out comes from a 256-byte aligned allocation;
// a ragged tail of numel % 4 elements is stored one by one).  A chunk that lies inside one alignment row whose source is
// 16-byte aligned is read with one float4 load, any other chunk element by element.
__global__ void attn_alpha_gather_kernel(const float* __restrict__ hist, const int* __restrict__ path,
                                         const int* __restrict__ len, float* __restrict__ out, int N, int S, int cap, int Tk) {
  const size_t numel = (size_t)N * S * Tk;
  const size_t chunks = (numel + 3) / 4;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < chunks; k += (size_t)gridDim.x * blockDim.x) {
    const size_t e0 = k * 4;
    const size_t r0 = e0 / Tk;
    const int t0 = (int)(e0 - r0 * Tk);
    float v[4];
    if (t0 + 4 <= Tk) {  // one row
      const int i = (int)(r0 / S), j = (int)(r0 - (size_t)i * S);
      if (j >= len[i]) {
        v[0] = v[1] = v[2] = v[3] = 0.f;
      } else {
        const size_t src = ((size_t)j * cap + path[(size_t)i * S + j]) * Tk + t0;
        if ((src & 3) == 0) {
          const float4 q = *reinterpret_cast<const float4*>(hist + src);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = hist[src + u];
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t e = e0 + u;
        v[u] = 0.f;
        if (e >= numel) continue;
        const size_t r = e / Tk;
        const int t = (int)(e - r * Tk), i = (int)(r / S), j = (int)(r - (size_t)i * S);
        if (j < len[i]) v[u] = hist[((size_t)j * cap + path[(size_t)i * S + j]) * Tk + t];
      }
    }
    if (e0 + 4 <= numel) {
      *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int u = 0; e0 + u < numel; ++u) out[e0 + u] = v[u];
    }
  }
}
hipError_t launch_attn_alpha_gather(const float* hist, const int* path, const int* len, float* out, int N, int S, int cap,
                                    int Tk, hipStream_t s) {
  if (N <= 0 || S <= 0 || Tk <= 0) return hipSuccess;
  if (reinterpret_cast<uintptr_t>(out) & 15) return hipErrorInvalidValue;  // the float4 stores need a 16-byte aligned base
  const size_t chunks = ((size_t)N * S * Tk + 3) / 4;
  const int blocks = (int)std::min<size_t>((chunks + 255) / 256, 2048);
  hipLaunchKernelGGL(attn_alpha_gather_kernel, dim3(blocks), dim3(256), 0, s, hist, path, len, out, N, S, cap, Tk);
  return hipGetLastError();
}

__global__ void gather_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ idx,
                                   int width) {
  const int i = blockIdx.x;
  for (int c = threadIdx.x; c < width; c += blockDim.x) dst[(size_t)i * width + c] = src[(size_t)idx[i] * width + c];
}
hipError_t launch_gather_rows(const float* src, float* dst, const int* idx, int rows, int width, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(rows), dim3(256), 0, s, src, dst, idx, width);
  return hipGetLastError();
}

}  // namespace d2t
