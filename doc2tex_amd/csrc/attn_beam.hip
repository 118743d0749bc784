// Device-side bookkeeping of the LSTM-attention beam search (Attention.forward_beam, prediction_head/seq2seq.py:83-222;
// AttentionV2.forward_beam, seq2seq_v2.py:12-174): what the host loop of engine_attn.hip does between two steps with the
// host functions of attn_beam_host.h, as kernels over the same record (AttnBeamDev, defined there), so that the step loop
// needs no host round trip and can be captured as a graph.  attn_beam_host_init / _advance / _finish and the three kernels
// of those names write the same arrays; tests/attn_beam_refs.py holds both to one description.
// Every kernel here is ordered by launches alone: no block waits for another one.
#include <algorithm>
#include <cstdint>

#include "../../include/d2t.h"
#include "kernels.h"

namespace d2t {

namespace {
__device__ __forceinline__ bool attn_beam_stopped(const int* ctrl) { return ctrl[2] && ctrl[0] >= ctrl[2]; }
}  // namespace

// Step 0 as the host loop lays it out: `beam` identical rows per sample from the token [GO] with score 0, of which the
// reference ranks row 0 only (seq2seq.py:145-146): seg = {i * beam, 1, beam}.
__global__ __launch_bounds__(256) void attn_beam_dev_init_kernel(const AttnBeamDev b, long long go_token) {
  for (int i = threadIdx.x; i < b.N; i += 256) {
    b.seg[3 * i] = i * b.beam; b.seg[3 * i + 1] = 1; b.seg[3 * i + 2] = b.beam;
    b.comp_n[i] = 0; b.fin[i] = 0; b.last_completed[i] = 0;
  }
  for (int r = threadIdx.x; r < b.N * b.beam; r += 256) {
    b.tok[r] = go_token; b.scores[r] = 0.f; b.map[r] = r / b.beam; b.idx_h[r] = r; b.idx_m[r] = r;
  }
  if (threadIdx.x == 0) { b.ctrl[0] = 0; b.ctrl[1] = b.N * b.beam; b.ctrl[2] = 0; b.ctrl[3] = 0; }
}
hipError_t launch_attn_beam_dev_init(const AttnBeamDev& b, int64_t go_token, hipStream_t s) {
  if (b.N < 1 || b.N > 1024 || b.beam < 1 || b.beam > 16 || (long long)b.cap < (long long)b.N * b.beam) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_beam_dev_init_kernel, dim3(1), dim3(256), 0, s, b, (long long)go_token);
  return hipGetLastError();
}

// One step of the reference's bookkeeping for every sample, in ONE single-block launch (thread i owns samples i, i + 256, ...).
// Pass 1 counts a sample's survivors among its k candidates (prev = idx / V, word = idx % V; word == [s] completes the
// hypothesis).  Pass 2: the counts are prefix-summed, so the new rows are compact and in sample order, as the host loop keeps
// them.  Pass 3 walks the candidates again: a completion records (step, parent row, score) and nothing else; a survivor gets
// its row -- idx_h = parent row (the LSTM state follows prev_word_inds), idx_m = first row + rank (the coverage memory follows
// the candidate's rank: the reference's quirk), token, score, sample, and the (parent, token) record of the history.
// A sample whose k reaches 0 is finished; last_completed is rewritten only for the samples this step processed; no survivor
// anywhere sets the stop step.
__global__ __launch_bounds__(256) void attn_beam_dev_advance_kernel(const AttnBeamDev b) {
  constexpr int SPT = 4;  // samples per thread (N <= 1024)
  __shared__ int s_new[1024], s_off[1024];
  const int t = b.ctrl[0];
  if (attn_beam_stopped(b.ctrl)) return;  // every sample finished at an earlier step (uniform: nobody has written ctrl yet)
  int off_q[SPT], k_q[SPT];
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int i = threadIdx.x + 256 * q;
    off_q[q] = 0; k_q[q] = 0;
    if (i >= b.N) continue;
    int newM = 0;
    if (!b.fin[i]) {
      off_q[q] = b.seg[3 * i]; k_q[q] = b.seg[3 * i + 2];
      for (int r = 0; r < k_q[q]; ++r) newM += b.topi[(size_t)i * b.beam + r] % b.V != b.end_token;
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
    if (run == 0) b.ctrl[2] = t + 1;  // nothing left to extend: the remaining launches of the loop return at once
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int i = threadIdx.x + 256 * q;
    if (i >= b.N || k_q[q] <= 0) continue;  // (a finished sample keeps seg = {., 0, 0} and its last_completed)
    const int off = off_q[q], k = k_q[q], row0 = s_off[i], newM = s_new[i];
    int cn = b.comp_n[i], j = 0;
    for (int r = 0; r < k; ++r) {
      const int idx = b.topi[(size_t)i * b.beam + r], prev = idx / b.V, word = idx - prev * b.V;
      const float val = b.topv[(size_t)i * b.beam + r];
      if (word == b.end_token) {
        if (cn < b.beam) {  // (always: every completion lowers k)
          b.comp_t[(size_t)i * b.beam + cn] = t; b.comp_par[(size_t)i * b.beam + cn] = off + prev; b.comp_score[(size_t)i * b.beam + cn] = val;
          ++cn;
        }
      } else {
        const int row = row0 + j;
        b.idx_h[row] = off + prev;
        b.idx_m[row] = off + r;
        b.tok[row] = word; b.scores[row] = val; b.map[row] = i;
        b.hist_par[(size_t)t * b.cap + row] = off + prev;
        b.hist_tok[(size_t)t * b.cap + row] = word;
        ++j;
      }
    }
    b.last_completed[i] = j < k;
    b.comp_n[i] = cn;
    b.seg[3 * i] = row0; b.seg[3 * i + 1] = newM; b.seg[3 * i + 2] = newM;
    if (newM == 0) b.fin[i] = 1;
  }
}
hipError_t launch_attn_beam_dev_advance(const AttnBeamDev& b, hipStream_t s) {
  if (b.N < 1 || b.N > 1024 || b.beam < 1 || b.beam > 16 || (long long)b.cap < (long long)b.N * b.beam) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_beam_dev_advance_kernel, dim3(1), dim3(256), 0, s, b);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void attn_beam_dev_gather_kernel(const int* __restrict__ ctrl, const int* __restrict__ idx_h,
                                                                   const int* __restrict__ idx_m, const float* __restrict__ h_out,
                                                                   const float* __restrict__ c_out, const float* __restrict__ mem_out,
                                                                   float* __restrict__ h_in, float* __restrict__ c_in,
                                                                   float* __restrict__ mem_in, int H, int ld) {
  const int row = blockIdx.x;
  if (row >= ctrl[1] || attn_beam_stopped(ctrl)) return;
  const size_t ph = (size_t)idx_h[row], pm = (size_t)idx_m[row];
  for (int c = threadIdx.x; c < H; c += 256) {
    h_in[(size_t)row * H + c] = h_out[ph * H + c];
    c_in[(size_t)row * H + c] = c_out[ph * H + c];
  }
  for (int c = threadIdx.x; c < ld; c += 256) mem_in[(size_t)row * ld + c] = mem_out[pm * ld + c];
}
hipError_t launch_attn_beam_dev_gather(const int* ctrl, const int* idx_h, const int* idx_m, const float* h_out, const float* c_out,
                                       const float* mem_out, float* h_in, float* c_in, float* mem_in, int cap, int H, int ld,
                                       hipStream_t s) {
  if (cap < 1 || H < 1 || ld < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_beam_dev_gather_kernel, dim3(cap), dim3(256), 0, s, ctrl, idx_h, idx_m, h_out, c_out, mem_out, h_in,
                     c_in, mem_in, H, ld);
  return hipGetLastError();
}

// The final pick (seq2seq.py:209-222), one sample per thread.  The last step that processed the sample completed nothing: its
// first live hypothesis and that hypothesis's score (the sample then was live at the last step run).  Otherwise the completed
// hypothesis with the largest score / length -- in double, the first maximum, the length counting [GO] as the host's vectors
// do -- with the MAXIMUM raw completed score.  The tokens and (maps) the launch rows come from walking the history back.
__global__ __launch_bounds__(64) void attn_beam_dev_finish_kernel(const AttnBeamDev b, long long* __restrict__ seq, int* __restrict__ len,
                                                                  float* __restrict__ score, int* __restrict__ path,
                                                                  int* __restrict__ plen) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= b.N) return;
  long long* out = seq + (size_t)i * b.S;
  int* pa = path ? path + (size_t)i * b.S : nullptr;
  int t, row = 0, n = 0;
  float sc = 0.f;
  if (!b.last_completed[i]) {
    t = b.ctrl[3] - 1;  // the last step run
    if (b.seg[3 * i + 1] > 0 && t >= 0) { row = b.seg[3 * i]; sc = b.scores[row]; n = t + 1; }
    else t = -1;
  } else {
    const int cn = b.comp_n[i];
    const float* cs = b.comp_score + (size_t)i * b.beam;
    const int* ct = b.comp_t + (size_t)i * b.beam;
    int best = 0;
    t = -1;
    if (cn >= 1) {  // (always, after a step that completed something)
      sc = cs[0];
      for (int j = 1; j < cn; ++j) {
        if ((double)cs[j] / (double)(ct[j] + 2) > (double)cs[best] / (double)(ct[best] + 2)) best = j;
        sc = fmaxf(sc, cs[j]);
      }
      t = ct[best];
      n = t + 1;
      row = b.comp_par[(size_t)i * b.beam + best];
      out[t] = b.end_token;
      if (pa) pa[t] = row;
      --t;
    }
  }
  for (; t >= 0; --t) {
    out[t] = b.hist_tok[(size_t)t * b.cap + row];
    row = b.hist_par[(size_t)t * b.cap + row];
    if (pa) pa[t] = row;
  }
  for (int j = n; j < b.S; ++j) out[j] = 0;
  len[i] = n;
  score[i] = sc;
  if (plen) plen[i] = n;
}
hipError_t launch_attn_beam_dev_finish(const AttnBeamDev& b, int64_t* seq, int* len, float* score, int* path, int* plen,
                                       hipStream_t s) {
  if (b.N < 1 || b.N > 1024 || b.beam < 1 || b.beam > 16 || !seq || !len || !score || (path != nullptr) != (plen != nullptr))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_beam_dev_finish_kernel, dim3((b.N + 63) / 64), dim3(64), 0, s, b, reinterpret_cast<long long*>(seq), len,
                     score, path, plen);
  return hipGetLastError();
}

__global__ void attn_alpha_gather_ld_kernel(const float* __restrict__ hist, const int* __restrict__ path, const int* __restrict__ len,
                                            float* __restrict__ out, int N, int S, int cap, int ld, int Tk) {
  const size_t numel = (size_t)N * S * Tk;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / Tk;
    const int tk = (int)(e - r * Tk), i = (int)(r / S), j = (int)(r - (size_t)i * S);
    out[e] = j < len[i] ? hist[((size_t)j * cap + path[(size_t)i * S + j]) * ld + tk] : 0.f;
  }
}
hipError_t launch_attn_alpha_gather_ld(const float* hist, const int* path, const int* len, float* out, int N, int S, int cap,
                                       int ld, int Tk, hipStream_t s) {
  if (N <= 0 || S <= 0 || Tk <= 0) return hipSuccess;
  if (ld < Tk) return hipErrorInvalidValue;
  const size_t numel = (size_t)N * S * Tk;
  const int blocks = (int)std::min<size_t>((numel + 255) / 256, 4096);
  hipLaunchKernelGGL(attn_alpha_gather_ld_kernel, dim3(blocks), dim3(256), 0, s, hist, path, len, out, N, S, cap, ld, Tk);
  return hipGetLastError();
}

}  // namespace d2t
