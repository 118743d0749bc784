// Backward kernels of the recurrent paths in the training step (train.hip), fp32: the bidirectional LSTM through time and
// the teacher-forced LSTM-attention loop, with the small kernels that finish their parameter gradients.  The forward
// kernels are inference's (recurrent.hip: bilstm_fwd_kernel<true>, attn_decode_kernel with the sv_* pointers set); the
// arithmetic both directions share is in recurrent_common.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/d2t.h"
#include "kernels.h"
#include "recurrent_common.h"

namespace d2t {

// ---------------------------------------------------------------------------
// BiLSTM backward through time, the forward's grid (2 directions, ceil(B / LSTM_RB)).  Per step (reverse processing
// order): phase 1, thread = (row, hidden unit): the cell's gradients and the pre-activation gate gradients (kept in LDS and
// written out); phase 2, thread = (quarter of the 4H gate rows, hidden unit k): dh_prev[b][k] = sum_r dgate[b][r] W_hh[r][k]
// for the block's four rows, each weight read once.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void bilstm_train_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ sv_gates,
                                                                const float* __restrict__ sv_c, const float* __restrict__ whh_fwd,
                                                                const float* __restrict__ whh_rev, float* __restrict__ dgates,
                                                                int B, int T, int H) {
  __shared__ float dh_s[LSTM_RB][256], dc_s[LSTM_RB][256], dg_s[LSTM_RB][1024], part_s[4][LSTM_RB][256];
  const int dir = blockIdx.x, b0 = blockIdx.y * LSTM_RB, tid = threadIdx.x;
  const int G4 = 4 * H;
  const float* W = dir == 0 ? whh_fwd : whh_rev;  // [4H][H]
  for (int i = tid; i < LSTM_RB * H; i += 1024) { (&dh_s[0][0])[i] = 0.f; (&dc_s[0][0])[i] = 0.f; }
  __syncthreads();
  for (int step = T - 1; step >= 0; --step) {
    const int t = dir == 0 ? step : T - 1 - step;
    const int tp = dir == 0 ? t - 1 : t + 1;  // the step processed before t (none when step == 0)
    {
      const int b = tid >> 8, j = tid & 255;
      LstmCellGrad d = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (b0 + b < B) {
        const size_t row = (size_t)(b0 + b) * T + t;
        const float* sg = sv_gates + row * (2 * G4) + dir * G4;
        const float ig = sg[j], fg = sg[H + j], gg = sg[2 * H + j], og = sg[3 * H + j];
        const float cc = sv_c[row * (2 * H) + dir * H + j];
        const float cp = step > 0 ? sv_c[((size_t)(b0 + b) * T + tp) * (2 * H) + dir * H + j] : 0.f;
        const float dh = dout[row * (2 * H) + dir * H + j] + dh_s[b][j];
        d = lstm_cell_bwd(ig, fg, gg, og, cp, tanhf(cc), dh, dc_s[b][j]);
        dc_s[b][j] = d.dc_prev;
        float* o = dgates + row * (2 * G4) + dir * G4;
        o[j] = d.dai; o[H + j] = d.daf; o[2 * H + j] = d.dag; o[3 * H + j] = d.dao;
      }
      dg_s[b][j] = d.dai; dg_s[b][H + j] = d.daf; dg_s[b][2 * H + j] = d.dag; dg_s[b][3 * H + j] = d.dao;
    }
    __syncthreads();
    {
      const int q = tid >> 8, k = tid & 255;
      float acc[LSTM_RB];
#pragma unroll
      for (int b = 0; b < LSTM_RB; ++b) acc[b] = 0.f;
      const int r0 = q * 256;
#pragma unroll 8
      for (int r = r0; r < r0 + 256; ++r) {
        const float w = W[(size_t)r * H + k];
#pragma unroll
        for (int b = 0; b < LSTM_RB; ++b) acc[b] = fmaf(dg_s[b][r], w, acc[b]);
      }
#pragma unroll
      for (int b = 0; b < LSTM_RB; ++b) part_s[q][b][k] = acc[b];
    }
    __syncthreads();
    (&dh_s[0][0])[tid] = sum_parts4_paired(&part_s[0][0][0], LSTM_RB * 256, tid);  // thread = (row, hidden unit) again
    __syncthreads();
  }
}
hipError_t launch_bilstm_train_bwd(const float* dout, const float* sv_gates, const float* sv_c, const float* whh_fwd,
                                   const float* whh_rev, float* dgates, int B, int T, int H, hipStream_t s) {
  if (H != 256 || B < 1 || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bilstm_train_bwd_kernel, dim3(2, (B + LSTM_RB - 1) / LSTM_RB), dim3(1024), 0, s, dout, sv_gates, sv_c, whh_fwd,
                     whh_rev, dgates, B, T, H);
  return hipGetLastError();
}
__global__ void bilstm_hprev_kernel(const float* __restrict__ out, float* __restrict__ hf, float* __restrict__ hr, int B, int T,
                                    int H) {
  const size_t total = (size_t)B * T * H;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % H), t = (int)((i / H) % T);
    const size_t b = i / ((size_t)H * T);
    hf[i] = t > 0 ? out[((b * T + t - 1) * 2) * H + j] : 0.f;
    hr[i] = t + 1 < T ? out[((b * T + t + 1) * 2 + 1) * H + j] : 0.f;
  }
}
hipError_t launch_bilstm_hprev(const float* out, float* hprev_fwd, float* hprev_rev, int B, int T, int H, hipStream_t s) {
  const size_t total = (size_t)B * T * H;  // four elements per thread of the grid-stride loop, as train_kernels.hip's movers
  const unsigned blocks = (unsigned)std::min<size_t>(((total + 3) / 4 + 255) / 256, 65535u * 16u);
  hipLaunchKernelGGL(bilstm_hprev_kernel, dim3(blocks), dim3(256), 0, s, out, hprev_fwd, hprev_rev, B, T, H);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Backward of the teacher-forced LSTM-attention loop (Attention / AttentionV2.forward_greedy with is_train,
// teacher_forcing = 1, coverage or location-aware memory): one block per batch row walks the steps in reverse.
// H = D = E = 256.  See AttnTrainBwdP for what is produced.
// ---------------------------------------------------------------------------
// dgate (1 x ROWS, in LDS) times ROWS rows of a row-major weight matrix with leading dimension LD, for the four consecutive
// columns w points at (16-byte loads), one fmaf per row in row order.
template <int ROWS, int LD>
__device__ __forceinline__ float4 dgate_rows_product(const float* __restrict__ w, const float* dgate_s) {
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
  for (int r = 0; r < ROWS; ++r) {
    const float4 w4 = *reinterpret_cast<const float4*>(w + (size_t)r * LD);
    const float g = dgate_s[r];
    a.x = fmaf(g, w4.x, a.x); a.y = fmaf(g, w4.y, a.y); a.z = fmaf(g, w4.z, a.z); a.w = fmaf(g, w4.w, a.w);
  }
  return a;
}

__global__ __launch_bounds__(1024) void attn_train_lstm_bwd_kernel(const AttnTrainBwdP p) {
  constexpr int H = 256;
  __shared__ float dh_s[H], dc_s[H], dgate_s[4 * H], dctx_s[H], dhprev_s[H], hq_s[H], dhq_s[H];
  __shared__ float alpha_s[AD_MAXT], mem_s[AD_MAXT + 16], dal_s[AD_MAXT], de_s[AD_MAXT], dcov_s[AD_MAXT], dmem_s[AD_MAXT + 16];
  __shared__ __attribute__((aligned(16))) float part_s[16][H];
  __shared__ float dl_s[1024], red_s[32];
  __shared__ __attribute__((aligned(16))) float wloc_s[11 * H];  // [tap][n]
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int Tk = p.T - p.key_off, half = p.taps / 2;
  const float* keys = p.mem + ((size_t)b * p.T + p.key_off) * p.D;
  const float* kp = p.kp + ((size_t)b * p.T + p.key_off) * H;
  float* dkeys = p.dmem + ((size_t)b * p.T + p.key_off) * p.D;
  float* dkp = p.dkp + ((size_t)b * p.T + p.key_off) * H;
  float* parts = &part_s[0][0];
  for (int i = tid; i < p.taps * H; i += 1024) wloc_s[i] = p.wloc[(i % H) * p.taps + i / H];
  if (tid < H) { dh_s[tid] = 0.f; dc_s[tid] = 0.f; }
  for (int i = tid; i < AD_MAXT; i += 1024) { dcov_s[i] = 0.f; mem_s[i] = 0.f; dmem_s[i] = 0.f; }
  if (tid < 16) { mem_s[AD_MAXT + tid] = 0.f; dmem_s[AD_MAXT + tid] = 0.f; }
  __syncthreads();
  // memory after the last step = sum of all alignments (coverage) / the last alignment (location-aware)
  for (int t = 0; t < p.S; ++t)
    for (int j = tid; j < Tk; j += 1024) {
      const float a = p.sv_alpha[((size_t)b * p.S + t) * Tk + j];
      mem_s[j] = p.coverage ? mem_s[j] + a : a;
    }
  // persistent per-lane accumulators over all steps (lane -> channels n0..n0+3 of the score layer)
  const int n0 = lane * 4;
  float acc_ws[4] = {0, 0, 0, 0}, acc_bl[4] = {0, 0, 0, 0}, acc_wl[11][4];
#pragma unroll
  for (int a = 0; a < 11; ++a)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc_wl[a][k] = 0.f;
  float acc_bs = 0.f;
  __syncthreads();

  for (int t = p.S - 1; t >= 0; --t) {
    const size_t bt = (size_t)b * p.S + t;
    // A. this step's alignment; memory BEFORE the step
    for (int j = tid; j < Tk; j += 1024) {
      const float a = p.sv_alpha[bt * Tk + j];
      alpha_s[j] = a;
      if (p.coverage) mem_s[j] -= a;
      else mem_s[j] = t > 0 ? p.sv_alpha[(bt - 1) * Tk + j] : 0.f;
    }
    if (tid < p.V) dl_s[tid] = p.dlogits[bt * p.V + tid];
    if (tid < H) hq_s[tid] = p.sv_hq[bt * H + tid];
    __syncthreads();
    // B. dh += generator^T dlogits   (4 threads per hidden unit)
    // (p.dhl: that product for every (row, step) from one GEMM before this kernel -- it does not depend on the recurrence,
    // and inside the loop it cost half a megabyte of generator weights per row and step)
    if (p.dhl) {
      if (tid < H) dh_s[tid] += p.dhl[bt * H + tid];
    } else if (!(p.probe & 1)) {
      const int n = tid >> 2, q = tid & 3;
      float a = 0.f;
      for (int v = q; v < p.V; v += 4) a = fmaf(dl_s[v], p.wg_t[(size_t)n * p.V + v], a);
      a += __shfl_xor(a, 1, 64);
      a += __shfl_xor(a, 2, 64);
      if (q == 0) dh_s[n] += a;
    }
    __syncthreads();
    // C. LSTMCell backward
    if (tid < H) {
      const float* gs = p.sv_gates + bt * 4 * H;
      const LstmCellGrad d = lstm_cell_bwd(gs[tid], gs[H + tid], gs[2 * H + tid], gs[3 * H + tid], p.sv_cprev[bt * H + tid],
                                           tanhf(p.sv_cafter[bt * H + tid]), dh_s[tid], dc_s[tid]);
      dgate_s[tid] = d.dai; dgate_s[H + tid] = d.daf; dgate_s[2 * H + tid] = d.dag; dgate_s[3 * H + tid] = d.dao;
      float* dg = p.dgates + bt * 4 * H;
      dg[tid] = d.dai; dg[H + tid] = d.daf; dg[2 * H + tid] = d.dag; dg[3 * H + tid] = d.dao;
      dc_s[tid] = d.dc_prev;
    }
    __syncthreads();
    // D. gradient of the LSTMCell input and of h_prev: dgates (1 x 4H) times W_ih (4H x 2H: context | embedding columns)
    // and W_hh (4H x H).  All 1024 threads take part: a thread owns four consecutive columns (16-byte loads) and one
    // part of the 4H rows, the parts are added through LDS in a fixed order.  The embedding half is not part of the
    // recurrence: when p.demb is null the caller computes it for all (row, step) with one GEMM on the saved dgates, and
    // only the context half (1 MB of the 2 MB of W_ih) is streamed here.  The phase is bound by the CU's L2 ingest.
    if (!(p.probe & 2)) {
      if (p.demb) {
        const int cg = tid & 127, rp = tid >> 7;  // 128 column groups x 8 row parts of 128 rows; part_s as [8][2H]
        *reinterpret_cast<float4*>(parts + rp * 2 * H + cg * 4) =
            dgate_rows_product<128, 2 * H>(p.wih_raw + (size_t)(rp * 128) * 2 * H + cg * 4, dgate_s + rp * 128);
      } else {
        const int cg = tid & 63, rp = tid >> 6;  // context columns only: 64 column groups x 16 row parts of 64 rows
        *reinterpret_cast<float4*>(&part_s[rp][cg * 4]) =
            dgate_rows_product<64, 2 * H>(p.wih_raw + (size_t)(rp * 64) * 2 * H + cg * 4, dgate_s + rp * 64);
      }
    }
    __syncthreads();
    if (p.demb) {
      if (tid < 2 * H) {
        const float a = sum_parts<8>(parts, 2 * H, tid);
        if (tid < H) dctx_s[tid] = a;
        else p.demb[bt * p.E + (tid - H)] = a;
      }
    } else if (tid < H) {
      dctx_s[tid] = sum_parts<16>(parts, H, tid);
    }
    __syncthreads();
    if (!(p.probe & 2)) {
      const int cg = tid & 63, rp = tid >> 6;  // W_hh: 64 column groups x 16 row parts of 64 rows
      *reinterpret_cast<float4*>(&part_s[rp][cg * 4]) =
          dgate_rows_product<64, H>(p.whh_raw + (size_t)(rp * 64) * H + cg * 4, dgate_s + rp * 64);
    }
    __syncthreads();
    if (tid < H) dhprev_s[tid] = sum_parts<16>(parts, H, tid);
    __syncthreads();
    // E. context backward: dalpha_j = dctx . key_j ; dkeys_j += alpha_j * dctx   (wave per key)
    if (!(p.probe & 4)) {
      const float4 dc4 = *reinterpret_cast<const float4*>(dctx_s + n0);
      for (int j = wave; j < Tk; j += 16) {
        const float4 k4 = *reinterpret_cast<const float4*>(keys + (size_t)j * p.D + n0);
        const float e = wsum(dc4.x * k4.x + dc4.y * k4.y + dc4.z * k4.z + dc4.w * k4.w);
        if (lane == 0) dal_s[j] = e;
        const float a = alpha_s[j];
        float4* dk = reinterpret_cast<float4*>(dkeys + (size_t)j * p.D + n0);
        float4 v = *dk;
        v.x = fmaf(a, dc4.x, v.x); v.y = fmaf(a, dc4.y, v.y); v.z = fmaf(a, dc4.z, v.z); v.w = fmaf(a, dc4.w, v.w);
        *dk = v;
      }
    }
    __syncthreads();
    // F. softmax backward (with the coverage gradient of later steps)
    {
      float s = 0.f;
      for (int j = tid; j < Tk; j += 1024) s = fmaf(alpha_s[j], dal_s[j] + dcov_s[j], s);
      const float tot = block_sum(s, red_s, wave, lane);
      for (int j = tid; j < Tk; j += 1024) {
        const float de = alpha_s[j] * (dal_s[j] + dcov_s[j] - tot);
        de_s[j] = de;
        acc_bs += de;
      }
    }
    __syncthreads();
    // G. score backward: u = key_proj_j + query + loc_j ; du = de_j * w * (1 - tanh(u)^2)   (wave per key)
    if (!(p.probe & 8)) {
      const float4 hq4 = *reinterpret_cast<const float4*>(hq_s + n0);
      const float4 ws4 = *reinterpret_cast<const float4*>(p.wscore + n0);
      const float4 bl4 = *reinterpret_cast<const float4*>(p.bloc + n0);
      float dq[4] = {0, 0, 0, 0};
      for (int j = wave; j < Tk; j += 16) {
        const float4 k4 = *reinterpret_cast<const float4*>(kp + (size_t)j * H + n0);
        const float4 lc = loc_term(mem_s, wloc_s, bl4, j, p.taps, half, Tk, n0);
        const float th[4] = {tanhf(k4.x + hq4.x + lc.x), tanhf(k4.y + hq4.y + lc.y), tanhf(k4.z + hq4.z + lc.z),
                             tanhf(k4.w + hq4.w + lc.w)};
        const float w4[4] = {ws4.x, ws4.y, ws4.z, ws4.w};
        const float de = de_s[j];
        float du[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          du[k] = de * w4[k] * (1.f - th[k] * th[k]);
          dq[k] += du[k];
          acc_ws[k] = fmaf(de, th[k], acc_ws[k]);
        }
        float4* dkp4 = reinterpret_cast<float4*>(dkp + (size_t)j * H + n0);
        float4 v = *dkp4;
        v.x += du[0]; v.y += du[1]; v.z += du[2]; v.w += du[3];
        *dkp4 = v;
        // the location term's backward: into the filter (per-lane accumulators) and into the memory around j
        for (int a = 0; a < p.taps; ++a) {
          const int tt = j + a - half;
          const bool in = tt >= 0 && tt < Tk;
          const float m = in ? mem_s[tt] : 0.f;
          const float4 wl = *reinterpret_cast<const float4*>(wloc_s + a * H + n0);
          float g = du[0] * wl.x + du[1] * wl.y + du[2] * wl.z + du[3] * wl.w;
#pragma unroll
          for (int k = 0; k < 4; ++k) acc_wl[a][k] = fmaf(du[k], m, acc_wl[a][k]);
          g = wsum(g);
          if (lane == 0 && in) atomicAdd(&dmem_s[tt], g);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) { part_s[wave][n0 + k] = dq[k]; acc_bl[k] += dq[k]; }
    }
    __syncthreads();
    if (tid < H) {
      const float a = sum_parts<16>(parts, H, tid);
      dhq_s[tid] = a;
      p.dhq[bt * H + tid] = a;
    }
    __syncthreads();
    // H. query projection backward into h_prev; I. coverage recursion; J. hand the state gradients to step t-1
    if (tid < H) {
      float a = dhprev_s[tid];
#pragma unroll 8
      for (int n = 0; n < H && !(p.probe & 16); ++n) a = fmaf(dhq_s[n], p.wq_raw[(size_t)n * H + tid], a);
      dh_s[tid] = a;
    }
    for (int j = tid; j < Tk; j += 1024) {
      if (p.coverage) dcov_s[j] += dmem_s[j];
      else dcov_s[j] = dmem_s[j];  // location-aware: the memory of step t is the alignment of step t-1 only
      dmem_s[j] = 0.f;
    }
    __syncthreads();
  }
  if (tid < H) { p.dh0[(size_t)b * H + tid] = dh_s[tid]; p.dc0[(size_t)b * H + tid] = dc_s[tid]; }
  // per-row partial sums of the score / location layers: reduce the 16 waves' lane accumulators through LDS;
  // channel n goes to dst[n * stride]
  auto reduce_store = [&](float (&v)[4], float* dst, int stride) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) part_s[wave][n0 + k] = v[k];
    __syncthreads();
    if (tid < H) dst[(size_t)tid * stride] = sum_parts<16>(parts, H, tid);
  };
  reduce_store(acc_ws, p.dwscore + (size_t)b * H, 1);
  reduce_store(acc_bl, p.dbloc + (size_t)b * H, 1);
  for (int a = 0; a < p.taps; ++a) reduce_store(acc_wl[a], p.dwloc + (size_t)b * H * p.taps + a, p.taps);
  __syncthreads();
  const float tot = block_sum(acc_bs, red_s, wave, lane);
  if (tid == 0) p.dbscore[b] = tot;
}
hipError_t launch_attn_train_lstm_bwd(const AttnTrainBwdP& p_in, hipStream_t s) {
  AttnTrainBwdP p = p_in;
  static const int probe = D2T_PROBE_ENV("D2T_LSTM_BWD_PROBE");
  p.probe = probe;
  // V > 1024 needs the dlogits . generator product from the caller (p.dhl); the in-kernel product stages 1024 classes
  if (p.H != 256 || p.D != 256 || p.E != 256 || p.V > D2T_ATTN_MAX_CLASSES || (p.V > 1024 && !p.dhl) ||
      p.T - p.key_off > AD_MAXT || p.T - p.key_off < 1 || p.taps > 11)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_train_lstm_bwd_kernel, dim3(p.B), dim3(1024), 0, s, p);
  return hipGetLastError();
}

// gradients of loc_conv.weight [kd][taps], loc_conv.bias [kd], loc_proj.weight [H][kd], loc_proj.bias [H] from the
// folded filter's: wloc[n][a] = sum_m Wp[n][m] Wc[m][a],  bloc[n] = bp[n] + sum_m Wp[n][m] bc[m]
__global__ void loc_unfold_bwd_kernel(const float* __restrict__ dwloc, const float* __restrict__ dbloc, int B,
                                      const float* __restrict__ cw, const float* __restrict__ cb,
                                      const float* __restrict__ pw, int H, int kd, int taps, float* d_cw, float* d_cb,
                                      float* d_pw, float* d_pb) {
  extern __shared__ float sm[];  // summed dwloc [H][taps] | dbloc [H]
  float* W = sm;
  float* Bv = sm + H * taps;
  for (int i = threadIdx.x; i < H * taps; i += blockDim.x) {
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dwloc[(size_t)b * H * taps + i];
    W[i] = a;
  }
  for (int i = threadIdx.x; i < H; i += blockDim.x) {
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dbloc[(size_t)b * H + i];
    Bv[i] = a;
    d_pb[i] = a;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H * kd; i += blockDim.x) {  // d_pw[n][m]
    const int n = i / kd, m = i % kd;
    float a = Bv[n] * cb[m];
    for (int t = 0; t < taps; ++t) a = fmaf(W[n * taps + t], cw[m * taps + t], a);
    d_pw[i] = a;
  }
  for (int i = threadIdx.x; i < kd * taps; i += blockDim.x) {  // d_cw[m][t]
    const int m = i / taps, t = i % taps;
    float a = 0.f;
    for (int n = 0; n < H; ++n) a = fmaf(W[n * taps + t], pw[n * kd + m], a);
    d_cw[i] = a;
  }
  for (int m = threadIdx.x; m < kd; m += blockDim.x) {
    float a = 0.f;
    for (int n = 0; n < H; ++n) a = fmaf(Bv[n], pw[n * kd + m], a);
    d_cb[m] = a;
  }
}
hipError_t launch_loc_unfold_bwd(const float* dwloc, const float* dbloc, int B, const float* conv_w, const float* conv_b,
                                 const float* proj_w, int H, int kd, int taps, float* d_conv_w, float* d_conv_b,
                                 float* d_proj_w, float* d_proj_b, hipStream_t s) {
  hipLaunchKernelGGL(loc_unfold_bwd_kernel, dim3(1), dim3(1024), (size_t)(H * taps + H) * 4, s, dwloc, dbloc, B, conv_w, conv_b,
                     proj_w, H, kd, taps, d_conv_w, d_conv_b, d_proj_w, d_proj_b);
  return hipGetLastError();
}
__global__ void sum_over_rows_kernel(const float* __restrict__ part, float* __restrict__ out, int B, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float a = 0.f;
  for (int b = 0; b < B; ++b) a += part[(size_t)b * C + c];
  out[c] = a;
}
hipError_t launch_sum_over_rows(const float* part, float* out, int B, int C, hipStream_t s) {
  hipLaunchKernelGGL(sum_over_rows_kernel, dim3((C + 127) / 128), dim3(128), 0, s, part, out, B, C);
  return hipGetLastError();
}

}  // namespace d2t
