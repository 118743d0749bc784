// Softmax attention of the training step (train.hip), fp32: forward saving the probabilities, backward, with causal and
// key-padding masks and the probability dropout of nn.MultiheadAttention (tfm.py:74-91).
//
// q/k/v/o are addressed as  base + (b*L + i)*ld + head*HD ; one block per (batch, head); K and V of the head live in LDS.
// probs [B][heads][Lq][Lk] is written for the backward pass, which overwrites it with dS.
// GKV (memories too long for a head's K and V to sit in LDS: crops beyond about 600 tokens, the shipped max_dimension [800, 800]
// gives 2526): the same loops read K / V rows from global memory (L2) -- slow, and the same sums in the same order.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "train_common.h"

namespace d2t {

// K and V of the block's (batch, head): staged in LDS as [Lk][HD + 1] and [Lk][VROW] at the start of sm (the caller's
// barrier makes them visible), or, GKV, left in global memory.  rows: the LDS behind them.
template <int HD, bool GKV, int VROW>
struct AttnHead {
  int b, hh;
  const float *Ks, *Vs;
  int ldk, ldv;  // GKV only
  float* rows;
  __device__ __forceinline__ AttnHead(const AttnTrainP& p, float* sm) {
    b = blockIdx.x / p.heads; hh = blockIdx.x % p.heads;
    ldk = p.ldk; ldv = p.ldv;
    if (GKV) {
      Ks = p.k + (size_t)b * p.Lk * p.ldk + hh * HD;
      Vs = p.v + (size_t)b * p.Lk * p.ldv + hh * HD;
      rows = sm;
    } else {
      float* ks = sm;
      float* vs = ks + (size_t)p.Lk * (HD + 1);
      rows = vs + (size_t)p.Lk * VROW;
      for (int i = threadIdx.x; i < p.Lk * HD; i += blockDim.x) {
        const int j = i / HD, c = i % HD;
        ks[j * (HD + 1) + c] = p.k[((size_t)b * p.Lk + j) * p.ldk + hh * HD + c];
        vs[j * VROW + c] = p.v[((size_t)b * p.Lk + j) * p.ldv + hh * HD + c];
      }
      Ks = ks; Vs = vs;
    }
  }
  // key j, channel c
  __device__ __forceinline__ float K(int j, int c) const { return Ks[(size_t)j * (GKV ? ldk : HD + 1) + c]; }
  __device__ __forceinline__ float V(int j, int c) const { return Vs[(size_t)j * (GKV ? ldv : VROW) + c]; }
  // row i of a [B*L][ld] tensor, this head's channels
  __device__ __forceinline__ size_t at(int L, int i, int ld) const { return ((size_t)b * L + i) * ld + hh * HD; }
  // this head's [Lq][Lk] matrix of probs / dropmask
  template <class T>
  __device__ __forceinline__ T* mat(T* base, const AttnTrainP& p) const { return base ? base + ((size_t)b * p.heads + hh) * p.Lq * p.Lk : nullptr; }
};

// out[c] = sum_{i < n} term(i, c) with a wave's lanes as (channel c = lane % HD, phase = lane / HD): a lane adds every
// (64 / HD)-th term through acc = term(acc, i, c), the phases are folded at the end; every lane of channel c returns the sum
template <int HD, class F>
__device__ __forceinline__ float lane_channel_reduce(int lane, int n, F term) {
  constexpr int PH = 64 / HD;
  const int c = lane % HD;
  float a = 0.f;
#pragma unroll 8
  for (int i = lane / HD; i < n; i += PH) a = term(a, i, c);
  if (PH == 2) a += __shfl_xor(a, 32, 64);
  return a;
}

template <int HD, bool GKV = false>
__global__ __launch_bounds__(1024) void attn_train_fwd_kernel(const AttnTrainP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const AttnHead<HD, GKV, HD> head(p, sm);
  if (!GKV) __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, NW = blockDim.x >> 6;
  const float scale = rsqrtf((float)HD);
  float* P = head.rows + (size_t)wave * p.Lk;  // [waves][Lk]
  float* probs = head.mat(p.probs, p);
  const uint8_t* dmask = head.mat(p.dropmask, p);
  for (int i = wave; i < p.Lq; i += NW) {
    const float* qp = p.q + head.at(p.Lq, i, p.ldq);
    float q[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) q[c] = qp[c];
    float mx = -INFINITY;
    for (int j = lane; j < p.Lk; j += 64) {
      bool ok = !(p.causal && j > i);
      if (ok && p.keytok) ok = p.keytok[(size_t)head.b * p.Lk + j] != p.pad_id;
      float a = -INFINITY;
      if (ok) {
        a = 0.f;
#pragma unroll
        for (int c = 0; c < HD; ++c) a = fmaf(q[c], head.K(j, c), a);
        a *= scale;
      }
      P[j] = a;
      mx = fmaxf(mx, a);
    }
    mx = wmax(mx);
    float sum = 0.f;
    for (int j = lane; j < p.Lk; j += 64) {
      const float e = P[j] == -INFINITY ? 0.f : expf(P[j] - mx);
      P[j] = e;
      sum += e;
    }
    sum = wsum(sum);
    const float inv = 1.f / sum;
    float* prow = probs + (size_t)i * p.Lk;
    const uint8_t* mrow = dmask ? dmask + (size_t)i * p.Lk : nullptr;
    for (int j = lane; j < p.Lk; j += 64) {
      const float w = P[j] * inv;
      prow[j] = w;                                            // saved: the softmax itself
      P[j] = mrow ? w * (mrow[j] ? p.dropscale : 0.f) : w;    // used: after dropout (nn.MultiheadAttention dropout)
    }
    // o[c] = sum_j P[j] * V[j][c]
    const float o = lane_channel_reduce<HD>(lane, p.Lk, [&](float a, int j, int c) { return fmaf(P[j], head.V(j, c), a); });
    if (lane < HD) p.o[head.at(p.Lq, i, p.ldo) + lane] = o;
  }
}

// Backward: dV = P^T dO;  dP = dO V^T;  dS = P * (dP - rowsum(dP * P));  dQ = scale * dS K;  dK = scale * dS^T Q.
// One block per (batch, head); dS overwrites the saved probabilities in place (phase 2), phases separated by
// block barriers.  p.o carries dO; p.dq / p.dk / p.dv use the q / k / v strides.
// (GKV: K / V rows from global memory, as in the forward kernel; any multiple of 64 threads)
template <int HD, bool GKV = false>
__global__ __launch_bounds__(1024) void attn_train_bwd_kernel(const AttnTrainP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const AttnHead<HD, GKV, HD + 1> head(p, sm);  // (visible after the barrier behind phase 1)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, NW = blockDim.x >> 6;
  float* probs = head.mat(p.probs, p);
  const uint8_t* dmask = head.mat(p.dropmask, p);
  // phase 1: dV[j][c] = sum_i (P o D)[i][j] * dO[i][c]   (wave per key; D = dropout keep mask * scale)
  for (int j = wave; j < p.Lk; j += NW) {
    const float a = lane_channel_reduce<HD>(lane, p.Lq, [&](float a, int i, int c) {
      float w = probs[(size_t)i * p.Lk + j];
      if (dmask) w *= dmask[(size_t)i * p.Lk + j] ? p.dropscale : 0.f;
      return fmaf(w, p.o[head.at(p.Lq, i, p.ldo) + c], a);
    });
    if (lane < HD) p.dv[head.at(p.Lk, j, p.ldv) + lane] = a;
  }
  __syncthreads();
  const float scale = rsqrtf((float)HD);
  // phase 2: per query row: dS, dQ (wave per query).  dP is computed twice rather than kept in the wave's D row as the fast
  // kernel does: one body for both cost this kernel 4 to 8 VGPRs (96 / 120 / 122 / 128 against 92 / 114 / 118 / 122)
  for (int i = wave; i < p.Lq; i += NW) {
    const float* dop = p.o + head.at(p.Lq, i, p.ldo);
    float d_o[HD];
#pragma unroll
    for (int cc = 0; cc < HD; ++cc) d_o[cc] = dop[cc];
    float* prow = probs + (size_t)i * p.Lk;
    const uint8_t* mrow = dmask ? dmask + (size_t)i * p.Lk : nullptr;
    float* D = head.rows + (size_t)wave * p.Lk;
    float dsum = 0.f;
    for (int j = lane; j < p.Lk; j += 64) {
      float dp = 0.f;
#pragma unroll
      for (int cc = 0; cc < HD; ++cc) dp = fmaf(d_o[cc], head.V(j, cc), dp);
      if (mrow) dp *= mrow[j] ? p.dropscale : 0.f;
      dsum = fmaf(dp, prow[j], dsum);
    }
    dsum = wsum(dsum);
    for (int j = lane; j < p.Lk; j += 64) {
      float dp = 0.f;
#pragma unroll
      for (int cc = 0; cc < HD; ++cc) dp = fmaf(d_o[cc], head.V(j, cc), dp);
      if (mrow) dp *= mrow[j] ? p.dropscale : 0.f;
      const float ds = prow[j] * (dp - dsum);
      prow[j] = ds;
      D[j] = ds;
    }
    const float a = lane_channel_reduce<HD>(lane, p.Lk, [&](float a, int j, int c) { return fmaf(D[j], head.K(j, c), a); });
    if (lane < HD) p.dq[head.at(p.Lq, i, p.ldq) + lane] = a * scale;
  }
  __syncthreads();
  // phase 3: dK[j][c] = scale * sum_i dS[i][j] * Q[i][c]   (wave per key)
  for (int j = wave; j < p.Lk; j += NW) {
    const float a = lane_channel_reduce<HD>(
        lane, p.Lq, [&](float a, int i, int c) { return fmaf(probs[(size_t)i * p.Lk + j], p.q[head.at(p.Lq, i, p.ldq) + c], a); });
    if (lane < HD) p.dk[head.at(p.Lk, j, p.ldk) + lane] = a * scale;
  }
}
// Same mathematics with coalesced accesses: dO and Q of the head are staged in LDS too, and the two column-wise
// reductions (dV over queries with P, dK over queries with dS) run with lane = key (consecutive lanes read consecutive
// probabilities of one query row) and wave = group of HD/4 channels.  Needs (2*Lk*(HD+1) + 2*Lq*HD + 4*Lk) floats of LDS.
// (written out rather than built on AttnHead and lane_channel_reduce: on them this kernel spilled less but ran 18 % longer
// at B = 32, 261 tokens -- 209 against 177 us)
template <int HD>
__global__ __launch_bounds__(1024) void attn_train_bwd_fast_kernel(const AttnTrainP p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Ks = sm;                             // [Lk][HD+1]
  float* Vs = Ks + (size_t)p.Lk * (HD + 1);   // [Lk][HD+1]
  float* dOs = Vs + (size_t)p.Lk * (HD + 1);  // [Lq][HD]
  float* Qs = dOs + (size_t)p.Lq * HD;        // [Lq][HD]
  float* Ds = Qs + (size_t)p.Lq * HD;         // [waves][Lk]
  const int b = blockIdx.x / p.heads, hh = blockIdx.x % p.heads;
  // a multiple of four waves: wave & 3 = channel group of the column reductions, wave >> 2 = which 64-key blocks it takes
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, NT = blockDim.x, NW = NT >> 6;
  const int cgrp = wave & 3, kgrp = wave >> 2, nkg = NW >> 2;
  for (int i = tid; i < p.Lk * HD; i += NT) {
    const int j = i / HD, c = i % HD;
    Ks[j * (HD + 1) + c] = p.k[((size_t)b * p.Lk + j) * p.ldk + hh * HD + c];
    Vs[j * (HD + 1) + c] = p.v[((size_t)b * p.Lk + j) * p.ldv + hh * HD + c];
  }
  for (int i = tid; i < p.Lq * HD; i += NT) {
    const int r = i / HD, c = i % HD;
    dOs[i] = p.o[((size_t)b * p.Lq + r) * p.ldo + hh * HD + c];
    Qs[i] = p.q[((size_t)b * p.Lq + r) * p.ldq + hh * HD + c];
  }
  __syncthreads();
  float* probs = p.probs + ((size_t)b * p.heads + hh) * p.Lq * p.Lk;
  constexpr int CG = HD / 4;  // channels per wave
  // column reduction out[j][c] = alpha * sum_i M[i][j] * R[i][c]
  const uint8_t* dmask = p.dropmask ? p.dropmask + ((size_t)b * p.heads + hh) * p.Lq * p.Lk : nullptr;
  auto colred = [&](const float* R, float* out, int ld, float alpha, const uint8_t* dm) {
    for (int j0 = kgrp * 64; j0 < p.Lk; j0 += 64 * nkg) {
      const int j = j0 + lane;
      float acc[CG];
#pragma unroll
      for (int c = 0; c < CG; ++c) acc[c] = 0.f;
      if (j < p.Lk) {
#pragma unroll 8
        for (int i = 0; i < p.Lq; ++i) {
          float m = probs[(size_t)i * p.Lk + j];
          if (dm) m *= dm[(size_t)i * p.Lk + j] ? p.dropscale : 0.f;
          const float* r = R + i * HD + cgrp * CG;
#pragma unroll
          for (int c = 0; c < CG; ++c) acc[c] = fmaf(m, r[c], acc[c]);
        }
        float* o = out + ((size_t)b * p.Lk + j) * ld + hh * HD + cgrp * CG;
#pragma unroll
        for (int c = 0; c < CG; ++c) o[c] = acc[c] * alpha;
      }
    }
  };
  if (!(p.probe & 1)) colred(dOs, p.dv, p.ldv, 1.f, dmask);  // phase 1: dV = (P o D)^T dO
  __syncthreads();
  const float scale = rsqrtf((float)HD);
  constexpr int PH = 64 / HD;
  const int c = lane % HD, ph = lane / HD;
  for (int i = wave; i < p.Lq && !(p.probe & 2); i += NW) {  // phase 2: dS (in place) and dQ, one wave per query row
    const float* d_o = dOs + i * HD;
    float* prow = probs + (size_t)i * p.Lk;
    float dsum = 0.f;
    for (int j = lane; j < p.Lk; j += 64) {
      float dp = 0.f;
#pragma unroll
      for (int cc = 0; cc < HD; ++cc) dp = fmaf(d_o[cc], Vs[j * (HD + 1) + cc], dp);
      if (dmask) dp *= dmask[(size_t)i * p.Lk + j] ? p.dropscale : 0.f;
      Ds[wave * p.Lk + j] = dp;
      dsum = fmaf(dp, prow[j], dsum);
    }
    dsum = wsum(dsum);
    for (int j = lane; j < p.Lk; j += 64) {
      const float ds = prow[j] * (Ds[wave * p.Lk + j] - dsum);
      prow[j] = ds;
      Ds[wave * p.Lk + j] = ds;
    }
    float a = 0.f;
#pragma unroll 8
    for (int j = ph; j < p.Lk; j += PH) a = fmaf(Ds[wave * p.Lk + j], Ks[j * (HD + 1) + c], a);
    if (PH == 2) a += __shfl_xor(a, 32, 64);
    if (lane < HD) p.dq[((size_t)b * p.Lq + i) * p.ldq + hh * HD + c] = a * scale;
  }
  __syncthreads();
  if (!(p.probe & 4)) colred(Qs, p.dk, p.ldk, scale, nullptr);  // phase 3: dK = scale * dS^T Q
}

// ---------------------------------------------------------------------------
// Launchers.  A block may take 160 KB of LDS.
// ---------------------------------------------------------------------------
constexpr size_t ATTN_LDS = 160 * 1024;
template <class K>
static hipError_t launch_attn(K kernel, int waves, size_t lds, const AttnTrainP& p, hipStream_t s) {
  if (lds > ATTN_LDS) return hipErrorInvalidValue;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_LDS);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(p.B * p.heads), dim3(waves * 64), lds, s, p);
  return hipGetLastError();
}
// f(std::integral_constant<int, hd>) for the head sizes the kernels are built for
template <class F>
static hipError_t attn_for_hd(int hd, F f) {
  if (hd == 32) return f(std::integral_constant<int, 32>{});
  if (hd == 64) return f(std::integral_constant<int, 64>{});
  return hipErrorInvalidValue;
}
// One block per (batch, head) leaves a CU with a single block; sixteen waves in it (four per SIMD) hide the latency of the
// per-query loops that four could not (forward 382 -> ~130 us, backward 656 -> ~250 us at B = 32, 261 tokens).  Fewer when
// the per-wave LDS rows do not fit.
static int attn_waves(size_t base_bytes, int Lk) {
  for (int nw = 16; nw > 4; nw -= 4)
    if (base_bytes + (size_t)nw * Lk * 4 <= ATTN_LDS) return nw;
  return 4;
}
// waves of the global-K/V forms: as many per-wave rows of Lk floats as fit (a multiple of four, at most sixteen)
static int attn_waves_gkv(int Lk) {
  int nw = (int)(ATTN_LDS / ((size_t)Lk * 4)) & ~3;
  return nw > 16 ? 16 : nw;
}
AttnTrainPlan attn_train_plan(int hd, int Lq, int Lk) {
  AttnTrainPlan pl{};
  if ((hd != 32 && hd != 64) || Lq < 1 || Lk < 1) return pl;
  const int nwg = attn_waves_gkv(Lk);
  const size_t lds_gkv = (size_t)nwg * Lk * 4;
  const size_t base = ((size_t)Lk * (hd + 1) + (size_t)Lk * hd) * 4;
  if (base + (size_t)4 * Lk * 4 > ATTN_LDS) {  // K and V of a head do not fit in LDS beside four score rows
    pl.fwd_form = ATTN_FWD_GKV;
    if (nwg >= 4) { pl.fwd_waves = nwg; pl.fwd_lds = lds_gkv; }
  } else {
    pl.fwd_form = ATTN_FWD_LDS;
    pl.fwd_waves = attn_waves(base, Lk);
    pl.fwd_lds = base + (size_t)pl.fwd_waves * Lk * 4;
  }
  const size_t lds = ((size_t)2 * Lk * (hd + 1) + 4 * (size_t)Lk) * 4;
  const size_t base_fast = ((size_t)2 * Lk * (hd + 1) + (size_t)2 * Lq * hd) * 4;
  const int nw = attn_waves(base_fast, Lk);
  const size_t lds_fast = base_fast + (size_t)nw * Lk * 4;
  if (lds_fast <= ATTN_LDS) {
    pl.bwd_form = ATTN_BWD_FAST; pl.bwd_waves = nw; pl.bwd_lds = lds_fast;
  } else if (lds > ATTN_LDS) {  // K and V of a head do not fit in LDS: rows from global memory
    pl.bwd_form = ATTN_BWD_GKV;
    if (nwg >= 4) { pl.bwd_waves = nwg; pl.bwd_lds = lds_gkv; }
  } else {
    pl.bwd_form = ATTN_BWD_PLAIN; pl.bwd_waves = 4; pl.bwd_lds = lds;
  }
  return pl;
}
hipError_t launch_attn_train_fwd(const AttnTrainP& p, hipStream_t s) {
  const AttnTrainPlan pl = attn_train_plan(p.hd, p.Lq, p.Lk);
  if (!pl.fwd_waves) return hipErrorInvalidValue;
  return attn_for_hd(p.hd, [&](auto hd) {
    constexpr int HD = decltype(hd)::value;
    if (pl.fwd_form == ATTN_FWD_GKV) return launch_attn(attn_train_fwd_kernel<HD, true>, pl.fwd_waves, pl.fwd_lds, p, s);
    return launch_attn(attn_train_fwd_kernel<HD, false>, pl.fwd_waves, pl.fwd_lds, p, s);
  });
}
hipError_t launch_attn_train_bwd(const AttnTrainP& p_in, hipStream_t s) {
  AttnTrainP p = p_in;
  static const int probe = D2T_PROBE_ENV("D2T_ATTN_BWD_PROBE");  // timing probe: skip phases (bit mask)
  p.probe = probe;
  const AttnTrainPlan pl = attn_train_plan(p.hd, p.Lq, p.Lk);
  if (!pl.bwd_waves) return hipErrorInvalidValue;
  return attn_for_hd(p.hd, [&](auto hd) {
    constexpr int HD = decltype(hd)::value;
    if (pl.bwd_form == ATTN_BWD_FAST) return launch_attn(attn_train_bwd_fast_kernel<HD>, pl.bwd_waves, pl.bwd_lds, p, s);
    if (pl.bwd_form == ATTN_BWD_GKV) return launch_attn(attn_train_bwd_kernel<HD, true>, pl.bwd_waves, pl.bwd_lds, p, s);
    return launch_attn(attn_train_bwd_kernel<HD, false>, pl.bwd_waves, pl.bwd_lds, p, s);
  });
}

}  // namespace d2t
