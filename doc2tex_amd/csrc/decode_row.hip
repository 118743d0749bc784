// The per-row decoder kernels of the decode step (gfx950, fp32): a layer's row work in one launch, the cross-attention over
// the projected K / V or, absorbed, over the encoder memory itself.  (The beam search's per-sample cross-attention between
// the MODE 1 / 2 builds is decode_beam.hip's.)
#include "decode_row_common.h"

namespace d2t {

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

// one beam step of a layer's row work: pre (per hypothesis) -> cross (per sample) -> post (per hypothesis).
// seg / nsamples: the samples' row segments (batched beam), or nullptr / 1 for a single sample whose rows are [0, r.M).
hipError_t launch_decoder_row_beam(const DecRowP& r, const float* mem, long long mem_stride, const float* wk, const float* wv_t,
                                   const float* bv, float* qp, float* x1, const int* seg, int nsamples, hipStream_t s) {
  if (r.heads != 8 || r.D != 256 || r.T < 1 || !qp || !x1 || nsamples < 1) return hipErrorInvalidValue;
  DecRow2P q{r, mem, mem_stride, wk, wv_t, bv, qp, x1, nullptr, nullptr};
  hipLaunchKernelGGL((decoder_row_absorbed_kernel<256, 1>), dim3(r.M), dim3(256), 0, s, q);
  BeamCrossP c{mem, mem_stride, r.T, qp, seg, r.M, r.step_ptr, r.stop_at};
  launch_beam_cross(c, nsamples, s);
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

// ---------------------------------------------------------------------------------------------------------------------
// decoder_row_kernel (one wave per head) that also hands out the row's cross-attention query: q2 goes to q2_out [M][D], where
// cross_attn_probs_kernel (decode_maps.hip) reads it.  Launched only by the teacher-forced replay behind
// d2t_decode_cross_attention.  The same phases in the same order; its own kernel and not a build of decoder_row_kernel so
// that the decode's kernels stay what they are, instruction for instruction.
// ---------------------------------------------------------------------------------------------------------------------
template <int D, int HD>
__global__ __launch_bounds__(512, 2) void decoder_row_maps_kernel(const DecRowP p, float* __restrict__ q2_out) {
  constexpr int NTH = 512, G = NTH / (D / 4);
  ROW_KERNEL_ENTRY(p, false);
  __shared__ __attribute__((aligned(16))) float a_s[D], y_s[D], x1_s[D], q2_s[D], part_s[G * D];
  const int tid = threadIdx.x, head = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int t = *p.step_ptr;
  row_self_attention<D, HD>(p, b, head, t, lane, a_s + head * HD);
  __syncthreads();
  row_gemv<D, NTH>(a_s, p.wo_t, part_s, tid);
  __syncthreads();
  if (tid < D) y_s[tid] = sum_parts<G, D>(part_s, tid, p.bo[tid] + p.xres[(size_t)b * D + tid]);
  __syncthreads();
  if (head == 0) row_ln1<D>(y_s, x1_s, lane, p);
  __syncthreads();
  row_gemv<D, NTH>(x1_s, p.wq_t, part_s, tid);
  __syncthreads();
  if (tid < D) {
    const float q = sum_parts<G, D>(part_s, tid, p.bq[tid]);
    q2_s[tid] = q;
    q2_out[(size_t)b * D + tid] = q;
  }
  __syncthreads();
  {
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

hipError_t launch_decoder_row_maps(const DecRowP& p, float* q2_out, hipStream_t s) {
  if (p.heads != 8 || !q2_out || p.anc || p.rows_ptr) return hipErrorInvalidValue;
  if (p.D == 256) hipLaunchKernelGGL((decoder_row_maps_kernel<256, 32>), dim3(p.M), dim3(512), 0, s, p, q2_out);
  else if (p.D == 512) hipLaunchKernelGGL((decoder_row_maps_kernel<512, 64>), dim3(p.M), dim3(512), 0, s, p, q2_out);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace d2t
