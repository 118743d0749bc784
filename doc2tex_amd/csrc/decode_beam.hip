// The beam search's device side (gfx950, fp32): the per-sample cross-attention of all live hypotheses, and the step's
// bookkeeping -- token embedding, top-k, cache gather, ancestry and the record of the device-resident loop.
#include "decode_row_common.h"

namespace d2t {

// ---------------------------------------------------------------------------------------------------------------------
// Beam search: ONE block per SAMPLE runs the cross-attention of all its live hypotheses (north_star's "K/V resident in LDS
// per wavefront", in the absorbed form: the sample's memory rows are staged in LDS ONCE per layer and step and serve every
// hypothesis and head; the reference repeats the memory per hypothesis, tfm.py:163, and the per-row kernel re-read it per
// hypothesis).  M <= 6 hypotheses x 8 heads = up to 48 query rows = three 16-row MFMA tiles (83 % filled at beam 5 against
// 50 % for a single row).  The four waves work through the key tiles TOGETHER: a ring of four 16 KB tile buffers with the
// LDS-DMA three tiles ahead; per tile wave w multiplies channel quarter w of the tile with the same slice of every q' row
// (the A fragment is read once for all row tiles), the partial score tiles are summed through LDS, each wave runs the online
// softmax of all rows and accumulates channel quarter w of the weighted memory rows.  (For ONE row this cooperative form
// lost to independent waves -- two block barriers per tile; with three row tiles per barrier pair it is the better split,
// and it needs no merge.)  In: q.qp = absorbed queries [rows][8][256] (from decoder_row_absorbed_kernel MODE 1); out: the
// normalised context rows in their place.
__global__ __launch_bounds__(256, 1) void beam_cross_kernel(const BeamCrossP p) {
  if (p.stop_at && *p.stop_at && *p.step_ptr >= *p.stop_at) return;
  constexpr int NR = 3, D = 256;
  int off = 0, M = p.M;
  if (p.seg) { off = p.seg[blockIdx.x * 3]; M = p.seg[blockIdx.x * 3 + 1]; }
  if (M <= 0) return;  // block-uniform (a finished sample)
  decode_wave_priority();
  __shared__ __attribute__((aligned(1024))) unsigned char stage[4 * 16384];
  __shared__ __attribute__((aligned(1024))) float qp_s[NR * 16 * D];
  __shared__ __attribute__((aligned(16))) float part[4 * 16 * NR * 16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, g = lane >> 4;
  const int R = 8 * M, nrt = (R + 15) >> 4;
  const float* mem = p.mem + (size_t)blockIdx.x * p.mem_stride;
  float* qrows = p.qp + (size_t)off * 8 * D;
  for (int idx = tid; idx < nrt * 16 * (D / 4); idx += 256) {  // q' rows, 16-byte chunks of row r XOR-ed with r & 15; rows >= R zero
    const int row = idx / (D / 4), c4 = idx % (D / 4);
    const float4 v = row < R ? *reinterpret_cast<const float4*>(qrows + (size_t)row * D + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(qp_s + row * D + ((c4 ^ (row & 15)) << 2)) = v;
  }
  float m_run[NR], l_run[NR];
  f32x4 acc[NR][4];
#pragma unroll
  for (int rt = 0; rt < NR; ++rt) {
    m_run[rt] = -INFINITY;
    l_run[rt] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[rt][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int T = p.T, ntiles = (T + 15) >> 4;
  auto issue = [&](int tile) {  // this wave's four rows of the tile: row i -> buffer + i * 1024, physical chunk c holds logical c ^ i
    unsigned char* buf = stage + (tile & 3) * 16384;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = wave * 4 + k;
      const int j = (tile << 4) + i < T ? (tile << 4) + i : T - 1;  // rows past the end: a valid row, its probability is forced to zero
      __builtin_amdgcn_global_load_lds(mem + (size_t)j * D + ((lane ^ i) << 2), (lds_ptr_dec)(buf + i * 1024), 16, 0, 0);
    }
  };
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the q' loads above are done: from here on vmcnt counts tile pieces only
  issue(0);
  if (ntiles > 1) issue(1);
  if (ntiles > 2) issue(2);
  for (int tile = 0; tile < ntiles; ++tile) {
    const int j0 = tile << 4;
    const int ahead = ntiles - 1 - tile;  // block-uniform
    if (ahead >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // the tile has landed for everyone (and, at tile 0, the q' rows are in LDS); nobody reads tile - 1 any more
    if (tile + 3 < ntiles) issue(tile + 3);
    const unsigned char* buf = stage + (tile & 3) * 16384;
    // ---- partial S^T[key = 4g' + reg][row = 16 rt + col] over this wave's channel quarter ----
    f32x4 sacc[NR];
#pragma unroll
    for (int rt = 0; rt < NR; ++rt) sacc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
      const int u = wave * 4 + uu;
      const float4 a4 = *reinterpret_cast<const float4*>(buf + col * 1024 + (((4 * u + g) ^ col) << 4));
#pragma unroll
      for (int rt = 0; rt < NR; ++rt) {
        if (rt < nrt) {
          const float4 q4 = *reinterpret_cast<const float4*>(reinterpret_cast<const unsigned char*>(qp_s) + (rt * 16 + col) * 1024 +
                                                              (((4 * u + g) ^ col) << 4));
          sacc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, q4.x, sacc[rt], 0, 0, 0);
          sacc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, q4.y, sacc[rt], 0, 0, 0);
          sacc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, q4.z, sacc[rt], 0, 0, 0);
          sacc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, q4.w, sacc[rt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int rt = 0; rt < NR; ++rt)
      if (rt < nrt) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) part[(wave * 16 + 4 * g + reg) * (NR * 16) + rt * 16 + col] = sacc[rt][reg];
      }
    __syncthreads();
    // ---- online softmax of every row (all waves, identically): this lane holds keys j0 + 4g + reg of row 16 rt + col ----
    float pv[NR][4];
#pragma unroll
    for (int rt = 0; rt < NR; ++rt) {
      if (rt < nrt) {
        f32x4 sc;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int o = (4 * g + reg) * (NR * 16) + rt * 16 + col;
          sc[reg] = (part[o] + part[16 * NR * 16 + o]) + (part[2 * 16 * NR * 16 + o] + part[3 * 16 * NR * 16 + o]);
        }
        float ar[4];  // the accumulators hold ctx[row 16 rt + 4g + reg]: lane 4g + reg has that row's alpha
        online_softmax_tile(sc, j0, g, T, m_run[rt], l_run[rt], pv[rt], ar);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[rt][e][reg] *= ar[reg];
      } else {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) pv[rt][reg] = 0.f;
      }
    }
    // ---- ctx[row][64 wave + 4 col + e] += sum_keys P[row][key] m[key][chan]; k-step sk <-> keys 4g + sk ----
#pragma unroll
    for (int sk = 0; sk < 4; ++sk) {
      const int key = 4 * g + sk;
      const float4 b4 = *reinterpret_cast<const float4*>(buf + key * 1024 + (((16 * wave + col) ^ key) << 4));
#pragma unroll
      for (int rt = 0; rt < NR; ++rt)
        if (rt < nrt) {
          acc[rt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[rt][sk], b4.x, acc[rt][0], 0, 0, 0);
          acc[rt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[rt][sk], b4.y, acc[rt][1], 0, 0, 0);
          acc[rt][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[rt][sk], b4.z, acc[rt][2], 0, 0, 0);
          acc[rt][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[rt][sk], b4.w, acc[rt][3], 0, 0, 0);
        }
    }
  }
  // ---- normalise and hand the context rows back in the queries' place ----
#pragma unroll
  for (int rt = 0; rt < NR; ++rt) {
    if (rt < nrt) {
      float l = l_run[rt];
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float inv = 1.f / __shfl(l, 4 * g + reg, 64);  // lane 4g + reg holds the denominator of row 16 rt + 4g + reg
        const int row = rt * 16 + 4 * g + reg;
        if (row < R)
          *reinterpret_cast<float4*>(qrows + (size_t)row * D + 64 * wave + 4 * col) =
              make_float4(acc[rt][0][reg] * inv, acc[rt][1][reg] * inv, acc[rt][2][reg] * inv, acc[rt][3][reg] * inv);
      }
    }
  }
}

void launch_beam_cross(const BeamCrossP& p, int nsamples, hipStream_t s) {
  hipLaunchKernelGGL(beam_cross_kernel, dim3(nsamples), dim3(256), 0, s, p);
}

// ---------------------------------------------------------------------------
// Beam search device side (reference: tfm.py:145-186 runs the model, tools/beam.py:68-105
// does log_softmax + flat top-k on the host).
// ---------------------------------------------------------------------------
__global__ void embed_tokens_kernel(const float* __restrict__ emb, const float* __restrict__ pe,
                                    const int64_t* __restrict__ tok, const int* __restrict__ step_ptr,
                                    float* __restrict__ x, int d, float sqrt_d, const int* __restrict__ rows_ptr,
                                    const int* __restrict__ stop) {
  const int b = blockIdx.x, t = *step_ptr;
  if ((rows_ptr && b >= *rows_ptr) || (stop && *stop && t >= *stop)) return;
  const int64_t tk = tok[b];
  for (int c = threadIdx.x; c < d; c += blockDim.x)
    x[(size_t)b * d + c] = emb[(size_t)tk * d + c] * sqrt_d + pe[(size_t)t * d + c];
}
hipError_t launch_embed_tokens(const float* emb, const float* pe, const int64_t* tok, const int* step_ptr, float* x,
                               int M, int d, hipStream_t s, const int* rows_ptr, const int* stop) {
  hipLaunchKernelGGL(embed_tokens_kernel, dim3(M), dim3(256), 0, s, emb, pe, tok, step_ptr, x, d, sqrtf((float)d), rows_ptr, stop);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void beam_topk_kernel(const float* __restrict__ logits,
                                                        const float* __restrict__ scores, int V,
                                                        float* __restrict__ topv, int* __restrict__ topi,
                                                        const int* __restrict__ seg, int kmax,
                                                        const int* __restrict__ step, const int* __restrict__ stop) {
  if (stop && *stop && *step >= *stop) return;  // device-side beam loop: every sample has finished
  // this block's segment of rows
  const int off = seg[blockIdx.x * 3], M = seg[blockIdx.x * 3 + 1], k = seg[blockIdx.x * 3 + 2];
  if (M <= 0 || k <= 0) return;  // block-uniform
  logits += (size_t)off * V;
  scores += off;
  topv += (size_t)blockIdx.x * kmax;
  topi += (size_t)blockIdx.x * kmax;
  __shared__ float s_lse[16];
  __shared__ float r_v[4];
  __shared__ int r_i[4];
  __shared__ float sel_v;
  __shared__ int sel_i;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // log-sum-exp of every row (F.log_softmax, tfm.py:169)
  for (int i = wave; i < M; i += 4) {
    const float* row = logits + (size_t)i * V;
    float mx = -INFINITY;
    for (int v = lane; v < V; v += 64) mx = fmaxf(mx, row[v]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += expf(row[v] - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) s_lse[i] = mx + logf(sum);
  }
  __syncthreads();
  const int total = M * V;
  float last_v = INFINITY;
  int last_i = -1;
  for (int sel = 0; sel < k; ++sel) {
    // best candidate strictly after (last_v, last_i) in (value desc, index asc) order
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int idx = tid; idx < total; idx += 256) {
      const int i = idx / V;
      const float c = scores[i] + (logits[idx] - s_lse[i]);
      const bool after = c < last_v || (c == last_v && idx > last_i);
      if (after && (c > bv || (c == bv && idx < bi))) { bv = c; bi = idx; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { r_v[wave] = bv; r_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w)
        if (r_v[w] > bv || (r_v[w] == bv && r_i[w] < bi)) { bv = r_v[w]; bi = r_i[w]; }
      sel_v = bv; sel_i = bi;
      topv[sel] = bv; topi[sel] = bi;
    }
    __syncthreads();
    last_v = sel_v; last_i = sel_i;
    __syncthreads();
  }
}
hipError_t launch_beam_topk_batch(const float* logits, const float* scores, const int* seg, int N, int V, int kmax,
                                  float* topv, int* topi, hipStream_t s, const int* step, const int* stop) {
  if (N < 1 || kmax < 1 || kmax > 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_topk_kernel, dim3(N), dim3(256), 0, s, logits, scores, V, topv, topi, seg, kmax, step, stop);
  return hipGetLastError();
}

__global__ void cache_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                    const int* __restrict__ prev, int cap, int M, int heads, int Lmax, int hd,
                                    int rows) {
  // grid: (slab, i, head); copies rows*hd contiguous floats
  const int slab = blockIdx.x, i = blockIdx.y, h = blockIdx.z;
  const size_t per_row = (size_t)heads * Lmax * hd;
  const float* s = src + ((size_t)slab * cap + prev[i]) * per_row + (size_t)h * Lmax * hd;
  float* d = dst + ((size_t)slab * cap + i) * per_row + (size_t)h * Lmax * hd;
  const int n4 = rows * hd / 4;
  for (int c = threadIdx.x; c < n4; c += blockDim.x)
    reinterpret_cast<float4*>(d)[c] = reinterpret_cast<const float4*>(s)[c];
}
hipError_t launch_cache_gather(const float* src, float* dst, const int* prev, int slabs, int cap, int M, int heads,
                               int Lmax, int hd, int rows, hipStream_t s) {
  hipLaunchKernelGGL(cache_gather_kernel, dim3(slabs, M, heads), dim3(256), 0, s, src, dst, prev, cap, M, heads, Lmax,
                     hd, rows);
  return hipGetLastError();
}

// Beam search without the cache copy: anc[row][j] = cache row that holds position j of hypothesis `row`.  Before step t
// (read from the host's step pack) the survivors inherit their parent's ancestry and add the parent's row for position
// t - 1; the kernel also publishes t in the engine's step counter.  One block per row.
__global__ void beam_ancestry_kernel(const int* __restrict__ anc_old, int* __restrict__ anc_new, const int* __restrict__ prev,
                                     int stride, const int* __restrict__ step_in, int* __restrict__ step_out,
                                     const int* __restrict__ rows_ptr, const int* __restrict__ stop) {
  const int t = *step_in, row = blockIdx.x;
  if (row == 0 && threadIdx.x == 0) *step_out = t;
  if (!anc_new || t < 1) return;
  if ((rows_ptr && row >= *rows_ptr) || (stop && *stop && t >= *stop)) return;
  const int p = prev[row];
  const int* src = anc_old + (size_t)p * stride;
  int* dst = anc_new + (size_t)row * stride;
  for (int j = threadIdx.x; j < t - 1; j += blockDim.x) dst[j] = src[j];
  if (threadIdx.x == 0) dst[t - 1] = p;
}
hipError_t launch_beam_ancestry(const int* anc_old, int* anc_new, const int* prev, int rows, int stride, const int* step_in,
                                int* step_out, hipStream_t s, const int* rows_ptr, const int* stop) {
  if (rows < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_ancestry_kernel, dim3(rows), dim3(64), 0, s, anc_old, anc_new, prev, stride, step_in, step_out, rows_ptr, stop);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Device-side beam bookkeeping (round 4): Beam.advance (tools/beam.py:68-105) for every sample of a batched beam search in ONE
// single-block launch per step, so that the step loop needs no host round trip and can be captured as a graph.
// Thread i owns sample i (i, i + 256, ...).  Pass 1: its `live` candidates in order -- prev = idx / V, word = idx % V; a
// candidate ending in [s] joins the sample's completed set (step, parent row, score), the others become next step's
// hypotheses; a sample with `beam` completed hypotheses is finished (Beam.done) and its rows drop out.  Pass 2: the samples'
// new row counts are prefix-summed (rows stay compact, in sample order, as the host version kept them).  Pass 3: the new rows'
// token / score / sample / parent, and the (parent, token) history record the host walks back through at the end.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_dev_init_kernel(const BeamDev b, long long go_token) {
  for (int i = threadIdx.x; i < b.N; i += 256) {
    b.seg[3 * i] = i; b.seg[3 * i + 1] = 1; b.seg[3 * i + 2] = b.beam;
    b.tok[i] = go_token; b.scores[i] = 0.f; b.map[i] = i; b.prev[i] = i;
    b.comp_n[i] = 0; b.fin[i] = 0;
  }
  if (threadIdx.x == 0) { b.ctrl[0] = 0; b.ctrl[1] = b.N; b.ctrl[2] = 0; b.ctrl[3] = 0; }
}
hipError_t launch_beam_dev_init(const BeamDev& b, int64_t go_token, hipStream_t s) {
  hipLaunchKernelGGL(beam_dev_init_kernel, dim3(1), dim3(256), 0, s, b, (long long)go_token);
  return hipGetLastError();
}
__global__ __launch_bounds__(256) void beam_dev_advance_kernel(const BeamDev b) {
  constexpr int KMAX = 16, SPT = 4;  // beam <= 16; up to 4 samples per thread (N <= 1024)
  __shared__ int s_new[1024], s_off[1024];
  const int t = b.ctrl[0];
  if (b.ctrl[2] && t >= b.ctrl[2]) return;  // every sample finished at an earlier step
  int n_par[SPT][KMAX], n_word[SPT][KMAX];
  float n_val[SPT][KMAX];
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int i = threadIdx.x + 256 * q;
    if (i >= b.N) break;
    int newM = 0;
    if (!b.fin[i] && b.seg[3 * i + 1] > 0) {
      const int off = b.seg[3 * i], live = b.seg[3 * i + 2];
      int cn = b.comp_n[i];
      for (int r = 0; r < live; ++r) {
        const int idx = b.topi[(size_t)i * b.beam + r], prev = idx / b.V, word = idx - prev * b.V;
        const float val = b.topv[(size_t)i * b.beam + r];
        if (word == b.end_token) {
          b.comp_t[(size_t)i * b.beam + cn] = t; b.comp_par[(size_t)i * b.beam + cn] = off + prev; b.comp_score[(size_t)i * b.beam + cn] = val;
          ++cn;
        } else {
          n_par[q][newM] = off + prev; n_word[q][newM] = word; n_val[q][newM] = val;
          ++newM;
        }
      }
      b.comp_n[i] = cn;
      if (cn == b.beam) { b.fin[i] = 1; newM = 0; }
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
    if (run == 0) b.ctrl[2] = t + 1;  // nothing left to extend: the remaining steps of the loop return at once
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int i = threadIdx.x + 256 * q;
    if (i >= b.N) break;
    const int off = s_off[i], newM = s_new[i];
    for (int j = 0; j < newM; ++j) {
      const int row = off + j;
      b.tok[row] = n_word[q][j]; b.scores[row] = n_val[q][j]; b.map[row] = i; b.prev[row] = n_par[q][j];
      b.hist_par[(size_t)t * b.cap + row] = n_par[q][j];
      b.hist_tok[(size_t)t * b.cap + row] = n_word[q][j];
    }
    b.seg[3 * i] = off; b.seg[3 * i + 1] = newM; b.seg[3 * i + 2] = b.fin[i] ? 0 : b.beam - b.comp_n[i];
  }
}
hipError_t launch_beam_dev_advance(const BeamDev& b, hipStream_t s) {
  if (b.N < 1 || b.N > 1024 || b.beam < 1 || b.beam > 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_dev_advance_kernel, dim3(1), dim3(256), 0, s, b);
  return hipGetLastError();
}

}  // namespace d2t
