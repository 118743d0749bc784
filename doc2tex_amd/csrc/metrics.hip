// The quadratic work of the reference's validation_step (engine/inferencing.py:133-134,226) on the device: Levenshtein
// distances of symbol strings (modules/metrics/ed.py) and BLEU's clipped n-gram counts (modules/metrics/bleu.py:96-105).
// include/d2t.h has the contract.  Integers only, one block per sample, no atomics, no host synchronisation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/d2t.h"

namespace d2t {

constexpr int ED_THREADS = 1024;  // one pair: a long diagonal has thousands of independent cells
constexpr int MET_THREADS = 256;  // one BLEU sample
constexpr int ED_LDS_DIAG = D2T_METRIC_ED_LDS_LEN + 1;  // entries of one diagonal kept in LDS

// Anti-diagonal wavefront.  D[i][j] = distance of s[0, i) and t[0, j); diagonal d holds the cells with i + j = d, stored
// at index i (0 <= i <= ls, ls <= lt).  A cell needs D[i-1][j] and D[i][j-1] from diagonal d - 1 and D[i-1][j-1] from
// d - 2, so three buffers of ls + 1 entries rotate: diagonal d overwrites d - 3, last read while d - 1 was formed, and one
// barrier per diagonal is enough.  Returns D[ls][lt] (every thread).
template <typename Buf>
__device__ __forceinline__ int32_t ed_wavefront(const int32_t* __restrict__ s, int ls, const int32_t* __restrict__ t, int lt,
                                                Buf* cur, Buf* p1, Buf* p2) {
  if (threadIdx.x == 0) cur[0] = 0;  // diagonal 0
  __syncthreads();
  const int last = ls + lt;
  for (int d = 1; d <= last; ++d) {
    Buf* const w = p2;  // rotate: the oldest buffer receives diagonal d
    p2 = p1;
    p1 = cur;
    cur = w;
    const int lo = d > lt ? d - lt : 0, hi = d < ls ? d : ls;
    for (int i = lo + (int)threadIdx.x; i <= hi; i += ED_THREADS) {
      const int j = d - i;
      int32_t v = d;  // first row / first column
      if (i > 0 && j > 0) {
        const int32_t up = p1[i - 1], left = p1[i];
        const int32_t diag = p2[i - 1] + (s[i - 1] != t[j - 1] ? 1 : 0);
        v = (up < left ? up : left) + 1;
        v = diag < v ? diag : v;
      }
      cur[i] = v;
    }
    __syncthreads();
  }
  return cur[ls];
}

__global__ __launch_bounds__(ED_THREADS) void edit_distance_kernel(const int32_t* __restrict__ a_sym, const int64_t* __restrict__ a_off,
                                                                    int64_t a_total, const int32_t* __restrict__ b_sym,
                                                                    const int64_t* __restrict__ b_off, int64_t b_total,
                                                                    int32_t* __restrict__ dist, int64_t max_len, int32_t* ws,
                                                                    int64_t ws_stride) {
  __shared__ int32_t lds[3 * ED_LDS_DIAG];
  const int p = blockIdx.x;
  const int64_t a0 = a_off[p], a1 = a_off[p + 1], b0 = b_off[p], b1 = b_off[p + 1];
  // block-uniform: a pair the call's bounds do not cover is reported, not read
  if (a0 < 0 || a1 < a0 || a1 > a_total || a1 - a0 > max_len || b0 < 0 || b1 < b0 || b1 > b_total || b1 - b0 > max_len) {
    if (threadIdx.x == 0) dist[p] = -1;
    return;
  }
  const int32_t* s = a_sym + a0;
  const int32_t* t = b_sym + b0;
  int ls = (int)(a1 - a0), lt = (int)(b1 - b0);
  if (ls > lt) {  // the distance is symmetric: the shorter string indexes the diagonals
    const int32_t* q = s; s = t; t = q;
    const int l = ls; ls = lt; lt = l;
  }
  int32_t r;
  if (ls == 0) {
    r = lt;
  } else if (ls < ED_LDS_DIAG) {
    r = ed_wavefront(s, ls, t, lt, lds, lds + ED_LDS_DIAG, lds + 2 * ED_LDS_DIAG);
  } else if (ws) {  // ls <= max_len, and ws_stride = 3 * (max_len + 1)
    int32_t* g = ws + (int64_t)p * ws_stride;
    const int64_t n = max_len + 1;
    r = ed_wavefront(s, ls, t, lt, g, g + n, g + 2 * n);
  } else {
    r = -1;
  }
  if (threadIdx.x == 0) dist[p] = r;
}

// block-wide reductions over the 256 threads, in a fixed order; the result is valid in every thread
__device__ __forceinline__ int block_min(int x, int* part) {
  for (int o = 32; o > 0; o >>= 1) {
    const int y = __shfl_xor(x, o, 64);
    x = y < x ? y : x;
  }
  __syncthreads();  // part may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
  __syncthreads();
  int r = part[0];
  for (int w = 1; w < MET_THREADS / 64; ++w) r = part[w] < r ? part[w] : r;
  return r;
}
__device__ __forceinline__ int block_sum(int x, int* part) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
  __syncthreads();
  int r = 0;
  for (int w = 0; w < MET_THREADS / 64; ++w) r += part[w];
  return r;
}

__global__ __launch_bounds__(MET_THREADS) void bleu_counts_kernel(const int64_t* __restrict__ cand, int cand_cols,
                                                                  const int64_t* __restrict__ ref, int ref_cols, int64_t end_token,
                                                                  int max_n, int64_t* __restrict__ out) {
  __shared__ int64_t sc[D2T_METRIC_BLEU_MAX_COLS];
  __shared__ int64_t sr[D2T_METRIC_BLEU_MAX_COLS];
  __shared__ int part[MET_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t* c = cand + (int64_t)p * cand_cols;
  const int64_t* r = ref + (int64_t)p * ref_cols;
  int cfirst = cand_cols, rfirst = ref_cols;  // first end_token of each row, or the row's width
  for (int i = tid; i < cand_cols; i += MET_THREADS) {
    const int64_t v = c[i];
    sc[i] = v;
    if (v == end_token && i < cfirst) cfirst = i;
  }
  for (int i = tid; i < ref_cols; i += MET_THREADS) {
    const int64_t v = r[i];
    sr[i] = v;
    if (v == end_token && i < rfirst) rfirst = i;
  }
  const int clen = block_min(cfirst, part);  // (its barriers publish sc / sr too)
  const int rlen = block_min(rfirst, part);
  int64_t* o = out + (int64_t)p * (2 + max_n);
  if (tid == 0) {
    o[0] = clen;
    o[1] = rlen;
  }
  for (int n = 1; n <= max_n; ++n) {
    const int nc = clen - n + 1, nr = rlen - n + 1;  // n-grams of each side (<= 0: none)
    int local = 0;
    for (int i = tid; i < nc; i += MET_THREADS) {
      int64_t g[4];
      for (int m = 0; m < 4; ++m) g[m] = m < n ? sc[i + m] : 0;
      int in_ref = 0;
      for (int k = 0; k < nr; ++k) {
        bool eq = sr[k] == g[0];
        for (int m = 1; m < n; ++m) eq = eq && sr[k + m] == g[m];
        in_ref += eq ? 1 : 0;
      }
      if (in_ref == 0) continue;
      int earlier = 0;
      for (int k = 0; k < i; ++k) {
        bool eq = sc[k] == g[0];
        for (int m = 1; m < n; ++m) eq = eq && sc[k + m] == g[m];
        earlier += eq ? 1 : 0;
      }
      local += earlier < in_ref ? 1 : 0;
    }
    const int total = block_sum(local, part);
    if (tid == 0) o[1 + n] = total;
  }
}

}  // namespace d2t

extern "C" {

int d2t_metric_edit_distance_workspace(int32_t N, int64_t max_len, int64_t* bytes_out) {
  if (!bytes_out || N < 0 || max_len < 0 || max_len > D2T_METRIC_ED_MAX_LEN) return D2T_EINVAL;
  *bytes_out = max_len <= D2T_METRIC_ED_LDS_LEN ? 0 : (int64_t)N * 3 * (max_len + 1) * (int64_t)sizeof(int32_t);
  return D2T_OK;
}

int d2t_metric_edit_distance(const int32_t* a_sym, const int64_t* a_off, int64_t a_total, const int32_t* b_sym,
                             const int64_t* b_off, int64_t b_total, int32_t* dist, int32_t N, int64_t max_len, void* workspace,
                             int64_t workspace_bytes, d2t_stream stream) {
  int64_t need = 0;
  if (d2t_metric_edit_distance_workspace(N, max_len, &need) != D2T_OK) return D2T_EINVAL;
  if (!a_off || !b_off || !dist || a_total < 0 || b_total < 0 || (!a_sym && a_total) || (!b_sym && b_total)) return D2T_EINVAL;
  if (need > 0 && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 3))) return D2T_EINVAL;
  if (N == 0) return D2T_OK;
  d2t::edit_distance_kernel<<<dim3(N), dim3(d2t::ED_THREADS), 0, (hipStream_t)stream>>>(
      a_sym, a_off, a_total, b_sym, b_off, b_total, dist, max_len, need > 0 ? (int32_t*)workspace : nullptr, 3 * (max_len + 1));
  return hipGetLastError() == hipSuccess ? D2T_OK : D2T_EHIP;
}

int d2t_metric_bleu_counts(const int64_t* cand, int32_t cand_cols, const int64_t* ref, int32_t ref_cols, int32_t N,
                           int64_t end_token, int32_t max_n, int64_t* out, d2t_stream stream) {
  if (!cand || !ref || !out || N < 0 || max_n < 1 || max_n > 4) return D2T_EINVAL;
  if (cand_cols < 1 || cand_cols > D2T_METRIC_BLEU_MAX_COLS || ref_cols < 1 || ref_cols > D2T_METRIC_BLEU_MAX_COLS) return D2T_EINVAL;
  if (N == 0) return D2T_OK;
  d2t::bleu_counts_kernel<<<dim3(N), dim3(d2t::MET_THREADS), 0, (hipStream_t)stream>>>(cand, cand_cols, ref, ref_cols, end_token,
                                                                                      max_n, out);
  return hipGetLastError() == hipSuccess ? D2T_OK : D2T_EHIP;
}

}  // extern "C"
