// The rest of the reference builder's optimizers (modules/optim/builder.py:76-94) on the pattern of optim.hip: LAMB, AdamP,
// MADGRAD and the Lookahead synchronisation as multi-tensor kernels over a table of chunks (one block = at most
// D2T_OPTIM_CHUNK elements of one tensor).  include/d2t.h has the contract.  Every sum above one element is a double, formed
// in a fixed order and without atomics; every new parameter is written twice, to the module's tensor and to the engine's raw
// copy of it; nothing waits for the device.
//   LAMB      sumsq, norm, moments + per-chunk sums of p^2 and u^2, apply (trust ratio summed per tensor by each block)
//   AdamP     [sumsq, norm,] moments + per-row sums, decision (one block per tensor), apply
//   MADGRAD   [sumsq, norm,] one elementwise launch
//   Lookahead one elementwise launch
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "optim_common.h"

namespace d2t {

// one block's work; the scalars of its tensor are in FamTensor[tensor]
struct FamChunk {
  float* p;
  const float* g;
  float *a, *b, *c;  // state: LAMB / AdamP exp_avg, exp_avg_sq, -; MADGRAD grad_sum_sq, s, x0; Lookahead slow, -, -
  float* mirror;     // engine copy of p, or nullptr
  int n;
  int tensor;
  int64_t off;       // of the chunk's first element in its tensor
};
static_assert(sizeof(FamChunk) == 64, "table entries are 16-byte multiples");

enum : int { FAM_ADAPT = 1, FAM_TRUST_CLIP = 2, FAM_NESTEROV = 4, FAM_DECOUPLED = 8, FAM_MOMENTUM = 16 };

// a tensor's scalars as the kernels use them (derived on the host in double, rounded once)
struct FamTensor {
  float b1, w1;      // beta1; its weight on g: 1 - beta1 (LAMB: beta3)
  float b2, w2;      // beta2, 1 - beta2
  float bc1, sbc2;   // LAMB: bias correction 1; sqrt(bias correction 2)
  float eps, wd;
  float lr;          // LAMB: lr.  AdamP: lr / bc1.  MADGRAD: lamb = (lr + eps) * sqrt(step)
  float decay;       // AdamP, MADGRAD (decoupled): 1 - lr * wd
  float decay_proj;  // AdamP: 1 - lr * wd * wd_ratio
  float ck;          // MADGRAD: 1 - momentum
  float keep;        // MADGRAD: 1 - ck
  int flags;
  int rows, len;     // AdamP: reshape(size(0), -1) of a tensor with more than one dimension; rows 0 = no projection
  int group;         // AdamP: lanes that share one row piece (a power of two up to 64)
  int first_chunk, nchunks;
  int pad_;
  int64_t row_base;  // first entry of this tensor's rows in the row sums
  double delta, deps;
  int32_t* mode_out;  // AdamP: where the caller reads the decision, or nullptr
};
static_assert(sizeof(FamTensor) % 16 == 0, "table entries are 16-byte multiples");

// scratch of one step, all in d2t_optim::family
struct FamScratch {
  double* partial;  // [chunks] sum of squares of the gradient
  double* csum;     // [chunks][2][4]  LAMB: [c][0][0..1] = sum p^2, sum u^2.  AdamP: row pieces cut by the chunk's head / tail
  double* rsum;     // [rows of all projecting tensors][4]  AdamP: g.p, g.g, p.p, p.perturb
  double* tsum;     // [tensors][4]  AdamP: the same over the whole tensor
  int* mode;        // [tensors]  AdamP: 0 none, 1 channel, 2 layer
};

__device__ inline bool fam_vec(const FamChunk& c) {
  return ((reinterpret_cast<uintptr_t>(c.p) | reinterpret_cast<uintptr_t>(c.g) | reinterpret_cast<uintptr_t>(c.a) |
           reinterpret_cast<uintptr_t>(c.b) | reinterpret_cast<uintptr_t>(c.c) | reinterpret_cast<uintptr_t>(c.mirror)) & 15) == 0;
}

template <int W> struct Vec { float v[W]; };
template <int W> __device__ inline Vec<W> vload(const float* p, int e) {
  Vec<W> r;
  if constexpr (W == 4) {
    const float4 x = *reinterpret_cast<const float4*>(p + e);
    r.v[0] = x.x; r.v[1] = x.y; r.v[2] = x.z; r.v[3] = x.w;
  } else {
    r.v[0] = p[e];
  }
  return r;
}
template <int W> __device__ inline void vstore(float* p, int e, const Vec<W>& r) {
  if constexpr (W == 4) *reinterpret_cast<float4*>(p + e) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else p[e] = r.v[0];
}

// body.run<4>(e) on this thread's quads when the chunk's pointers allow 16-byte accesses, body.run<1>(e) on the rest
template <class Body> __device__ inline void chunk_loop(int n, bool vec, Body& body) {
  int done = 0;
  if (vec) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += OPT_THREADS) body.template run<4>(i << 2);
    done = n4 << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += OPT_THREADS) body.template run<1>(i);
}

// K sums over the block in block_sum's fixed order, the results in every thread
template <int K> __device__ inline void block_sum_all(double (&x)[K]) {
  __shared__ double part[K][OPT_THREADS / 64];
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) x[k] += __shfl_down(x[k], o, 64);
  __syncthreads();  // a previous call's readers are done
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < K; ++k) part[k][threadIdx.x >> 6] = x[k];
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    double r = 0.0;
    for (int w = 0; w < OPT_THREADS / 64; ++w) r += part[k][w];
    x[k] = r;
  }
}

// ---- the global gradient norm ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void fam_sumsq_kernel(const FamChunk* __restrict__ table, double* __restrict__ partial) {
  const FamChunk c = table[blockIdx.x];
  const double s = block_sum((double)chunk_sumsq(c.g, c.n));
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one block: norm = sqrt(sum of the partials), in double and in a fixed order.  coef multiplies the gradients:
// clip_grad_norm_'s min(1, max_norm / (norm + 1e-6)), or under `lamb` divides them: norm / max_norm where norm > max_norm,
// else 1 (LAMB's own rule, without the 1e-6).  A NaN norm gives a NaN coefficient in the first and 1 in the second, as
// the formulas do.
__global__ __launch_bounds__(OPT_THREADS) void fam_norm_kernel(const double* __restrict__ partial, int count, float max_norm, int lamb,
                                                               float* __restrict__ norm_out, float* __restrict__ coef_out) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += OPT_THREADS) acc += partial[i];
  const double s = block_sum(acc);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    if (norm_out) *norm_out = norm;
    if (lamb) {
      *coef_out = norm > max_norm ? norm / max_norm : 1.f;
    } else {
      const float c = max_norm / (norm + 1e-6f);
      *coef_out = c < 1.f ? c : (c != c ? c : 1.f);
    }
  }
}

// ---- LAMB --------------------------------------------------------------------------------------------------------------
// the update direction: a pure function of the new moments and the old parameter, formed in both passes
__device__ inline float lamb_update(const FamTensor& t, float p, float m, float v) {
  float u = (m / t.bc1) / (sqrtf(v) / t.sbc2 + t.eps);
  if (t.wd != 0.f) u += t.wd * p;
  return u;
}

struct LambMoments {
  const FamChunk& c;
  const FamTensor& t;
  float div;
  double pp, uu;
  template <int W> __device__ void run(int e) {
    const Vec<W> g = vload<W>(c.g, e), p = vload<W>(c.p, e);
    Vec<W> m = vload<W>(c.a, e), v = vload<W>(c.b, e);
    for (int k = 0; k < W; ++k) {
      const float gk = g.v[k] / div;
      m.v[k] = t.b1 * m.v[k] + t.w1 * gk;
      v.v[k] = t.b2 * v.v[k] + t.w2 * gk * gk;
      const float u = lamb_update(t, p.v[k], m.v[k], v.v[k]);
      pp += (double)p.v[k] * (double)p.v[k];
      uu += (double)u * (double)u;
    }
    vstore<W>(c.a, e, m);
    vstore<W>(c.b, e, v);
  }
};

__global__ __launch_bounds__(OPT_THREADS) void lamb_moments_kernel(const FamChunk* __restrict__ table, const FamTensor* __restrict__ tensors,
                                                                   const float* __restrict__ div_dev, double* __restrict__ csum) {
  const FamChunk c = table[blockIdx.x];
  const FamTensor t = tensors[c.tensor];
  LambMoments body{c, t, *div_dev, 0.0, 0.0};
  chunk_loop(c.n, fam_vec(c), body);
  if (!(t.flags & FAM_ADAPT)) return;
  double s[2] = {body.pp, body.uu};
  block_sum_all<2>(s);
  if (threadIdx.x == 0) {
    csum[(size_t)blockIdx.x * 8 + 0] = s[0];
    csum[(size_t)blockIdx.x * 8 + 1] = s[1];
  }
}

struct LambApply {
  const FamChunk& c;
  const FamTensor& t;
  float trust;
  template <int W> __device__ void run(int e) {
    Vec<W> p = vload<W>(c.p, e);
    const Vec<W> m = vload<W>(c.a, e), v = vload<W>(c.b, e);
    for (int k = 0; k < W; ++k) p.v[k] -= t.lr * (lamb_update(t, p.v[k], m.v[k], v.v[k]) * trust);
    vstore<W>(c.p, e, p);
    if (c.mirror) vstore<W>(c.mirror, e, p);
  }
};

__global__ __launch_bounds__(OPT_THREADS) void lamb_apply_kernel(const FamChunk* __restrict__ table, const FamTensor* __restrict__ tensors,
                                                                 const double* __restrict__ csum) {
  const FamChunk c = table[blockIdx.x];
  const FamTensor t = tensors[c.tensor];
  float trust = 1.f;
  if (t.flags & FAM_ADAPT) {
    // this tensor's chunks in chunk order: every block of the tensor forms the same two sums
    double s[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < t.nchunks; j += OPT_THREADS) {
      s[0] += csum[(size_t)(t.first_chunk + j) * 8 + 0];
      s[1] += csum[(size_t)(t.first_chunk + j) * 8 + 1];
    }
    block_sum_all<2>(s);
    const float pn = (float)sqrt(s[0]), un = (float)sqrt(s[1]);
    if (pn > 0.f && un > 0.f) trust = pn / un;
    if ((t.flags & FAM_TRUST_CLIP) && trust > 1.f) trust = 1.f;
  }
  LambApply body{c, t, trust};
  chunk_loop(c.n, fam_vec(c), body);
}

// ---- AdamP -------------------------------------------------------------------------------------------------------------
__device__ inline void adamp_moments(const FamTensor& t, float g, float& m, float& v) {
  m = t.b1 * m + t.w1 * g;
  v = t.b2 * v + t.w2 * g * g;
}
// a pure function of the new moments and the (clipped) gradient, formed in both passes
__device__ inline float adamp_perturb(const FamTensor& t, float g, float m, float v) {
  const float denom = sqrtf(v) / t.sbc2 + t.eps;
  return ((t.flags & FAM_NESTEROV) ? t.b1 * m + t.w1 * g : m) / denom;
}

struct AdampMoments {
  const FamChunk& c;
  const FamTensor& t;
  float coef;
  template <int W> __device__ void run(int e) {
    const Vec<W> g = vload<W>(c.g, e);
    Vec<W> m = vload<W>(c.a, e), v = vload<W>(c.b, e);
    for (int k = 0; k < W; ++k) adamp_moments(t, g.v[k] * coef, m.v[k], v.v[k]);
    vstore<W>(c.a, e, m);
    vstore<W>(c.b, e, v);
  }
};

// the moments of W elements of a row piece and their share of the piece's four sums
struct AdampRowSums {
  const FamChunk& c;
  const FamTensor& t;
  float coef;
  double s[4];
  template <int W> __device__ void run(int e) {
    const Vec<W> g = vload<W>(c.g, e), p = vload<W>(c.p, e);
    Vec<W> m = vload<W>(c.a, e), v = vload<W>(c.b, e);
    for (int k = 0; k < W; ++k) {
      const float gk = g.v[k] * coef;
      adamp_moments(t, gk, m.v[k], v.v[k]);
      const float pert = adamp_perturb(t, gk, m.v[k], v.v[k]);
      s[0] += (double)gk * (double)p.v[k];
      s[1] += (double)gk * (double)gk;
      s[2] += (double)p.v[k] * (double)p.v[k];
      s[3] += (double)p.v[k] * (double)pert;
    }
    vstore<W>(c.a, e, m);
    vstore<W>(c.b, e, v);
  }
};

// Moments of one chunk and, for a tensor that may be projected, the four sums of every row piece the chunk holds: a piece
// is one row cut to the chunk, `group` lanes stride over it -- by quads between its first and last 16-byte boundary where
// the chunk's pointers allow, by single elements at its ends and otherwise -- and fold their doubles by halving strides.
// A whole row goes to rsum; a piece of a row that began in an earlier chunk to the chunk's head slot, one that ends in a
// later chunk to its tail slot (the decision kernel adds those in chunk order).
__global__ __launch_bounds__(OPT_THREADS) void adamp_moments_kernel(const FamChunk* __restrict__ table, const FamTensor* __restrict__ tensors,
                                                                    const float* __restrict__ coef_dev, FamScratch sc) {
  const FamChunk c = table[blockIdx.x];
  const FamTensor t = tensors[c.tensor];
  const float coef = coef_dev ? *coef_dev : 1.f;
  const bool vec = fam_vec(c);
  if (t.rows == 0) {
    AdampMoments body{c, t, coef};
    chunk_loop(c.n, vec, body);
    return;
  }
  const int64_t L = t.len, lo_c = c.off, hi_c = c.off + c.n;
  const int64_t r0 = lo_c / L;
  const int pieces = (int)((hi_c - 1) / L - r0) + 1;
  const int G = t.group, lane = threadIdx.x & (G - 1), groups = OPT_THREADS / G, gid = threadIdx.x / G;
  for (int k0 = 0; k0 < pieces; k0 += groups) {  // uniform trip count: every lane takes part in the shuffles
    const int k = k0 + gid;
    const int64_t r = r0 + k;
    // the piece in the chunk's own indices: [a, b), quads in [a4, b4)
    const int a = k < pieces ? (int)(std::max(lo_c, r * L) - lo_c) : 0, b = k < pieces ? (int)(std::min(hi_c, (r + 1) * L) - lo_c) : 0;
    const int a4 = vec ? std::min(b, (a + 3) & ~3) : b, b4 = vec ? std::max(a4, b & ~3) : b;
    AdampRowSums body{c, t, coef, {0.0, 0.0, 0.0, 0.0}};
    for (int e = a + lane; e < a4; e += G) body.template run<1>(e);
    for (int e = a4 + 4 * lane; e < b4; e += 4 * G) body.template run<4>(e);
    for (int e = b4 + lane; e < b; e += G) body.template run<1>(e);
    for (int j = 0; j < 4; ++j)
      for (int o = G >> 1; o > 0; o >>= 1) body.s[j] += __shfl_down(body.s[j], o, G);
    if (k < pieces && lane == 0) {
      double* out;
      if (r * L < lo_c) out = sc.csum + (size_t)blockIdx.x * 8;
      else if ((r + 1) * L > hi_c) out = sc.csum + (size_t)blockIdx.x * 8 + 4;
      else out = sc.rsum + (size_t)(t.row_base + r) * 4;
      for (int j = 0; j < 4; ++j) out[j] = body.s[j];
    }
  }
}

// F.cosine_similarity(g, p, eps): g.p / (max(|g|, eps) * max(|p|, eps)), absolute
__device__ inline double abs_cos(const double* s, double eps) {
  return fabs(s[0] / (fmax(sqrt(s[1]), eps) * fmax(sqrt(s[2]), eps)));
}

// One block per tensor: completes the rows that span chunks, sums the rows in row order to the tensor's sums, and decides:
// channel mode where the largest |cos| of a row is below delta / sqrt(row length), else layer mode where the tensor's
// |cos| is below delta / sqrt(numel), else none.  A NaN cosine stays in the maximum and compares false, as in torch.
__global__ __launch_bounds__(OPT_THREADS) void adamp_decide_kernel(const FamTensor* __restrict__ tensors, FamScratch sc) {
  const FamTensor t = tensors[blockIdx.x];
  if (t.rows == 0 || t.nchunks == 0) {
    if (threadIdx.x == 0) {
      sc.mode[blockIdx.x] = 0;
      if (t.mode_out) *t.mode_out = 0;
    }
    return;
  }
  const int64_t L = t.len;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double mx = 0.0;
  for (int r = threadIdx.x; r < t.rows; r += OPT_THREADS) {
    double* row = sc.rsum + (size_t)(t.row_base + r) * 4;
    const int cf = (int)(r * L / D2T_OPTIM_CHUNK), cl = (int)(((r + 1) * L - 1) / D2T_OPTIM_CHUNK);
    double s[4];
    if (cf == cl) {
      for (int j = 0; j < 4; ++j) s[j] = row[j];
    } else {
      for (int j = 0; j < 4; ++j) s[j] = sc.csum[(size_t)(t.first_chunk + cf) * 8 + 4 + j];
      for (int ch = cf + 1; ch <= cl; ++ch)
        for (int j = 0; j < 4; ++j) s[j] += sc.csum[(size_t)(t.first_chunk + ch) * 8 + j];
      for (int j = 0; j < 4; ++j) row[j] = s[j];
    }
    const double cs = abs_cos(s, t.deps);
    if (cs > mx || cs != cs) mx = cs;
    for (int j = 0; j < 4; ++j) acc[j] += s[j];
  }
  block_sum_all<4>(acc);
  __shared__ double wave_max[OPT_THREADS / 64];
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_down(mx, o, 64);
    if (other > mx || other != other) mx = other;
  }
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < OPT_THREADS / 64; ++w)
      if (wave_max[w] > mx || wave_max[w] != wave_max[w]) mx = wave_max[w];
    int mode = 0;
    if (mx < t.delta / sqrt((double)L)) mode = 1;
    else if (abs_cos(acc, t.deps) < t.delta / sqrt((double)L * (double)t.rows)) mode = 2;
    for (int j = 0; j < 4; ++j) sc.tsum[(size_t)blockIdx.x * 4 + j] = acc[j];
    sc.mode[blockIdx.x] = mode;
    if (t.mode_out) *t.mode_out = mode;
  }
}

struct AdampApply {
  const FamChunk& c;
  const FamTensor& t;
  const double* sums;  // mode 1: the tensor's rows in rsum; mode 2: the tensor's entry of tsum
  float coef;
  int mode;
  int64_t have;        // the row whose two scalars are at hand
  float pn, dot;
  template <int W> __device__ void run(int e) {
    const Vec<W> g = vload<W>(c.g, e), m = vload<W>(c.a, e), v = vload<W>(c.b, e);
    Vec<W> p = vload<W>(c.p, e);
    for (int k = 0; k < W; ++k) {
      float pert = adamp_perturb(t, g.v[k] * coef, m.v[k], v.v[k]);
      if (mode) {
        const int64_t row = mode == 1 ? (uint32_t)(c.off + e + k) / (uint32_t)t.len : 0;  // numel < 2^31 (checked)
        if (row != have) {
          // p_n = p / (|p| + eps);  sum over the row of p_n * perturb = (p . perturb) / (|p| + eps)
          pn = (float)sqrt(sums[row * 4 + 2]) + t.eps;
          dot = (float)(sums[row * 4 + 3] / (double)pn);
          have = row;
        }
        pert -= (p.v[k] / pn) * dot;
      }
      if (t.wd > 0.f) p.v[k] *= mode ? t.decay_proj : t.decay;
      p.v[k] -= t.lr * pert;
    }
    vstore<W>(c.p, e, p);
    if (c.mirror) vstore<W>(c.mirror, e, p);
  }
};

__global__ __launch_bounds__(OPT_THREADS) void adamp_apply_kernel(const FamChunk* __restrict__ table, const FamTensor* __restrict__ tensors,
                                                                  const float* __restrict__ coef_dev, FamScratch sc) {
  const FamChunk c = table[blockIdx.x];
  const FamTensor t = tensors[c.tensor];
  const int mode = t.rows ? sc.mode[c.tensor] : 0;
  const double* sums = mode == 1 ? sc.rsum + (size_t)t.row_base * 4 : sc.tsum + (size_t)c.tensor * 4;
  AdampApply body{c, t, sums, coef_dev ? *coef_dev : 1.f, mode, -1, 0.f, 0.f};
  chunk_loop(c.n, fam_vec(c), body);
}

// ---- MADGRAD -----------------------------------------------------------------------------------------------------------
struct Madgrad {
  const FamChunk& c;
  const FamTensor& t;
  float coef;
  template <int W> __device__ void run(int e) {
    const Vec<W> g = vload<W>(c.g, e);
    Vec<W> p = vload<W>(c.p, e), q = vload<W>(c.a, e), s = vload<W>(c.b, e), x0;
    if (t.flags & FAM_MOMENTUM) x0 = vload<W>(c.c, e);
    for (int k = 0; k < W; ++k) {
      float gk = g.v[k] * coef;
      if (t.wd != 0.f) {
        if (t.flags & FAM_DECOUPLED) p.v[k] *= t.decay;
        else gk += t.wd * p.v[k];
      }
      // without momentum x0 is rebuilt from the accumulators before they move.  The iterate z is a difference of terms of
      // like size: it is formed in double from the fp32 accumulators and rounded once
      const double x = (t.flags & FAM_MOMENTUM) ? (double)x0.v[k] : (double)p.v[k] + (double)s.v[k] / (cbrt((double)q.v[k]) + (double)t.eps);
      q.v[k] += t.lr * (gk * gk);
      s.v[k] += t.lr * gk;
      const double z = x - (double)s.v[k] / (cbrt((double)q.v[k]) + (double)t.eps);
      p.v[k] = (float)((t.flags & FAM_MOMENTUM) ? (double)t.keep * (double)p.v[k] + (double)t.ck * z : z);
    }
    vstore<W>(c.p, e, p);
    vstore<W>(c.a, e, q);
    vstore<W>(c.b, e, s);
    if (c.mirror) vstore<W>(c.mirror, e, p);
  }
};

__global__ __launch_bounds__(OPT_THREADS) void madgrad_kernel(const FamChunk* __restrict__ table, const FamTensor* __restrict__ tensors,
                                                              const float* __restrict__ coef_dev) {
  const FamChunk c = table[blockIdx.x];
  const FamTensor t = tensors[c.tensor];
  Madgrad body{c, t, coef_dev ? *coef_dev : 1.f};
  chunk_loop(c.n, fam_vec(c), body);
}

// ---- Lookahead ---------------------------------------------------------------------------------------------------------
struct LookaheadSync {
  const FamChunk& c;
  float alpha;
  template <int W> __device__ void run(int e) {
    const Vec<W> fast = vload<W>(c.p, e);
    Vec<W> slow = vload<W>(c.a, e);
    for (int k = 0; k < W; ++k) slow.v[k] += alpha * (fast.v[k] - slow.v[k]);
    vstore<W>(c.a, e, slow);
    vstore<W>(c.p, e, slow);
    if (c.mirror) vstore<W>(c.mirror, e, slow);
  }
};

__global__ __launch_bounds__(OPT_THREADS) void lookahead_kernel(const FamChunk* __restrict__ table, float alpha) {
  const FamChunk c = table[blockIdx.x];
  LookaheadSync body{c, alpha};
  chunk_loop(c.n, fam_vec(c), body);
}

}  // namespace d2t

using d2t::FamChunk;
using d2t::FamScratch;
using d2t::FamTensor;
using d2t::ofail;

namespace {

// one record of any entry point, in the kernels' terms
struct FamRec {
  float* p;
  const float* g;
  float *a, *b, *c, *mirror;
  const char *an, *bn, *cn;  // names of a, b, c for messages; nullptr: that pointer is not used
  int64_t numel;
  FamTensor t;
};

struct FamPlan {
  size_t chunks = 0;
  const FamChunk* table = nullptr;
  const FamTensor* tensors = nullptr;
  FamScratch sc{};
};

// which parts of the scratch an entry point's kernels use
enum : unsigned { SC_PARTIAL = 1, SC_CSUM = 2, SC_ROWS = 4 };

bool finite_all(std::initializer_list<double> xs) {
  for (double x : xs)
    if (!std::isfinite(x)) return false;
  return true;
}

// Validates every pointer (D2T_EINVAL before anything is enqueued), lays the chunk and tensor tables out, sends them through
// the staging rotation and carves the parts `need` of the scratch.  plan.chunks == 0: nothing to do.
int fam_prepare(d2t_optim* o, std::vector<FamRec>& recs, bool need_grad, unsigned need, hipStream_t s, FamPlan& plan) {
  size_t chunks = 0;
  int64_t rows = 0;
  for (size_t i = 0; i < recs.size(); ++i) {
    FamRec& r = recs[i];
    const int id = (int)i;
    if (r.numel < 0) return ofail(o, D2T_EINVAL, "tensor %d: null pointer or negative size", id);
    r.t.first_chunk = (int)chunks;
    r.t.nchunks = 0;
    r.t.row_base = rows;
    if (r.numel == 0) {
      r.t.rows = 0;
      continue;
    }
    if (!r.p || (need_grad && !r.g) || (r.an && !r.a) || (r.bn && !r.b) || (r.cn && !r.c))
      return ofail(o, D2T_EINVAL, "tensor %d: null pointer or negative size", id);
    int rc;
    if ((rc = d2t::optim_dev_ptr(o, r.p, id, "param")) || (need_grad && (rc = d2t::optim_dev_ptr(o, r.g, id, "grad"))) ||
        (r.an && (rc = d2t::optim_dev_ptr(o, r.a, id, r.an))) || (r.bn && (rc = d2t::optim_dev_ptr(o, r.b, id, r.bn))) ||
        (r.cn && (rc = d2t::optim_dev_ptr(o, r.c, id, r.cn))) || (r.mirror && (rc = d2t::optim_dev_ptr(o, r.mirror, id, "mirror"))) ||
        (r.t.mode_out && (rc = d2t::optim_dev_ptr(o, r.t.mode_out, id, "mode"))))
      return rc;
    r.t.nchunks = (int)((r.numel + D2T_OPTIM_CHUNK - 1) / D2T_OPTIM_CHUNK);
    chunks += (size_t)r.t.nchunks;
    rows += r.t.rows;
    if (chunks > (1u << 24)) return ofail(o, D2T_EINVAL, "more than %u chunks in one step", 1u << 24);
  }
  plan.chunks = chunks;
  if (chunks == 0) return D2T_OK;
  const size_t n = recs.size();
  const size_t table_bytes = chunks * sizeof(FamChunk), bytes = table_bytes + n * sizeof(FamTensor);
  d2t_optim::Stage* g = nullptr;
  if (int rc = d2t::optim_stage_take(o, bytes, &g)) return rc;
  // only what the caller's kernels use: a Lookahead synchronisation or an unclipped MADGRAD step carves nothing
  const size_t n_partial = (need & SC_PARTIAL) ? chunks : 0, n_csum = (need & SC_CSUM) ? chunks * 8 : 0;
  const size_t n_rsum = (need & SC_ROWS) ? (size_t)rows * 4 : 0, n_tsum = (need & SC_ROWS) ? n * 4 : 0;
  const size_t bytes_needed = (n_partial + n_csum + n_rsum + n_tsum) * sizeof(double) + ((need & SC_ROWS) ? n * sizeof(int) : 0);
  if (bytes_needed > o->family_cap) {
    if (o->family) { OHIP(o, hipDeviceSynchronize()); OHIP(o, hipFree(o->family)); }
    o->family = nullptr;
    o->family_cap = 0;
    OHIP(o, hipMalloc(&o->family, bytes_needed * 2));
    o->family_cap = bytes_needed * 2;
  }
  plan.sc.partial = static_cast<double*>(o->family);
  plan.sc.csum = plan.sc.partial + n_partial;
  plan.sc.rsum = plan.sc.csum + n_csum;
  plan.sc.tsum = plan.sc.rsum + n_rsum;
  plan.sc.mode = reinterpret_cast<int*>(plan.sc.tsum + n_tsum);
  FamChunk* t = static_cast<FamChunk*>(g->h);
  FamTensor* tt = reinterpret_cast<FamTensor*>(static_cast<char*>(g->h) + table_bytes);
  for (size_t i = 0; i < n; ++i) {
    const FamRec& r = recs[i];
    tt[i] = r.t;
    FamChunk c{};
    c.tensor = (int)i;
    for (int64_t off = 0; off < r.numel; off += D2T_OPTIM_CHUNK) {
      c.p = r.p + off;
      c.g = r.g ? r.g + off : nullptr;
      c.a = r.a ? r.a + off : nullptr;
      c.b = r.b ? r.b + off : nullptr;
      c.c = r.c ? r.c + off : nullptr;
      c.mirror = r.mirror ? r.mirror + off : nullptr;
      c.n = (int)std::min<int64_t>(D2T_OPTIM_CHUNK, r.numel - off);
      c.off = off;
      *t++ = c;
    }
  }
  if (int rc = d2t::optim_stage_send(o, *g, bytes, s)) return rc;
  plan.table = static_cast<const FamChunk*>(g->d);
  plan.tensors = reinterpret_cast<const FamTensor*>(static_cast<const char*>(g->d) + table_bytes);
  return D2T_OK;
}

// clip_grad_norm_'s coefficient (or LAMB's divisor) into o->coef, the norm into norm_dev (may be nullptr under `lamb`)
void fam_norm(d2t_optim* o, const FamPlan& plan, float max_grad_norm, int lamb, float* norm_dev, hipStream_t s) {
  hipLaunchKernelGGL(d2t::fam_sumsq_kernel, dim3((unsigned)plan.chunks), dim3(d2t::OPT_THREADS), 0, s, plan.table, plan.sc.partial);
  hipLaunchKernelGGL(d2t::fam_norm_kernel, dim3(1), dim3(d2t::OPT_THREADS), 0, s, plan.sc.partial, (int)plan.chunks, max_grad_norm,
                     lamb, norm_dev, o->coef);
}

int clip_args(d2t_optim* o, int32_t n, const void* recs, float max_grad_norm, float* norm_dev) {
  if (n < 0 || (n && !recs)) return ofail(o, D2T_EINVAL, "bad argument: %d tensors", n);
  if (max_grad_norm > 0.f && !norm_dev) return ofail(o, D2T_EINVAL, "clipping needs a device float for the norm");
  if (max_grad_norm > 0.f)
    if (int rc = d2t::optim_dev_ptr(o, norm_dev, -1, "norm")) return rc;
  return D2T_OK;
}

}  // namespace

extern "C" {

int d2t_optim_lamb_step(d2t_optim* o, const d2t_optim_lamb_tensor* in, int32_t n, float max_grad_norm, float* norm_dev,
                        d2t_stream stream) {
  if (!o) return D2T_EINVAL;
  d2t::OptDevGuard dg_(o);
  if (n < 0 || (n && !in)) return ofail(o, D2T_EINVAL, "bad argument: %d tensors", n);
  if (!(max_grad_norm > 0.f) || !std::isfinite(max_grad_norm)) return ofail(o, D2T_EINVAL, "bad scalars (max_grad_norm %g)", max_grad_norm);
  if (norm_dev)
    if (int rc = d2t::optim_dev_ptr(o, norm_dev, -1, "norm")) return rc;
  std::vector<FamRec> recs((size_t)n);
  for (int i = 0; i < n; ++i) {
    const d2t_optim_lamb_tensor& r = in[i];
    if (!(r.bc1 > 0.0) || !(r.sqrt_bc2 > 0.0) || !(r.eps >= 0.0) || !finite_all({r.lr, r.weight_decay, r.beta1, r.beta2, r.beta3}))
      return ofail(o, D2T_EINVAL, "tensor %d: bad scalars (bc1 %g, sqrt_bc2 %g, eps %g, lr %g, weight_decay %g)", i, r.bc1, r.sqrt_bc2,
                   r.eps, r.lr, r.weight_decay);
    FamTensor t{};
    t.b1 = (float)r.beta1;
    t.w1 = (float)r.beta3;
    t.b2 = (float)r.beta2;
    t.w2 = (float)(1.0 - r.beta2);
    t.bc1 = (float)r.bc1;
    t.sbc2 = (float)r.sqrt_bc2;
    t.eps = (float)r.eps;
    t.wd = (float)r.weight_decay;
    t.lr = (float)r.lr;
    t.flags = (r.adapt ? d2t::FAM_ADAPT : 0) | (r.trust_clip ? d2t::FAM_TRUST_CLIP : 0);
    recs[i] = FamRec{r.param, r.grad, r.exp_avg, r.exp_avg_sq, nullptr, r.mirror, "exp_avg", "exp_avg_sq", nullptr, r.numel, t};
  }
  hipStream_t s = (hipStream_t)stream;
  FamPlan plan;
  if (int rc = fam_prepare(o, recs, true, SC_PARTIAL | SC_CSUM, s, plan)) return rc;
  if (plan.chunks == 0) {
    if (norm_dev) OHIP(o, hipMemsetAsync(norm_dev, 0, 4, s));
    return D2T_OK;
  }
  fam_norm(o, plan, max_grad_norm, 1, norm_dev, s);
  hipLaunchKernelGGL(d2t::lamb_moments_kernel, dim3((unsigned)plan.chunks), dim3(d2t::OPT_THREADS), 0, s, plan.table, plan.tensors,
                     o->coef, plan.sc.csum);
  hipLaunchKernelGGL(d2t::lamb_apply_kernel, dim3((unsigned)plan.chunks), dim3(d2t::OPT_THREADS), 0, s, plan.table, plan.tensors,
                     plan.sc.csum);
  OHIP(o, hipGetLastError());
  return D2T_OK;
}

int d2t_optim_adamp_step(d2t_optim* o, const d2t_optim_adamp_tensor* in, int32_t n, float max_grad_norm, float* norm_dev,
                         d2t_stream stream) {
  if (!o) return D2T_EINVAL;
  d2t::OptDevGuard dg_(o);
  if (int rc = clip_args(o, n, in, max_grad_norm, norm_dev)) return rc;
  const bool clip = max_grad_norm > 0.f;
  std::vector<FamRec> recs((size_t)n);
  for (int i = 0; i < n; ++i) {
    const d2t_optim_adamp_tensor& r = in[i];
    if (!(r.bc1 > 0.0) || !(r.sqrt_bc2 > 0.0) || !(r.eps >= 0.0) || !finite_all({r.lr, r.weight_decay, r.beta1, r.beta2, r.delta, r.wd_ratio}))
      return ofail(o, D2T_EINVAL, "tensor %d: bad scalars (bc1 %g, sqrt_bc2 %g, eps %g, lr %g, weight_decay %g, delta %g, wd_ratio %g)",
                   i, r.bc1, r.sqrt_bc2, r.eps, r.lr, r.weight_decay, r.delta, r.wd_ratio);
    if (r.rows < 0 || (r.rows > 0 && (r.numel % r.rows != 0 || r.numel > INT32_MAX)))
      return ofail(o, D2T_EINVAL, "tensor %d: %lld rows do not divide %lld elements (or more than 2^31 - 1 of them)", i,
                   (long long)r.rows, (long long)r.numel);
    FamTensor t{};
    t.b1 = (float)r.beta1;
    t.w1 = (float)(1.0 - r.beta1);
    t.b2 = (float)r.beta2;
    t.w2 = (float)(1.0 - r.beta2);
    t.sbc2 = (float)r.sqrt_bc2;
    t.eps = (float)r.eps;
    t.wd = (float)r.weight_decay;
    t.lr = (float)(r.lr / r.bc1);
    t.decay = (float)(1.0 - r.lr * r.weight_decay);
    t.decay_proj = (float)(1.0 - r.lr * r.weight_decay * r.wd_ratio);
    t.flags = r.nesterov ? d2t::FAM_NESTEROV : 0;
    t.rows = r.numel > 0 ? (int)r.rows : 0;
    t.len = t.rows ? (int)(r.numel / r.rows) : 0;
    t.group = 1;
    while (t.group < 64 && t.group * 8 < t.len) t.group <<= 1;
    t.delta = r.delta;
    t.deps = r.eps;
    t.mode_out = r.mode;
    recs[i] = FamRec{r.param, r.grad, r.exp_avg, r.exp_avg_sq, nullptr, r.mirror, "exp_avg", "exp_avg_sq", nullptr, r.numel, t};
  }
  hipStream_t s = (hipStream_t)stream;
  FamPlan plan;
  if (int rc = fam_prepare(o, recs, true, (clip ? SC_PARTIAL : 0u) | SC_CSUM | SC_ROWS, s, plan)) return rc;
  if (plan.chunks == 0) {
    if (clip) OHIP(o, hipMemsetAsync(norm_dev, 0, 4, s));
    return D2T_OK;
  }
  if (clip) fam_norm(o, plan, max_grad_norm, 0, norm_dev, s);
  const float* coef = clip ? o->coef : nullptr;
  hipLaunchKernelGGL(d2t::adamp_moments_kernel, dim3((unsigned)plan.chunks), dim3(d2t::OPT_THREADS), 0, s, plan.table, plan.tensors,
                     coef, plan.sc);
  hipLaunchKernelGGL(d2t::adamp_decide_kernel, dim3((unsigned)n), dim3(d2t::OPT_THREADS), 0, s, plan.tensors, plan.sc);
  hipLaunchKernelGGL(d2t::adamp_apply_kernel, dim3((unsigned)plan.chunks), dim3(d2t::OPT_THREADS), 0, s, plan.table, plan.tensors, coef,
                     plan.sc);
  OHIP(o, hipGetLastError());
  return D2T_OK;
}

int d2t_optim_madgrad_step(d2t_optim* o, const d2t_optim_madgrad_tensor* in, int32_t n, float max_grad_norm, float* norm_dev,
                           d2t_stream stream) {
  if (!o) return D2T_EINVAL;
  d2t::OptDevGuard dg_(o);
  if (int rc = clip_args(o, n, in, max_grad_norm, norm_dev)) return rc;
  const bool clip = max_grad_norm > 0.f;
  std::vector<FamRec> recs((size_t)n);
  for (int i = 0; i < n; ++i) {
    const d2t_optim_madgrad_tensor& r = in[i];
    if (!(r.eps >= 0.0) || !(r.momentum >= 0.0 && r.momentum < 1.0) || !(r.lamb >= 0.0) || !finite_all({r.lr, r.weight_decay, r.lamb}))
      return ofail(o, D2T_EINVAL, "tensor %d: bad scalars (eps %g, momentum %g, lamb %g, lr %g, weight_decay %g)", i, r.eps, r.momentum,
                   r.lamb, r.lr, r.weight_decay);
    const bool mom = r.momentum != 0.0;
    const double ck = 1.0 - r.momentum;
    FamTensor t{};
    t.eps = (float)r.eps;
    t.wd = (float)r.weight_decay;
    t.lr = (float)r.lamb;
    t.decay = (float)(1.0 - r.lr * r.weight_decay);
    t.ck = (float)ck;
    t.keep = (float)(1.0 - ck);
    t.flags = (mom ? d2t::FAM_MOMENTUM : 0) | (r.decoupled_decay ? d2t::FAM_DECOUPLED : 0);
    recs[i] = FamRec{r.param, r.grad, r.grad_sum_sq, r.s, mom ? r.x0 : nullptr, r.mirror, "grad_sum_sq", "s", mom ? "x0" : nullptr,
                     r.numel, t};
  }
  hipStream_t s = (hipStream_t)stream;
  FamPlan plan;
  if (int rc = fam_prepare(o, recs, true, clip ? SC_PARTIAL : 0u, s, plan)) return rc;
  if (plan.chunks == 0) {
    if (clip) OHIP(o, hipMemsetAsync(norm_dev, 0, 4, s));
    return D2T_OK;
  }
  if (clip) fam_norm(o, plan, max_grad_norm, 0, norm_dev, s);
  hipLaunchKernelGGL(d2t::madgrad_kernel, dim3((unsigned)plan.chunks), dim3(d2t::OPT_THREADS), 0, s, plan.table, plan.tensors,
                     clip ? o->coef : nullptr);
  OHIP(o, hipGetLastError());
  return D2T_OK;
}

int d2t_optim_lookahead_sync(d2t_optim* o, const d2t_optim_lookahead_tensor* in, int32_t n, float alpha, d2t_stream stream) {
  if (!o) return D2T_EINVAL;
  d2t::OptDevGuard dg_(o);
  if (n < 0 || (n && !in)) return ofail(o, D2T_EINVAL, "bad argument: %d tensors", n);
  if (!(alpha >= 0.f && alpha <= 1.f)) return ofail(o, D2T_EINVAL, "bad scalars (alpha %g)", alpha);
  std::vector<FamRec> recs((size_t)n);
  for (int i = 0; i < n; ++i)
    recs[i] = FamRec{in[i].fast, nullptr, in[i].slow, nullptr, nullptr, in[i].mirror, "slow", nullptr, nullptr, in[i].numel, FamTensor{}};
  hipStream_t s = (hipStream_t)stream;
  FamPlan plan;
  if (int rc = fam_prepare(o, recs, false, 0u, s, plan)) return rc;
  if (plan.chunks == 0) return D2T_OK;
  hipLaunchKernelGGL(d2t::lookahead_kernel, dim3((unsigned)plan.chunks), dim3(d2t::OPT_THREADS), 0, s, plan.table, alpha);
  OHIP(o, hipGetLastError());
  return D2T_OK;
}

}  // extern "C"
