// Shared pieces of the implicit-GEMM convolution kernels (fp32 and bf16x3 variants).
#pragma once
#include "kernels.h"

namespace d2t {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4v = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == ACT_RELU) return fmaxf(v, 0.f);
  if (act == ACT_GELU) return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
  return v;
}

// fp32 <-> split bf16 (hi = upper 16 bits, lo = bf16(x - hi), round to nearest even)
__device__ __forceinline__ float bf16_bits_to_f32(uint16_t b) { return __uint_as_float((unsigned)b << 16); }
__device__ __forceinline__ void split_f32(float x, uint16_t& hi, uint16_t& lo) {
  const unsigned u = __float_as_uint(x);
  hi = (uint16_t)(u >> 16);
  const __bf16 l = (__bf16)(x - __uint_as_float(u & 0xFFFF0000u));
  lo = *reinterpret_cast<const uint16_t*>(&l);
}

// fp16x2 mode (ConvP::f16, round 3): a record holds the activation ONCE, as fp16, in its hi half (the lo half is unused);
// the convolution is x16 * w_lo + x16 * w_hi with the weights as fp16 hi + fp16 lo -- two MFMAs per product instead of three.
// FINITE values beyond the fp16 range saturate (a feature map of a trained model stays far below 65504); NaN and +-Inf pass
// through the conversion unchanged, so a numerically broken forward stays visible in the logits as it does in the other modes
// (fmaxf / fminf alone would turn a NaN into -65504 and the next ReLU into 0).
__device__ __forceinline__ uint16_t f32_to_f16_bits(float x) {
  const float c = fminf(fmaxf(x, -65504.f), 65504.f);
  const _Float16 h = (_Float16)(fabsf(x) <= 3.402823466e38f ? c : x);  // v_cvt_f16_f32: round to nearest even; NaN -> NaN, Inf -> Inf
  return *reinterpret_cast<const uint16_t*>(&h);
}
__device__ __forceinline__ float f16_bits_to_f32(uint16_t b) { return (float)*reinterpret_cast<const _Float16*>(&b); }
// record formats: 0 = bf16 hi | lo (x ~ hi + lo), 1 = ONE fp16 in the hi half (lo half unused), 2 = fp16 hi | fp16 lo (x ~ hi + lo)
enum : int { REC_BF16 = 0, REC_F16 = 1, REC_F16_PAIR = 2 };
__device__ __forceinline__ int out_fmt(const ConvP& p) { return p.out_fmt ? p.out_fmt - 1 : p.f16; }
__device__ __forceinline__ int res_fmt(const ConvP& p) { return p.res_fmt ? p.res_fmt - 1 : p.f16; }
// one element of a record: (hi, lo) <-> fp32
__device__ __forceinline__ void split_rec(float x, uint16_t& hi, uint16_t& lo, int fmt) {
  if (fmt == REC_BF16) { split_f32(x, hi, lo); return; }
  hi = f32_to_f16_bits(x);
  lo = fmt == REC_F16_PAIR ? f32_to_f16_bits(x - f16_bits_to_f32(hi)) : (uint16_t)0;  // (x - hi is exact in fp32)
}
__device__ __forceinline__ float join_rec(uint16_t hi, uint16_t lo, int fmt) {
  if (fmt == REC_BF16) return bf16_bits_to_f32(hi) + bf16_bits_to_f32(lo);
  return fmt == REC_F16_PAIR ? f16_bits_to_f32(hi) + f16_bits_to_f32(lo) : f16_bits_to_f32(hi);
}
// W (4 | 8) consecutive elements of a record, W / 2 packed words per half.  `rec` points at the hi half; the lo half lies 32
// elements further.
template <int W>
using rec_words = unsigned __attribute__((ext_vector_type(W / 2)));
// residual add: v += hi (+ lo).  One-fp16 records: the value is the hi half, the lo half is not read.
template <int W>
__device__ __forceinline__ void add_rec(float (&v)[W], const uint16_t* rec, int fmt) {
  const rec_words<W> h = *reinterpret_cast<const rec_words<W>*>(rec);
  if (fmt == REC_F16) {
#pragma unroll
    for (int e = 0; e < W / 2; ++e) {
      v[2 * e] += f16_bits_to_f32((uint16_t)(h[e] & 0xFFFFu));
      v[2 * e + 1] += f16_bits_to_f32((uint16_t)(h[e] >> 16));
    }
    return;
  }
  const rec_words<W> l = *reinterpret_cast<const rec_words<W>*>(rec + 32);
  if (fmt == REC_F16_PAIR) {
#pragma unroll
    for (int e = 0; e < W / 2; ++e) {
      v[2 * e] += f16_bits_to_f32((uint16_t)(h[e] & 0xFFFFu)) + f16_bits_to_f32((uint16_t)(l[e] & 0xFFFFu));
      v[2 * e + 1] += f16_bits_to_f32((uint16_t)(h[e] >> 16)) + f16_bits_to_f32((uint16_t)(l[e] >> 16));
    }
  } else {
#pragma unroll
    for (int e = 0; e < W / 2; ++e) {
      v[2 * e] += __uint_as_float(h[e] << 16) + __uint_as_float(l[e] << 16);
      v[2 * e + 1] += __uint_as_float(h[e] & 0xFFFF0000u) + __uint_as_float(l[e] & 0xFFFF0000u);
    }
  }
}
// split, pack and store.  The 8-wide store skips the lo half of one-fp16 records (it is never read); the 4-wide store
// writes its zeros.
template <int W>
__device__ __forceinline__ void store_rec(const float (&v)[W], uint16_t* rec, int fmt) {
  rec_words<W> oh, ol;
#pragma unroll
  for (int e = 0; e < W / 2; ++e) {
    uint16_t h0, l0, h1, l1;
    split_rec(v[2 * e], h0, l0, fmt);
    split_rec(v[2 * e + 1], h1, l1, fmt);
    oh[e] = (unsigned)h0 | ((unsigned)h1 << 16);
    ol[e] = (unsigned)l0 | ((unsigned)l1 << 16);
  }
  *reinterpret_cast<rec_words<W>*>(rec) = oh;
  if (W == 4 || fmt != REC_F16) *reinterpret_cast<rec_words<W>*>(rec + 32) = ol;
}
// W consecutive floats (16-byte accesses): the epilogue tile in LDS, bias / residual / positional rows, fp32 output rows
template <int W>
__device__ __forceinline__ void load_tile(const float* src, float (&v)[W]) {
#pragma unroll
  for (int e = 0; e < W; e += 4) {
    const float4 a = *reinterpret_cast<const float4*>(src + e);
    v[e] = a.x, v[e + 1] = a.y, v[e + 2] = a.z, v[e + 3] = a.w;
  }
}
template <int W>
__device__ __forceinline__ void add_row(float (&v)[W], const float* src) {
  float a[W];
  load_tile<W>(src, a);
#pragma unroll
  for (int e = 0; e < W; ++e) v[e] += a[e];
}
template <int W>
__device__ __forceinline__ void store_row(const float (&v)[W], float* dst) {
#pragma unroll
  for (int e = 0; e < W; e += 4) *reinterpret_cast<float4*>(dst + e) = make_float4(v[e], v[e + 1], v[e + 2], v[e + 3]);
}

// Split-activation layout ("planes"): per row and per 32-channel group one 128-byte record
// [32 x hi | 32 x lo] (bf16), so both halves of a K-step's operand share a cache line.
// Index (in uint16 units) of the hi part of element (row, c); the lo part sits 32 elements further.
__device__ __forceinline__ size_t plane_idx(size_t row, int c, int C) {
  return (row * C + (size_t)(c & ~31)) * 2 + (c & 31);
}

// LDS rows of one operand plane are 64 bytes (32 x 16 bit); the 16-byte k-chunk index is XOR-swizzled with (row >> 2) & 3 so
// that the 16-lane groups of a ds_read_b128 of the 32x32x16 fragment pattern touch all 64 banks exactly once
__device__ __forceinline__ int swz_chunk(int row, int c) { return c ^ ((row >> 2) & 3); }

// GEMM row m -> output pixel (b, oh, ow): row-major, or pooled order when a 2x2 max-pool is fused (ConvP::pool2)
__device__ __forceinline__ void row_major_coords(const ConvP& p, int m, int& b, int& oh, int& ow) {
  const int ohow = p.OH * p.OW;
  b = m / ohow;
  const int rem = m - b * ohow;
  oh = rem / p.OW;
  ow = rem - oh * p.OW;
}
__device__ __forceinline__ void conv_row_coords(const ConvP& p, int m, int& b, int& oh, int& ow) {
  if (p.pool2) {
    const int q = m >> 2, sb = m & 3, pw2 = p.OW >> 1, ph2 = p.OH >> 1;
    const int t = q / pw2;
    ow = 2 * (q - t * pw2) + (sb & 1);
    b = t / ph2;
    oh = 2 * (t - b * ph2) + (sb >> 1);
  } else {
    row_major_coords(p, m, b, oh, ow);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The K loop's phases, each written once for the fp32 kernel (conv_mfma.hip), the split-bf16 kernels (conv_bf16x3.hip) and
// the pipelined kernel (conv_bf16x3p.hip).  All of them are inlined, and the callers' register budgets
// decided their form: check the resource table of every kernel of the three sources after touching one.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int XBK = 32;   // K-step
constexpr int XROW = 64;  // bytes per LDS row of one 16-bit plane (32 elements)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// THE K ORDER, and with it the bits, of every convolution: position of the next K-step to fetch.  Taps cycle fastest (kw,
// then kh), then the 32-channel chunk -> the taps of a chunk re-read the same 128-byte channel slices of neighbouring pixels
// back to back (L2 / L1 hits instead of HBM).  SECOND: behind the last chunk the K-steps of a 1x1 second input follow
// (ConvP::in2_hi, c0 - Cin = its channel chunk; wave-uniform).
template <bool SECOND = false>
struct TapCursor {
  int kh = 0, kw = 0, c0 = 0;
  __device__ __forceinline__ bool second(const ConvP& p) const { return SECOND && c0 >= p.Cin; }
  __device__ __forceinline__ int tap(const ConvP& p) const { return kh * p.KW + kw; }  // bit of a row's tap mask
  // element offset of this K-step's 32 channels from the first channel of a row's top-left tap (NHWC) -- or, in the second
  // input, from the first channel of the row
  __device__ __forceinline__ int offset(const ConvP& p) const { return second(p) ? c0 - p.Cin : (kh * p.W + kw) * p.Cin + c0; }
  __device__ __forceinline__ void advance(const ConvP& p) {
    if (second(p)) {
      c0 += 32;
    } else if (++kw == p.KW) {
      kw = 0;
      if (++kh == p.KH) { kh = 0; c0 += 32; }
    }
  }
};

// A GEMM row of the kernels that read fp32 rows: top-left input coordinate of output pixel m and the sample's first pixel
struct F32Row {
  int ih0, iw0, pix;
};
__device__ __forceinline__ F32Row f32_row(const ConvP& p, int m) {
  if (m >= p.M) return {-0x40000000, 0, 0};  // never in range
  int b, oh, ow;
  row_major_coords(p, m, b, oh, ow);
  return {oh * p.SH - p.PH, ow * p.SW - p.PW, b * p.H * p.W};
}

// A GEMM row of the kernels that read records: `off` = element offset (uint16 units) of 16-byte chunk `chunk` of the record
// at the row's top-left tap, first channel chunk (negative in the padding); `mask` = validity over the filter taps (bit
// kh * KW + kw; KH * KW <= 16).  Rows beyond M: no valid tap.
// Through references, not a returned pair: with the pair the pipelined 256 x 128 build, which sits at its register limit,
// came out with 28 instead of 20 bytes of scratch per lane and 2 % more instructions.
__device__ __forceinline__ void rec_row(const ConvP& p, int m, int chunk, int& off, unsigned& mask) {
  off = 0;
  mask = 0;
  if (m < p.M) {
    int b, oh, ow;
    conv_row_coords(p, m, b, oh, ow);
    const int ih0 = oh * p.SH - p.PH, iw0 = ow * p.SW - p.PW;
    off = ((b * p.H + ih0) * p.W + iw0) * p.Cin * 2 + chunk * 8;
    for (int kh = 0; kh < p.KH; ++kh)
      for (int kw = 0; kw < p.KW; ++kw)
        if ((unsigned)(ih0 + kh) < (unsigned)p.H && (unsigned)(iw0 + kw) < (unsigned)p.W) mask |= 1u << (kh * p.KW + kw);
  }
}
// 16-byte chunk `chunk` of K-step 0 of weight row n in the hi / lo planes; nullptr for rows beyond Cout
struct WeightRow {
  const uint16_t* hi;
  const uint16_t* lo;
};
__device__ __forceinline__ WeightRow weight_row(const ConvP& p, int n, int chunk) {
  const bool ok = n < p.Cout;
  return {ok ? p.w_hi + (size_t)n * p.K + chunk * 8 : nullptr, ok ? p.w_lo + (size_t)n * p.K + chunk * 8 : nullptr};
}

template <class A, int MI, int NJ>
__device__ __forceinline__ void zero_acc(A (&acc)[MI][NJ]) {
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = A{};
}

// THE ARITHMETIC CONTRACT: one product of split operands on top of acc -- lo*hi, hi*lo, hi*hi in this order (the dropped
// lo*lo term is ~2^-18 relative), or with F16 (ConvP::f16: a_hi holds the fp16 activation, a_lo is not read, the weights are
// fp16 hi / lo) x*w_lo, x*w_hi.  The only place that spells the order of the MFMAs of a product: "the 256 x 128 kernel and
// its 64 x 128 tail are bit-identical" rests on it.  One overload per MFMA shape (32x32x16: half a K-step, 16x16x32: all of it).
template <bool F16 = false>
__device__ __forceinline__ f32x16 product(f32x16 acc, bf16x8 a_hi, bf16x8 a_lo, bf16x8 b_hi, bf16x8 b_lo) {
  if constexpr (F16) {
    const f16x8 x = __builtin_bit_cast(f16x8, a_hi);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, __builtin_bit_cast(f16x8, b_lo), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(x, __builtin_bit_cast(f16x8, b_hi), acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc, 0, 0, 0);
  }
}
template <bool F16 = false>
__device__ __forceinline__ f32x4v product(f32x4v acc, bf16x8 a_hi, bf16x8 a_lo, bf16x8 b_hi, bf16x8 b_lo) {
  if constexpr (F16) {
    const f16x8 x = __builtin_bit_cast(f16x8, a_hi);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(x, __builtin_bit_cast(f16x8, b_lo), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, __builtin_bit_cast(f16x8, b_hi), acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, b_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_lo, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_hi, acc, 0, 0, 0);
  }
}

// Fragments of the 32x32x16 MFMAs from the swizzled 64-byte-row planes (swz_chunk): N blocks of 32 rows from row0 on, lane
// (r = lane & 31, h = lane >> 5) reads 16-byte chunk c = 2 * kk + h of row r of each block.  LO = false: no lo plane (F16 A operand).
template <bool LO = true, int N>
__device__ __forceinline__ void read_frags32(const unsigned char* hi, const unsigned char* lo, int row0, int c, bf16x8 (&fh)[N], bf16x8 (&fl)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int row = row0 + i * 32;
    const int off = row * XROW + swz_chunk(row, c) * 16;
    fh[i] = *reinterpret_cast<const bf16x8*>(hi + off);
    if (LO) fl[i] = *reinterpret_cast<const bf16x8*>(lo + off);
  }
}

// XCD-aware tile order: consecutive logical tiles (same A rows, neighbouring pixels) run on the
// same XCD so they share its L2 (bijective remap, cdna guide T1).
__device__ __forceinline__ int xcd_logical_tile() {
  const int nwg = gridDim.x, orig = blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (blockIdx.x >> 3);
}

// C/D register maps of the MFMAs: row of register `reg` of a lane in the result block whose first row is `base`.  A lane's
// column in the block is lc, its row group lr -- the kernels hold both already (their fragment reads use them), and
// recomputing them from the lane id here costs the 16x16x32 tail kernels 4 VGPRs and one wave of occupancy.
struct Map32 {  // v_mfma_*_32x32*: lc = lane & 31 -> n, lr = lane >> 5, row = (reg & 3) + 8 * (reg >> 2) + 4 * lr -> m
  using acc_t = f32x16;
  static constexpr int BLK = 32, REGS = 16;
  static __device__ __forceinline__ int row(int base, int lr, int reg) { return base + (reg & 3) + 8 * (reg >> 2) + 4 * lr; }
};
struct Map16 {  // v_mfma_f32_16x16x32_*: lc = lane & 15 -> n, lr = lane >> 4, row = 4 * lr + reg -> m
  using acc_t = f32x4v;
  static constexpr int BLK = 16, REGS = 4;
  static __device__ __forceinline__ int row(int base, int lr, int reg) { return base + 4 * lr + reg; }
};

// What the element-wise epilogue below compiles in, by what a kernel's launcher lets through.
// The 32x32 kernels: records are bf16 hi | lo or, with ConvP::f16, one fp16 -- HERE they never see another format in
// ConvP::out_fmt / res_fmt (launch_conv_bf16x3 rejects a record launch that would bring one to this epilogue; their tile
// epilogue below honours all three through store_rec / add_rec), and the three-way format code costs the fp32 kernel, which
// runs at the VGPR limit, 700 bytes of scratch per lane and half its speed.
struct ElemTwoWay {
  static constexpr bool kv_store = true;
  static __device__ __forceinline__ float res_at(const ConvP& p, size_t ri) {
    return p.f16 ? f16_bits_to_f32(p.res_hi[ri]) : bf16_bits_to_f32(p.res_hi[ri]) + bf16_bits_to_f32(p.res_hi[ri + 32]);
  }
  static __device__ __forceinline__ void split(const ConvP& p, float v, uint16_t& hi, uint16_t& lo) {
    if (p.f16) { hi = f32_to_f16_bits(v); lo = 0; } else split_f32(v, hi, lo);
  }
};
// The pipelined 16x16x32 kernels: all three record formats; no head-split store (launch_conv_bf16x3p rejects it).
struct ElemThreeWay {
  static constexpr bool kv_store = false;
  static __device__ __forceinline__ float res_at(const ConvP& p, size_t ri) { return join_rec(p.res_hi[ri], p.res_hi[ri + 32], res_fmt(p)); }
  static __device__ __forceinline__ void split(const ConvP& p, float v, uint16_t& hi, uint16_t& lo) { split_rec(v, hi, lo, out_fmt(p)); }
};

// Element-wise epilogue of one wave's MI x NJ grid of accumulator blocks whose top-left output element is (mw, nw): bias
// (folded BN), residual, activation, positional-table add, row / head-split remaps.  The layers the tile epilogue below
// does not take (Cout % 32 != 0, head_dim % 4 != 0; in the LDS-DMA kernels also every remap).
template <class Map, class Elem, int MI, int NJ>
__device__ __forceinline__ void conv_epilogue(const ConvP& p, typename Map::acc_t (&acc)[MI][NJ], int mw, int nw, int lc, int lr) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = nw + j * Map::BLK + lc;
    if (n >= p.Cout) continue;
    const float bias = p.bias ? p.bias[n] : 0.f;
    int slab = 0, head = 0, e = 0;
    if (Elem::kv_store && p.store_mode == STORE_KV) {
      const int d = p.kv_heads * p.kv_hd;
      slab = n / d;
      const int within = n - slab * d;
      head = within / p.kv_hd;
      e = within - head * p.kv_hd;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int reg = 0; reg < Map::REGS; ++reg) {
        const int m = Map::row(mw + i * Map::BLK, lr, reg);
        if (m >= p.M) continue;
        float v = acc[i][j][reg] + bias;
        if (Elem::kv_store && p.store_mode == STORE_KV) {
          const int bb = m / p.kv_T, jj = m - bb * p.kv_T;
          p.out[((((size_t)slab * p.kv_B + bb) * p.kv_heads + head) * p.kv_T + jj) * p.kv_hd + e] = v;
          continue;
        }
        size_t row = (size_t)m;
        int in_img = 0;
        if (p.rows_per_img > 0) {
          const int img = m / p.rows_per_img;
          in_img = m - img * p.rows_per_img;
          row = (size_t)img * p.img_stride + p.row_off + in_img;
        }
        const size_t off = row * p.Cout + n;
        if (p.res) v += p.res[off];
        if (p.res_hi) v += Elem::res_at(p, plane_idx(row, n, p.Cout));
        v = apply_act(v, p.act);
        if (p.row_add) v += p.row_add[(size_t)(p.row_add_off + in_img) * p.Cout + n];
        if (p.out_hi) {
          uint16_t hi, lo;
          Elem::split(p, v, hi, lo);
          const size_t oi = plane_idx(row, n, p.Cout);
          p.out_hi[oi] = hi;
          p.out_hi[oi + 32] = lo;
        } else {
          p.out[off] = v;
        }
      }
    }
  }
}

// Tile epilogue for block tiles whose LDS staging area is free after the K loop: the accumulators go through LDS once so
// that a thread afterwards owns W (4 | 8) CONSECUTIVE CHANNELS of one output row, and the residual is read and the result
// written with 8/16-byte accesses instead of one 2-byte (or 4-byte) access per element -- the element-wise epilogue above
// costs a residual layer ~10 % of its run time and dominates the short-K layers.
// Same arithmetic per element, in the same order, as conv_epilogue: v = acc + bias; v += res | (res_hi + res_lo);
// activation; positional add; split.
// LDS tile: fp32 [BM][BN], the 32-float column block XOR-ed with bit 2 of the row so that the two half-waves of an MFMA
// result (rows 4 apart, same columns) hit different banks.
__device__ __forceinline__ int tile_col(int row, int col) { return col ^ (((row >> 2) & 1) << 5); }

// phase one: one wave's MI x NJ accumulator blocks, top-left tile element (wrow, wcol), into the tile
template <class Map, int BN, int MI, int NJ>
__device__ __forceinline__ void acc_to_tile(typename Map::acc_t (&acc)[MI][NJ], float* tile, int wrow, int wcol, int lc, int lr) {
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int reg = 0; reg < Map::REGS; ++reg) {
        const int row = Map::row(wrow + i * Map::BLK, lr, reg);
        tile[row * BN + tile_col(row, wcol + j * Map::BLK + lc)] = acc[i][j][reg];
      }
}

// The three forms of phase two:
//   lean  no row remap, no positional add, no head-split store (wide_epilogue_ok): the LDS-DMA kernels;
//   pool  lean with the fused 2x2 max-pool (ConvP::pool2): tile rows 4r .. 4r+3 are one pooling window (pooled row order of
//         the GEMM's rows), a thread owns W channels of one POOLED row.  max, then bias, then activation = the pool of the
//         activated convolution outputs (both monotone), bit for bit; no residual (the layers in front of a pool have none);
//   full  with the row remap (rows_per_img), the positional-table add and the head-split K/V store, for the kernels whose
//         register budget does not matter (the on-the-fly split-bf16 kernel, the fp32 kernel).  Kept out of the lean form
//         on purpose: with the remap code compiled in, the split-bf16 LDS-DMA kernel needs 107-121 VGPRs instead of 101;
//         above 104 a decode wave no longer fits on a SIMD next to four convolution waves and the decode streams starve
//         (measured: 1139 instead of 1210 formulas/s).
// All need Cout % 32 == 0; the head-split store also head_dim % W == 0.
enum class Epi { lean, pool, full };
// (host too: launch_conv_bf16x3 decides by the same predicate which launches it lets through)
__host__ __device__ __forceinline__ bool wide_epilogue_ok(const ConvP& p) {
  return p.store_mode == STORE_ROWS && p.rows_per_img == 0 && !p.row_add && (p.Cout & 31) == 0;
}
__device__ __forceinline__ bool wide_epilogue_full_ok(const ConvP& p) {
  return (p.Cout & 31) == 0 && (p.store_mode == STORE_ROWS || (p.kv_hd & 3) == 0);
}

// phase two, run by every thread of the block (NT; in the pipelined kernel the loader waves included): LDS reads to global
// stores.  The caller puts a barrier in front (the tile is complete) and behind (the tile is staging memory again).
template <Epi KIND, int W, int BM, int BN, int NT>
__device__ __forceinline__ void tile_rows_epilogue(const ConvP& p, const unsigned char* smem, int m0, int n0, int tid) {
  static_assert(KIND != Epi::full || W == 4, "the head-split store is checked for four channels (wide_epilogue_full_ok)");
  const float* tile = reinterpret_cast<const float*>(smem);
  constexpr int GPR = BN / W;                    // W-channel groups per tile row
  constexpr int RS = KIND == Epi::pool ? 4 : 1;  // tile rows per output row
  const uint16_t* __restrict__ res_hi = p.res_hi;
  const float* __restrict__ res = p.res;
  const float* __restrict__ bias = p.bias;
  uint16_t* __restrict__ out_hi = p.out_hi;
  float* __restrict__ out = p.out;
  // unroll 2, not more: more would cost the registers that let a decode wave share the SIMD with four convolution waves;
  // the pooled loop is not unrolled at all (109-115 instead of 102-108 VGPRs in the LDS-DMA kernels)
#pragma unroll KIND == Epi::pool ? 1 : 2
  for (int idx = tid; idx < (BM / RS) * GPR; idx += NT) {
    const int row = RS * (idx / GPR), g = idx % GPR;
    const int m = m0 + row, n = n0 + g * W;
    if (m >= p.M || n >= p.Cout) continue;
    const float* src = tile + row * BN + tile_col(row, g * W);  // (rows 4 r .. 4 r + 3 share the column XOR)
    float v[W];
    load_tile<W>(src, v);
    if constexpr (KIND == Epi::pool) {
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        float t[W];
        load_tile<W>(src + k * BN, t);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = fmaxf(v[e], t[e]);
      }
    }
    if (bias) add_row<W>(v, bias + n);
    size_t orow = (size_t)(KIND == Epi::pool ? m >> 2 : m);
    int in_img = 0;
    if constexpr (KIND == Epi::full) {
      if (p.store_mode == STORE_KV) {  // n -> (slab, head, e), m -> (b, j): W consecutive e of one head
        const int d = p.kv_heads * p.kv_hd, slab = n / d, within = n - slab * d;
        const int head = within / p.kv_hd, e = within - head * p.kv_hd;
        const int bb = m / p.kv_T, jj = m - bb * p.kv_T;
        store_row<W>(v, out + ((((size_t)slab * p.kv_B + bb) * p.kv_heads + head) * p.kv_T + jj) * p.kv_hd + e);
        continue;
      }
      if (p.rows_per_img > 0) {
        const int img = m / p.rows_per_img;
        in_img = m - img * p.rows_per_img;
        orow = (size_t)img * p.img_stride + p.row_off + in_img;
      }
    }
    const size_t off = orow * p.Cout + n;
    const size_t pi = plane_idx(orow, n, p.Cout);
    if constexpr (KIND != Epi::pool) {
      if (res) add_row<W>(v, res + off);
      if (res_hi) add_rec<W>(v, res_hi + pi, res_fmt(p));
    }
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] = apply_act(v[e], p.act);
    if constexpr (KIND == Epi::full) {
      if (p.row_add) add_row<W>(v, p.row_add + (size_t)(p.row_add_off + in_img) * p.Cout + n);
    }
    if (out_hi) store_rec<W>(v, out_hi + pi, out_fmt(p));
    else store_row<W>(v, out + off);
  }
}

// both phases for the kernels whose every wave holds accumulators (four channels per thread)
template <Epi KIND, int BM, int BN, int NT, int MI, int NJ>
__device__ __forceinline__ void conv_epilogue_tile(const ConvP& p, f32x16 (&acc)[MI][NJ], unsigned char* smem, int m0, int n0,
                                                   int wrow, int wcol, int lc, int lr, int tid) {
  acc_to_tile<Map32, BN>(acc, reinterpret_cast<float*>(smem), wrow, wcol, lc, lr);
  __syncthreads();
  tile_rows_epilogue<KIND, 4, BM, BN, NT>(p, smem, m0, n0, tid);
  __syncthreads();  // the tile is staging memory again (next tile's LDS-DMA)
}

}  // namespace d2t
