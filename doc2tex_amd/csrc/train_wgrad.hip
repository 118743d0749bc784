// Weight gradients of the training step (train.hip), all accumulated in fp32:
//
//   wgrad_kernel          Conv2d / Linear: the "TN" GEMM  dW[co][tap][ci] = sum_p dz[p][co] * x[p+tap][ci] on the fp32 MFMA,
//                         split over pixel chunks (deterministic two-pass reduction)
//   wgrad_bf16x3_kernel   the same GEMM in split-bf16 arithmetic (conv_precision = bf16x3), operands split on the fly
//   wgrad_rec_kernel      ... on operand records that already exist (the convolutions between BatchNorm layers), by LDS-DMA
//   wgrad_reduce_*        second pass: the sum over the chunks
//   stem_wgrad_kernel     the stem convolution (one or three image channels)
//
// The three GEMM kernels share their block coordinates (WgradBlock), the pixel -> input-row geometry (wgrad_src_row), the
// transposing fragment read (frag_tr16) and the accumulator store (wgrad_store_tile; conv_common.h zero_acc).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_common.h"
#include "kernels.h"

namespace d2t {

// what block (x, y, z) of a wgrad grid works on: tile origin, filter tap, pixel-row chunk, its slice of p.part
template <int BM, int BN>
struct WgradBlock {
  int m0, n0, tap, kh, kw;
  long long r_begin, r_end;
  __device__ __forceinline__ explicit WgradBlock(const WgradP& p) {
    const int tiles_n = (p.N + BN - 1) / BN;
    m0 = (blockIdx.x / tiles_n) * BM; n0 = (blockIdx.x % tiles_n) * BN;
    tap = blockIdx.y; kh = tap / p.KW; kw = tap % p.KW;
    r_begin = (long long)blockIdx.z * p.chunk;
    r_end = r_begin + p.chunk < p.P ? r_begin + p.chunk : p.P;
  }
  // the [M][N] partial of (chunk, tap)
  __device__ __forceinline__ float* out(const WgradP& p) const { return p.part + ((size_t)blockIdx.z * p.taps + tap) * p.M * p.N; }
  __device__ __forceinline__ int steps(int BK) const { return (int)((r_end - r_begin + BK - 1) / BK); }
};
// row of p.b that output pixel r reads under filter tap (kh, kw); ok = false: it lies in the padding
__device__ __forceinline__ long long wgrad_src_row(const WgradP& p, long long r, int kh, int kw, bool& ok) {
  ok = true;
  if (!p.geom) return r;
  const int ohow = p.OH * p.OW;
  const int b = (int)(r / ohow), rem = (int)(r - (long long)b * ohow);
  const int oh = rem / p.OW, ow = rem - oh * p.OW;
  const int ih = oh * p.SH - p.PH + kh, iw = ow * p.SW - p.PW + kw;
  ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
  return ((long long)b * p.H + ih) * p.W + iw;
}
// a wave's MI x NJ accumulators of 32 x 32 (MFMA layout: lane = column r + 32 h, register -> row) to out[M][N] from
// (mw, nw) on; GUARD: the tile may reach past M / N
template <int MI, int NJ, bool GUARD>
__device__ __forceinline__ void wgrad_store_tile(const f32x16 (&acc)[MI][NJ], float* out, int M, int N, int mw, int nw, int r, int h) {
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = nw + j * 32 + r;
      if (GUARD && n >= N) continue;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int m = mw + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (!GUARD || m < M) out[(size_t)m * N + n] = acc[i][j][reg];
      }
    }
}

// ---------------------------------------------------------------------------
// wgrad: out[z][tap][m][n] = sum_{p in chunk z} A[p][m] * X[src(p, tap)][n]
// Block tile BM x BN, 4 waves (2x2), K-step = 32 rows; both operand tiles are stored [k][col] in LDS exactly as
// they lie in memory (rows = pixels, contiguous channels), and v_mfma_f32_32x32x2_f32 wants A[i][k] / B[k][j] with
// i, j = lane & 31: consecutive lanes read consecutive floats of one LDS row -> conflict-free ds_read_b32.
// ---------------------------------------------------------------------------
template <int BM, int BN>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradP p) {
  constexpr int BK = 32;
  constexpr int WTM = BM / 2, WTN = BN / 2, MI = WTM / 32, NJ = WTN / 32;
  constexpr int AV = BM / 4, BV = BN / 4;               // float4 per tile row
  constexpr int ALD = (BK * AV) / 256, BLD = (BK * BV) / 256;  // float4 loads per thread per stage
  static_assert(ALD >= 1 && BLD >= 1, "tile too small");
  __shared__ __attribute__((aligned(16))) float As[2][BK][BM];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const WgradBlock<BM, BN> blk(p);
  const int m0 = blk.m0, n0 = blk.n0;
  const long long r_begin = blk.r_begin, r_end = blk.r_end;

  float4 ra[ALD], rb[BLD];
  auto fetch = [&](long long r0) {
#pragma unroll
    for (int i = 0; i < ALD; ++i) {
      const int idx = tid + i * 256, row = idx / AV, c4 = (idx % AV) * 4;
      const long long r = r0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < r_end && m0 + c4 < p.M) v = *reinterpret_cast<const float4*>(p.a + r * p.lda + m0 + c4);
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < BLD; ++i) {
      const int idx = tid + i * 256, row = idx / BV, c4 = (idx % BV) * 4;
      const long long r = r0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < r_end && n0 + c4 < p.N) {
        bool ok;
        const long long src = wgrad_src_row(p, r, blk.kh, blk.kw, ok);
        if (ok) v = *reinterpret_cast<const float4*>(p.b + src * p.ldb + n0 + c4);
      }
      rb[i] = v;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < ALD; ++i) {
      const int idx = tid + i * 256, row = idx / AV, c4 = (idx % AV) * 4;
      *reinterpret_cast<float4*>(&As[buf][row][c4]) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < BLD; ++i) {
      const int idx = tid + i * 256, row = idx / BV, c4 = (idx % BV) * 4;
      *reinterpret_cast<float4*>(&Bs[buf][row][c4]) = rb[i];
    }
  };

  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  f32x16 acc[MI][NJ];
  zero_acc(acc);

  const int steps = blk.steps(BK);
  if (steps > 0) {
    fetch(r_begin);
    stash(0);
  }
  __syncthreads();
  for (int st = 0; st < steps; ++st) {
    const int cur = st & 1;
    if (st + 1 < steps) fetch(r_begin + (long long)(st + 1) * BK);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      float fa[MI], fb[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[i] = As[cur][2 * kk + h][wm * WTM + i * 32 + r];
#pragma unroll
      for (int j = 0; j < NJ; ++j) fb[j] = Bs[cur][2 * kk + h][wn * WTN + j * 32 + r];
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (st + 1 < steps) stash(cur ^ 1);
    __syncthreads();
  }
  wgrad_store_tile<MI, NJ, true>(acc, blk.out(p), p.M, p.N, m0 + wm * WTM, n0 + wn * WTN, r, h);
}

// ---------------------------------------------------------------------------
// Split-bf16 weight gradient (conv_precision = bf16x3): the same TN GEMM on v_mfma_f32_32x32x16_bf16 with
// dz = hi + lo, x = hi + lo and three MFMAs per product.  Both operand tiles stay pixel-major in LDS (rows = pixels,
// exactly as they are loaded and split); the MFMA wants, per lane, eight consecutive K (= pixel) values of ONE column,
// which is what gfx950's transposing LDS read delivers: ds_read_b64_tr_b16 hands lane i of a 16-lane group column i of
// a 4-row x 16-column block.  Two of them per fragment.  LDS rows are 320 B (256 B of data + 64 B pad): a 32-lane
// half reads 4 rows x 64 B, and a row stride of 64 (mod 256) bytes makes those 256 bytes hit all 64 banks once.
// Block tile 128 x 128, 4 waves (wave tile 64 x 64), K-step = 16 pixels, double-buffered, 40 KB of LDS.
// ---------------------------------------------------------------------------
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short s4_t __attribute__((ext_vector_type(4)));
typedef short s8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s4_t* lds_s4_ptr;

// one MFMA operand fragment (eight consecutive K values of this lane's column) from a [K][column] bf16 tile in LDS: two
// transposing reads, K rows +0..3 at q and +4..7 four rows (of row_bytes) further down
__device__ __forceinline__ bf16x8_t frag_tr16(const unsigned char* q, int row_bytes) {
  const s4_t lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(q));
  const s4_t hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(q + 4 * row_bytes));
  s8_t v = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}

__device__ __forceinline__ void split4_bf16(const float4 v, uint2& hi, uint2& lo) {
  const unsigned x0 = __float_as_uint(v.x), x1 = __float_as_uint(v.y), x2 = __float_as_uint(v.z), x3 = __float_as_uint(v.w);
  hi.x = (x0 >> 16) | (x1 & 0xFFFF0000u);
  hi.y = (x2 >> 16) | (x3 & 0xFFFF0000u);
  const __bf16 l0 = (__bf16)(v.x - __uint_as_float(x0 & 0xFFFF0000u)), l1 = (__bf16)(v.y - __uint_as_float(x1 & 0xFFFF0000u));
  const __bf16 l2 = (__bf16)(v.z - __uint_as_float(x2 & 0xFFFF0000u)), l3 = (__bf16)(v.w - __uint_as_float(x3 & 0xFFFF0000u));
  lo.x = (unsigned)*reinterpret_cast<const unsigned short*>(&l0) | ((unsigned)*reinterpret_cast<const unsigned short*>(&l1) << 16);
  lo.y = (unsigned)*reinterpret_cast<const unsigned short*>(&l2) | ((unsigned)*reinterpret_cast<const unsigned short*>(&l3) << 16);
}

__global__ __launch_bounds__(256) void wgrad_bf16x3_kernel(const WgradP p) {
  constexpr int BM = 128, BN = 128, BK = 16, LDR = 160;  // LDR: uint16 per LDS row (320 B)
  constexpr int PLANE = BK * LDR;                         // uint16 per plane per stage
  __shared__ __attribute__((aligned(16))) unsigned short sm[2][4][PLANE];  // [stage][A_hi, A_lo, B_hi, B_lo]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const WgradBlock<BM, BN> blk(p);
  const int m0 = blk.m0, n0 = blk.n0;
  const long long r_begin = blk.r_begin, r_end = blk.r_end;
  // staging: 16 rows x 32 float4 per operand = 512 float4 -> two per thread
  float4 ra[2], rb[2];
  auto fetch = [&](long long r0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256, row = idx >> 5, c4 = (idx & 31) * 4;
      const long long r = r0 + row;
      float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
      if (r < r_end) {
        if (m0 + c4 < p.M) va = *reinterpret_cast<const float4*>(p.a + r * p.lda + m0 + c4);
        if (n0 + c4 < p.N) {
          bool ok;
          const long long src = wgrad_src_row(p, r, blk.kh, blk.kw, ok);
          if (ok) vb = *reinterpret_cast<const float4*>(p.b + src * p.ldb + n0 + c4);
        }
      }
      ra[i] = va; rb[i] = vb;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256, row = idx >> 5, c4 = (idx & 31) * 4;
      uint2 hi, lo;
      split4_bf16(ra[i], hi, lo);
      *reinterpret_cast<uint2*>(&sm[buf][0][row * LDR + c4]) = hi;
      *reinterpret_cast<uint2*>(&sm[buf][1][row * LDR + c4]) = lo;
      split4_bf16(rb[i], hi, lo);
      *reinterpret_cast<uint2*>(&sm[buf][2][row * LDR + c4]) = hi;
      *reinterpret_cast<uint2*>(&sm[buf][3][row * LDR + c4]) = lo;
    }
  };
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  // transposing read: group g = lane / 16 covers columns 16 (g & 1) .. +15 of a 32-column fragment and K rows 8 (g >> 1) .. +7
  const int g = lane >> 4, l16 = lane & 15;
  const int tr_off = ((8 * (g >> 1) + (l16 >> 2)) * LDR + 16 * (g & 1) + 4 * (l16 & 3));  // uint16 units, rows +0..3
  auto frag = [&](const unsigned short* plane, int col0) -> bf16x8_t {
    return frag_tr16(reinterpret_cast<const unsigned char*>(plane + tr_off + col0), LDR * 2);
  };
  f32x16 acc[2][2];
  zero_acc(acc);
  const int steps = blk.steps(BK);
  if (steps > 0) { fetch(r_begin); stash(0); }
  __syncthreads();
  for (int st = 0; st < steps; ++st) {
    const int cur = st & 1;
    if (st + 1 < steps) fetch(r_begin + (long long)(st + 1) * BK);
    bf16x8_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ah[i] = frag(sm[cur][0], wm * 64 + i * 32);
      al[i] = frag(sm[cur][1], wm * 64 + i * 32);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bh[j] = frag(sm[cur][2], wn * 64 + j * 32);
      bl[j] = frag(sm[cur][3], wn * 64 + j * 32);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
      }
    if (st + 1 < steps) stash(cur ^ 1);
    __syncthreads();
  }
  wgrad_store_tile<2, 2, true>(acc, blk.out(p), p.M, p.N, m0 + wm * 64, n0 + wn * 64, r, h);
}

// ---------------------------------------------------------------------------
// Split-bf16 weight gradient on operand RECORDS (the convolution layers whose dz and input already exist as
// [pixel][32 x hi | 32 x lo] records: the BatchNorm kernels write them for the forward / data-gradient convolutions).
// Same products as wgrad_bf16x3_kernel -- lo*hi, hi*lo, hi*hi into one fp32 accumulator -- but nothing is split or staged
// through registers: a K-step's 16 pixel rows of both operands travel global -> LDS by LDS-DMA (16 bytes per lane), three
// stages deep with a counted vmcnt wait and ONE raw barrier per step (the scheme of conv_bf16x3p.hip), and three blocks
// share a CU so that one block's barrier is covered by the others' MFMAs.
//   LDS stage = A [16 rows][512 B] | B [16 rows][512 B]; a row = the tile's four records of one pixel = 32 chunks of
//   16 bytes (chunk 8 g + 0..3: hi of group g, 8 g + 4..7: lo).  Row stride 512 B puts every row on the same banks, so
//   chunk c of row r is stored at position c ^ ((r & 3) << 2): the four rows of a transposing read (ds_read_b64_tr_b16:
//   4 rows x 64 B per 32 lanes) then start 64 B apart modulo 256 B and cover the 64 banks once.  The LDS-DMA writes lane
//   l of a wave at base + 16 l, so the swizzle is applied on the SOURCE side: the lane fetches the chunk that belongs at
//   its position.
// ---------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_void_ptr;
template <int N>
__device__ __forceinline__ void wg_wait_vm() {
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}

// chunk swizzle of an LDS row of ROWB bytes: the four consecutive rows of a transposing read must start in four different
// 64-byte slots modulo 256 bytes.  Rows of 256 bytes or more all start in the same slot: XOR the row's low two bits into
// bits 2-3 of the chunk index; 128-byte rows alternate between two slots: flip bit 2 (hi <-> lo half) on rows 2, 3 mod 4.
template <int ROWB>
__device__ __forceinline__ int wg_swz(int row) {
  static_assert(ROWB >= 128, "a row holds at least one record");
  return ROWB >= 256 ? (row & 3) << 2 : ((row >> 1) & 1) << 2;
}

template <int MI, int NJ, int WM, int WN, int ABL = 0>
// (ABL: timing probes -- 1 no MFMAs, 2 no fragment reads, 3 no LDS-DMA, 4 plain ds_read_b64, 5 the step's LDS-DMA issued
// in one burst behind the barrier)
// wave tile (32 MI) x (32 NJ), WM x WN waves.  <4,2,2,4> 256 x 256 with 512 threads, one block per CU (a third less
// L2 -> LDS traffic per MFMA than 256 x 128); <4,2,2,2> 256 x 128, two; <2,2,2,2> 128 x 128, three; and for the narrow
// layers at the front of the network <2,2,2,1> 128 x 64 (two waves) and <2,1,1,1> 64 x 32 (one wave)
// (second launch bound = waves per SIMD the register budget must allow: 3 for the 128 x 128 tile, 2 otherwise)
__global__ __launch_bounds__(64 * WM * WN, WM * WN == 4 && MI == 2 ? 3 : 2)
void wgrad_rec_kernel(const WgradP p) {
  constexpr int BK = 16, NS = 3, BM = 32 * MI * WM, BN = 32 * NJ * WN, NT = 64 * WM * WN;
  constexpr int AROWB = BM * 4, BROWB = BN * 4;      // bytes per LDS row: the tile's records of one pixel
  constexpr int AOPB = BK * AROWB, BOPB = BK * BROWB, STAGE = AOPB + BOPB;
  constexpr int ACH = AROWB / 16, BCH = BROWB / 16;  // 16-byte chunks per row
  constexpr int ARPI = NT / ACH, ANI = BK / ARPI;    // rows per block-wide DMA instruction, instructions per step
  constexpr int BRPI = NT / BCH, BNI = BK / BRPI;
  constexpr int PIECES = ANI + BNI, IBYTES = NT * 16;
  static_assert(ARPI % 4 == 0 && BRPI % 4 == 0, "the source-side swizzle needs (row + k RPI) & 3 == row & 3");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * STAGE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const WgradBlock<BM, BN> blk(p);  // (N % BN == 0 here)
  const int m0 = blk.m0, n0 = blk.n0, kh = blk.kh, kw = blk.kw;
  const long long r_begin = blk.r_begin, r_end = blk.r_end;
  const int KT = blk.steps(BK);
  const unsigned char* zero = reinterpret_cast<const unsigned char*>(p.zero) + (lane & 15) * 16;

  // ---- LDS-DMA source side.  A: rows arow + ARPI i (i < ANI) of every stage, chunk position acpos; B: rows brow + BRPI i ----
  const int arow = tid / ACH, acpos = tid % ACH, brow = tid / BCH, bcpos = tid % BCH;
  const int acsrc = acpos ^ wg_swz<AROWB>(arow), bcsrc = bcpos ^ wg_swz<BROWB>(brow);
  const size_t arow_b = (size_t)p.M * 4, brow_b = (size_t)p.N * 4;  // bytes per pixel row of the record arrays
  const unsigned char* a_src = reinterpret_cast<const unsigned char*>(p.a_rec) + (size_t)(r_begin + arow) * arow_b +
                               (size_t)(m0 / 32 + (acsrc >> 3)) * 128 + (acsrc & 7) * 16;
  const unsigned char* b_base = reinterpret_cast<const unsigned char*>(p.b_rec) + (size_t)(n0 / 32 + (bcsrc >> 3)) * 128 + (bcsrc & 7) * 16;
  long long rr = r_begin;  // first pixel row of the step about to be issued
  int pb[BNI], poh[BNI], pow_[BNI];
#pragma unroll
  for (int i = 0; i < BNI; ++i) {
    const long long r = r_begin + brow + BRPI * i;
    const int ohow = p.OH * p.OW;
    pb[i] = (int)(r / ohow);
    const int rem = (int)(r - (long long)pb[i] * ohow);
    poh[i] = rem / p.OW;
    pow_[i] = rem - poh[i] * p.OW;
  }
  long long rrb = r_begin;
  // one LDS-DMA instruction of the stage: pieces 0 .. ANI-1 = the A rows, ANI .. ANI+BNI-1 = the B rows
  auto issue_piece = [&](int stage, int k) {
    unsigned char* sa = smem + stage * STAGE + wave * 1024;  // wave-uniform bases; the hardware adds 16 * lane
    if (k < ANI) {
      const bool live = rr + arow + ARPI * k < r_end;
      const unsigned char* as = live ? a_src + (size_t)(ARPI * k) * arow_b : zero;
      __builtin_amdgcn_global_load_lds(as, (lds_void_ptr)(sa + k * IBYTES), 16, 0, 0);
      if (k == ANI - 1) { a_src += (size_t)BK * arow_b; rr += BK; }
    } else {
      const int i = k - ANI;
      const bool live = rrb + brow + BRPI * i < r_end;
      const int ih = poh[i] * p.SH - p.PH + kh, iw = pow_[i] * p.SW - p.PW + kw;
      const bool ok = live && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      const unsigned char* bs = ok ? b_base + ((size_t)((long long)pb[i] * p.H + ih) * p.W + iw) * brow_b : zero;
      __builtin_amdgcn_global_load_lds(bs, (lds_void_ptr)(sa + AOPB + i * IBYTES), 16, 0, 0);
      pow_[i] += BK;  // advance to the same piece of the next step
      while (pow_[i] >= p.OW) {
        pow_[i] -= p.OW;
        if (++poh[i] == p.OH) { poh[i] = 0; ++pb[i]; }
      }
      if (i == BNI - 1) rrb += BK;
    }
  };
  auto issue = [&](int stage) {
#pragma unroll
    for (int k = 0; k < PIECES; ++k) issue_piece(stage, k);
  };

  // ---- fragment side ----
  const int wm = wave / WN, wn = wave % WN, r = lane & 31, h = lane >> 5;
  const int g16 = lane >> 4, l16 = lane & 15;
  // (the second transposing read of a fragment is four rows further down: same swizzle term)
  const int frow = 8 * (g16 >> 1) + (l16 >> 2), fsub = (g16 & 1) * 2 + ((l16 & 3) >> 1);
  const int fxa = wg_swz<AROWB>(frow), fxb = wg_swz<BROWB>(frow);
  int offa[MI][2], offb[NJ][2];  // [fragment][hi, lo]
#pragma unroll
  for (int part = 0; part < 2; ++part) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
      offa[i][part] = frow * AROWB + (l16 & 1) * 8 + (((((wm * MI + i) << 3) | (part << 2) | fsub) ^ fxa) << 4);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      offb[j][part] = AOPB + frow * BROWB + (l16 & 1) * 8 + (((((wn * NJ + j) << 3) | (part << 2) | fsub) ^ fxb) << 4);
  }
  auto frag = [&](const unsigned char* q, int rowb) -> bf16x8_t {
    if (ABL == 4) {
      const s4_t a4 = *reinterpret_cast<const s4_t*>(q), b4 = *reinterpret_cast<const s4_t*>(q + 4 * rowb);
      s8_t v = {a4[0], a4[1], a4[2], a4[3], b4[0], b4[1], b4[2], b4[3]};
      return __builtin_bit_cast(bf16x8_t, v);
    }
    return frag_tr16(q, rowb);
  };
  f32x16 acc[MI][NJ];
  zero_acc(acc);

  if (KT > 0) issue(0);
  if (KT > 1) issue(1);
  int cur = 0, nxt2 = 2;
  constexpr bool burst = ABL == 3 || ABL == 5;
  bf16x8_t ah[MI], al[MI], bh[NJ], bl[NJ];
  for (int kt = 0; kt < KT; ++kt) {
    if (kt + 1 < KT) wg_wait_vm<PIECES>(); else wg_wait_vm<0>();  // this wave's pieces of step kt have landed
    __builtin_amdgcn_s_barrier();  // ... and everybody else's; nobody reads stage kt-1 any more
    if (burst && kt + 2 < KT && (ABL != 3 || kt + 2 < 3)) issue(nxt2);
    __builtin_amdgcn_sched_barrier(0);
    const unsigned char* st = smem + cur * STAGE;
    if (ABL != 2 || kt == 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        bh[j] = frag(st + offb[j][0], BROWB);
        bl[j] = frag(st + offb[j][1], BROWB);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        ah[i] = frag(st + offa[i][0], AROWB);
        al[i] = frag(st + offa[i][1], AROWB);
      }
    }
    if (ABL == 1) {
#pragma unroll
      for (int i = 0; i < MI; ++i) asm volatile("" ::"v"(ah[i]), "v"(al[i]));
#pragma unroll
      for (int j = 0; j < NJ; ++j) asm volatile("" ::"v"(bh[j]), "v"(bl[j]));
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (ABL != 1 || kt == 0) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
        // the LDS-DMA of step kt+2: one instruction behind each (i, j) group of MFMAs, the last PIECES groups of the step.
        // (In one burst behind the barrier the waves of a block queue up in the vector-memory path together and the
        // MFMAs wait behind them: 951 us on the dominant layer against 833 us this way; all at once after the first /
        // second row of groups: 867 / 847 us.)
        // The narrow tiles have more pieces than groups: PPG pieces behind each group from the first on.
        if (!burst && kt + 2 < KT) {
          constexpr int GROUPS = MI * NJ, PPG = (PIECES + GROUPS - 1) / GROUPS;
          constexpr int first = PPG == 1 ? GROUPS - PIECES : 0;
          const int g = i * NJ + j - first;
          if (g >= 0) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < PPG; ++q)
              if (g * PPG + q < PIECES) issue_piece(nxt2, g * PPG + q);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the fragment reads have returned before the next barrier (WAR on the stage)
    cur = cur == 2 ? 0 : cur + 1;
    nxt2 = nxt2 == 2 ? 0 : nxt2 + 1;
  }
  wgrad_store_tile<MI, NJ, false>(acc, blk.out(p), p.M, p.N, m0 + wm * 32 * MI, n0 + wn * 32 * NJ, r, h);
}

// The record kernel's tiles, widest first.  slots = blocks the device holds at once (256 CUs x blocks per CU by LDS and
// registers): train.hip sizes the split over pixel chunks by it.
#define D2T_REC_TILE(MI, NJ, WM, WN, SLOTS) \
  { 32 * MI * WM, 32 * NJ * WN, 64 * WM * WN, SLOTS, wgrad_rec_kernel<MI, NJ, WM, WN, 0> }
static const WgradRecTile REC_256x256 = D2T_REC_TILE(4, 2, 2, 4, 256), REC_256x128 = D2T_REC_TILE(4, 2, 2, 2, 512),
                          REC_128x128 = D2T_REC_TILE(2, 2, 2, 2, 768),
                          REC_128x64 = D2T_REC_TILE(2, 2, 2, 1, 1024),  // Cin = 64
                          REC_64x32 = D2T_REC_TILE(2, 1, 1, 1, 2048);   // conv0_2: 32 -> 64 channels
#undef D2T_REC_TILE
// (probe builds: D2T_WGRAD_WIDE = 0 / 1 caps the three wide tiles at 128 x 128 / 256 x 128, D2T_WGRAD_NARROW = 0 takes the
// two narrow ones away)
const WgradRecTile* wgrad_rec_tile(int M, int N) {
  static const int mode = D2T_PROBE_ENV_STR("D2T_WGRAD_WIDE") ? D2T_PROBE_ENV("D2T_WGRAD_WIDE") : 2;
  static const bool narrow = !(D2T_PROBE_ENV_STR("D2T_WGRAD_NARROW") && D2T_PROBE_ENV("D2T_WGRAD_NARROW") == 0);
  if (M % 128 == 0 && N % 128 == 0) {
    if (mode >= 2 && M % 256 == 0 && N % 256 == 0) return &REC_256x256;
    if (mode >= 1 && M % 256 == 0) return &REC_256x128;
    return &REC_128x128;
  }
  if (narrow && M % 128 == 0 && N == 64) return &REC_128x64;
  if (narrow && M == 64 && N == 32) return &REC_64x32;
  return nullptr;
}
hipError_t launch_wgrad(const WgradP& p, hipStream_t s) {
  if (p.M <= 0 || p.N <= 0 || p.P <= 0) return hipSuccess;
  if (p.M % 4 || p.N % 4 || p.lda % 4 || p.ldb % 4 || p.S < 1 || p.chunk < 1 || p.taps < 1) return hipErrorInvalidValue;
  if (p.a_rec) {  // record operands
    const WgradRecTile* t = wgrad_rec_tile(p.M, p.N);
    if (!p.b_rec || !p.zero || !p.geom || !p.bf16x3 || !t || p.chunk % 16) return hipErrorInvalidValue;
    void (*kernel)(const WgradP) = t->kernel;
#ifdef D2T_PROBES  // D2T_WGRAD_ABL = 1 .. 5: the timing probes of the 256 x 128 tile
    static void (*const abl[6])(const WgradP) = {nullptr, wgrad_rec_kernel<4, 2, 2, 2, 1>, wgrad_rec_kernel<4, 2, 2, 2, 2>,
                                                 wgrad_rec_kernel<4, 2, 2, 2, 3>, wgrad_rec_kernel<4, 2, 2, 2, 4>,
                                                 wgrad_rec_kernel<4, 2, 2, 2, 5>};
    static const int which = D2T_PROBE_ENV("D2T_WGRAD_ABL");
    if (t == &REC_256x128 && which >= 1 && which <= 5) kernel = abl[which];
#endif
    hipLaunchKernelGGL(kernel, dim3((p.M / t->bm) * (p.N / t->bn), p.taps, p.S), dim3(t->threads), 0, s, p);
  } else if (p.M <= 64 || p.N <= 64) {
    dim3 grid(((p.M + 63) / 64) * ((p.N + 63) / 64), p.taps, p.S);
    hipLaunchKernelGGL((wgrad_kernel<64, 64>), grid, dim3(256), 0, s, p);
  } else {
    dim3 grid(((p.M + 127) / 128) * ((p.N + 127) / 128), p.taps, p.S);
    if (p.bf16x3) hipLaunchKernelGGL(wgrad_bf16x3_kernel, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((wgrad_kernel<128, 128>), grid, dim3(256), 0, s, p);
  }
  return hipGetLastError();
}

// dst = (accumulate ? dst : 0) + sum_z part[z][tap][m][n];  layout 0: dst[m][n] (taps == 1);  layout 1: OIHW dst[m][n][tap]
__global__ void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dst, int S, int taps, int M, int N,
                                    int layout, int accumulate) {
  const size_t total = (size_t)taps * M * N;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    float v = 0.f;
#pragma unroll 8
    for (int z = 0; z < S; ++z) v += part[(size_t)z * total + i];
    const int n = (int)(i % N), m = (int)((i / N) % M), tap = (int)(i / ((size_t)M * N));
    const size_t o = layout == 1 ? ((size_t)m * N + n) * taps + tap : (size_t)m * N + n;
    dst[o] = accumulate ? dst[o] + v : v;
  }
}
// few outputs, many partials (the stem's 288 filter taps over ~2000 pixel chunks, conv0_2's 18432 over 227): one block per output, its 256 threads
// take every 256th partial and a fixed-order tree adds them (a thread per output would walk the partials serially)
__global__ __launch_bounds__(256) void wgrad_reduce_small_kernel(const float* __restrict__ part, float* __restrict__ dst, int S,
                                                                 int taps, int M, int N, int layout, int accumulate) {
  __shared__ float red[256];
  const size_t total = (size_t)taps * M * N, i = blockIdx.x;
  float v = 0.f;
  for (int z = threadIdx.x; z < S; z += 256) v += part[(size_t)z * total + i];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int n = (int)(i % N), m = (int)((i / N) % M), tap = (int)(i / ((size_t)M * N));
    const size_t o = layout == 1 ? ((size_t)m * N + n) * taps + tap : (size_t)m * N + n;
    dst[o] = accumulate ? dst[o] + red[0] : red[0];
  }
}
hipError_t launch_wgrad_reduce(const float* part, float* dst, int S, int taps, int M, int N, int layout, int accumulate,
                               hipStream_t s) {
  const size_t total = (size_t)taps * M * N;
  if ((total <= 4096 && S >= 256) || (total <= 65536 && S >= 128)) {
    hipLaunchKernelGGL(wgrad_reduce_small_kernel, dim3((unsigned)total), dim3(256), 0, s, part, dst, S, taps, M, N, layout,
                       accumulate);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, part,
                     dst, S, taps, M, N, layout, accumulate);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Stem convolution (Cin = 1 or 3, 3x3, pad 1; forward: stem_raw_kernel, train_kernels.hip): dW[co][ci][kh][kw] =
// sum_p dz[p][co] * x[ci][p + tap], the image NCHW planar, tap = (ci * 3 + kh) * 3 + kw in the OIHW order of the weights.
// part[chunk][tap][co]: chunked over pixels; reduced by launch_wgrad_reduce with M = Cout, N = 1 ... (taps = 9 * CIN)
// ---------------------------------------------------------------------------
template <int CO, int CIN>  // output channels: 32 (ResNet conv0_1) or 64 (VGG's first convolution); image channels 1 or 3
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ img, const float* __restrict__ dz,
                                                         float* __restrict__ part, int B, int H, int W, int chunk) {
  // thread -> (co = tid % CO, pixel lane = tid / CO)
  constexpr int NPL = 256 / CO, K = 9 * CIN;
  __shared__ float red[NPL][K][CO];
  const int co = threadIdx.x % CO, pl = threadIdx.x / CO;
  const long long P = (long long)B * H * W;
  const long long r0 = (long long)blockIdx.x * chunk, r1 = r0 + chunk < P ? r0 + chunk : P;
  float acc[K];
#pragma unroll
  for (int t = 0; t < K; ++t) acc[t] = 0.f;
  for (long long r = r0 + pl; r < r1; r += NPL) {
    const int x = (int)(r % W), y = (int)((r / W) % H);
    const long long b = r / ((long long)W * H);
    const float g = dz[(size_t)r * CO + co];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ih = y + kh - 1, iw = x + kw - 1;
          if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
            acc[(ci * 3 + kh) * 3 + kw] = fmaf(g, img[(((size_t)b * CIN + ci) * H + ih) * W + iw], acc[(ci * 3 + kh) * 3 + kw]);
        }
  }
#pragma unroll
  for (int t = 0; t < K; ++t) red[pl][t][co] = acc[t];
  __syncthreads();
  for (int i = threadIdx.x; i < K * CO; i += 256) {
    const int t = i / CO, c = i % CO;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < NPL; ++k) v += red[k][t][c];
    part[((size_t)blockIdx.x * K + t) * CO + c] = v;  // [chunk][tap][co] == wgrad partial layout with M = Cout, N = 1
  }
}
hipError_t launch_stem_wgrad(const float* img, const float* dz, float* part, int B, int Cin, int H, int W, int Cout, int chunk,
                             int nchunks, hipStream_t s) {
#define D2T_STEM_WGRAD(CO, CI) hipLaunchKernelGGL((stem_wgrad_kernel<CO, CI>), dim3(nchunks), dim3(256), 0, s, img, dz, part, B, H, W, chunk)
  if (Cout == 32 && Cin == 1) D2T_STEM_WGRAD(32, 1);
  else if (Cout == 64 && Cin == 1) D2T_STEM_WGRAD(64, 1);
  else if (Cout == 32 && Cin == 3) D2T_STEM_WGRAD(32, 3);
  else if (Cout == 64 && Cin == 3) D2T_STEM_WGRAD(64, 3);
  else return hipErrorInvalidValue;
#undef D2T_STEM_WGRAD
  return hipGetLastError();
}

}  // namespace d2t
