// Implicit-GEMM convolution on the bf16 matrix cores with fp32-class accuracy ("bf16x3").
//
// Every fp32 operand is split as x = hi + lo with hi = the upper 16 bits of x (a bf16) and
// lo = bf16(x - hi); the product is accumulated in fp32 as  a_hi*b_hi + a_hi*b_lo + a_lo*b_hi
// (the dropped a_lo*b_lo term is ~2^-18 relative).  Three v_mfma_f32_32x32x16_bf16 replace eight
// v_mfma_f32_32x32x2_f32 for the same K=16 slice: 5.3x the fp32-MFMA rate at ~2^-17 relative
// product error.  Measured end to end on the headline model (CPU emulation in tools/, GPU parity
// tests): encoder memory error 1e-4, logits error 2.4e-5 (budget 1e-3), greedy tokens unchanged.
//
// Same GEMM view, tile shape (128x128x32, 2x2 waves, 64x64 wave tile), loader geometry and
// epilogue as conv_mfma.hip.  Weights arrive pre-split (two bf16 planes, OHWI); activations stay
// fp32 in HBM and are split in registers while staging.  LDS holds four bf16 planes per stage
// ([rows][32] = 64-byte rows); the 16-byte k-chunk index is XOR-swizzled with (row>>2)&3 so that
// the 16-lane groups of every ds_read_b128 touch all 64 banks exactly once.
// MFMA operand map (32x32x16 bf16): lane l holds A[row l&31][k = 8*(l>>5) + j], j = 0..7, and the
// same for B with its column: one 16-byte chunk per lane per k16-step.
#include <type_traits>

#include "conv_dma.h"

namespace d2t {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// four consecutive-k floats -> packed hi (truncation) and lo (RNE of the remainder) bf16 quads
__device__ __forceinline__ void split4(const float4 v, uint2& hi, uint2& lo) {
  const unsigned x0 = __float_as_uint(v.x), x1 = __float_as_uint(v.y), x2 = __float_as_uint(v.z),
                 x3 = __float_as_uint(v.w);
  hi.x = __builtin_amdgcn_perm(x1, x0, 0x07060302u);  // [x0.hi16 | x1.hi16 << 16]
  hi.y = __builtin_amdgcn_perm(x3, x2, 0x07060302u);
  const f32x2 r01 = {v.x - __uint_as_float(x0 & 0xFFFF0000u), v.y - __uint_as_float(x1 & 0xFFFF0000u)};
  const f32x2 r23 = {v.z - __uint_as_float(x2 & 0xFFFF0000u), v.w - __uint_as_float(x3 & 0xFFFF0000u)};
  const bf16x2 l01 = __builtin_convertvector(r01, bf16x2), l23 = __builtin_convertvector(r23, bf16x2);
  lo.x = *reinterpret_cast<const unsigned*>(&l01);
  lo.y = *reinterpret_cast<const unsigned*>(&l23);
}

template <int BM, int BN, int WM, int WN, bool DEEP>  // block tile, wave grid (WM x WN waves), pipelining depth
__global__ __launch_bounds__(WM * WN * 64, (WM * WN) / 2) void conv_bf16x3_kernel(const ConvP p) {
  constexpr int NT = WM * WN * 64;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int MI = WTM / 32, NJ = WTN / 32;
  constexpr int RPP = NT / 8;          // A rows staged per pass (8 threads x float4 per row)
  constexpr int AR = BM / RPP;         // A rows per thread per K-step (one float4 each)
  constexpr int BC = BN * 4 / NT;      // B 16-byte chunks per thread per plane
  static_assert(AR >= 1 && BC >= 1 && MI >= 1 && NJ >= 1, "tile too small for the wave grid");
  constexpr int PLANE_A = BM * XROW, PLANE_B = BN * XROW;
  constexpr int STAGE = 2 * PLANE_A + 2 * PLANE_B;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE];
  static_assert(BM * BN * 4 <= 2 * STAGE, "the wide epilogue's fp32 tile must fit in the staging area");

  const int nt = (p.Cout + BN - 1) / BN;
  const int logical = xcd_logical_tile();
  const int m0 = (logical / nt) * BM;
  const int n0 = (logical % nt) * BN;
  const int tid = threadIdx.x;
  const int kq = tid & 7, lrow = tid >> 3;

  F32Row a[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) a[i] = f32_row(p, m0 + lrow + RPP * i);
  // B chunks of this thread: chunk id q = tid + 256*j -> row q>>2, k-chunk q&3
  size_t b_off[BC];
  bool b_ok[BC];
#pragma unroll
  for (int j = 0; j < BC; ++j) {
    const int q = tid + NT * j, row = q >> 2, c = q & 3;
    const int n = n0 + row;
    b_ok[j] = n < p.Cout;
    b_off[j] = (size_t)(b_ok[j] ? n : 0) * p.K + c * 8;
  }

  // Two register sets for the staged K-steps: loads for K-step t+2 are issued at the top of
  // iteration t, while the set fetched one iteration earlier (K-step t+1) is converted and written to
  // LDS in small pieces BETWEEN the MFMAs of step t, so VALU / LDS-store issue hides under the matrix pipe.
  float4 ra[2][AR];
  uint4 rbh[2][BC], rbl[2][BC];
  TapCursor<> cur;  // the NEXT K-step to fetch
  const int KT = p.K / XBK;

  auto fetch = [&](int kt, float4 (&xa)[AR], uint4 (&xh)[BC], uint4 (&xl)[BC]) {
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      // branch-free: out-of-image taps read a valid address (the tensor base) and are zeroed by a select
      const int ih = a[i].ih0 + cur.kh, iw = a[i].iw0 + cur.kw;
      const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      const size_t off = ok ? (size_t)(a[i].pix + ih * p.W + iw) * p.Cin + cur.c0 + kq * 4 : (size_t)(kq * 4);
      const float4 v = *reinterpret_cast<const float4*>(p.in + off);
      const unsigned msk = ok ? 0xFFFFFFFFu : 0u;  // bit-mask instead of a select keeps the load unconditional
      xa[i] = make_float4(__uint_as_float(__float_as_uint(v.x) & msk), __uint_as_float(__float_as_uint(v.y) & msk),
                          __uint_as_float(__float_as_uint(v.z) & msk), __uint_as_float(__float_as_uint(v.w) & msk));
    }
#pragma unroll
    for (int j = 0; j < BC; ++j) {
      const uint4 vh = *reinterpret_cast<const uint4*>(p.w_hi + b_off[j] + (size_t)kt * XBK);
      const uint4 vl = *reinterpret_cast<const uint4*>(p.w_lo + b_off[j] + (size_t)kt * XBK);
      const unsigned msk = b_ok[j] ? 0xFFFFFFFFu : 0u;
      xh[j] = make_uint4(vh.x & msk, vh.y & msk, vh.z & msk, vh.w & msk);
      xl[j] = make_uint4(vl.x & msk, vl.y & msk, vl.z & msk, vl.w & msk);
    }
    cur.advance(p);
  };
  // piece q of the staging work of one K-step: q < AR -> A row group q, else B chunk q - AR
  auto stage_piece = [&](int buf, int q, const float4 (&xa)[AR], const uint4 (&xh)[BC], const uint4 (&xl)[BC]) {
    unsigned char* ah = smem + buf * STAGE;
    unsigned char* al = ah + PLANE_A;
    unsigned char* bh = al + PLANE_A;
    unsigned char* bl = bh + PLANE_B;
    if (q < AR) {
      const int row = lrow + RPP * q;
      const int off = row * XROW + swz_chunk(row, kq >> 1) * 16 + (kq & 1) * 8;
      uint2 hi, lo;
      split4(xa[q], hi, lo);
      *reinterpret_cast<uint2*>(ah + off) = hi;
      *reinterpret_cast<uint2*>(al + off) = lo;
    } else if (q - AR < BC) {
      const int j = q - AR;
      const int qq = tid + NT * j, row = qq >> 2, c = qq & 3;
      const int off = row * XROW + swz_chunk(row, c) * 16;
      *reinterpret_cast<uint4*>(bh + off) = xh[j];
      *reinterpret_cast<uint4*>(bl + off) = xl[j];
    }
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WN, wn = wave % WN;
  const int r = lane & 31, h = lane >> 5;

  f32x16 acc[MI][NJ];
  zero_acc(acc);

  // prologue: K-step 0 -> LDS[0]; K-step 1 in flight in set 1
  fetch(0, ra[0], rbh[0], rbl[0]);
#pragma unroll
  for (int q = 0; q < AR + BC; ++q) stage_piece(0, q, ra[0], rbh[0], rbl[0]);
  if (KT > 1) fetch(1, ra[1], rbh[1], rbl[1]);
  __syncthreads();

  constexpr int NPIECE = AR + BC;
  // K-step kt from LDS[kt&1]; if STAGE_NEXT the set (sa,sh,sl) = K-step kt+1 is converted and written
  // to the other LDS buffer one piece per MFMA triple, and (FETCH) K-step kt+2 is loaded into (na,nh,nl).
  auto compute = [&](int kt, auto stage_next, auto fetch_next, const float4 (&sa)[AR], const uint4 (&sh)[BC],
                     const uint4 (&sl)[BC], float4 (&na)[AR], uint4 (&nh)[BC], uint4 (&nl)[BC]) {
    constexpr bool STAGE_NEXT = decltype(stage_next)::value, FETCH = decltype(fetch_next)::value;
    const int cur = kt & 1;
    const unsigned char* ah = smem + cur * STAGE;
    const unsigned char* al = ah + PLANE_A;
    const unsigned char* bh = al + PLANE_A;
    const unsigned char* bl = bh + PLANE_B;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int c = 2 * kk + h;
      bf16x8 fah[MI], fal[MI], fbh[NJ], fbl[NJ];
      read_frags32(ah, al, wm * WTM + r, c, fah, fal);
      read_frags32(bh, bl, wn * WTN + r, c, fbh, fbl);
      if (FETCH && kk == 0) fetch(kt + 2, na, nh, nl);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          acc[i][j] = product(acc[i][j], fah[i], fal[i], fbh[j], fbl[j]);
          const int piece = (kk * MI + i) * NJ + j;  // compile-time after unrolling
          if (STAGE_NEXT && DEEP && piece < NPIECE) stage_piece(cur ^ 1, piece, sa, sh, sl);
        }
    }
    if (STAGE_NEXT) {  // leftovers (or, without DEEP, the whole staging: the loads were issued this iteration)
#pragma unroll
      for (int piece = DEEP ? 2 * MI * NJ : 0; piece < NPIECE; ++piece) stage_piece(cur ^ 1, piece, sa, sh, sl);
    }
    __syncthreads();
  };
  using T_ = std::integral_constant<bool, true>;
  using F_ = std::integral_constant<bool, false>;

  if constexpr (!DEEP) {
    // occupancy-driven variant (4 waves per SIMD): one register set, K-step t+1 fetched at the top of
    // iteration t and staged after its MFMAs; other waves cover the staging time
    for (int kt2 = 0; kt2 < KT; ++kt2) {
      if (kt2 + 1 < KT) {
        if (kt2 > 0) fetch(kt2 + 1, ra[1], rbh[1], rbl[1]);  // (K-step 1 was fetched in the prologue)
        compute(kt2, T_{}, F_{}, ra[1], rbh[1], rbl[1], ra[0], rbh[0], rbl[0]);
      } else {
        compute(kt2, F_{}, F_{}, ra[1], rbh[1], rbl[1], ra[0], rbh[0], rbl[0]);
      }
    }
    if (wide_epilogue_full_ok(p)) conv_epilogue_tile<Epi::full, BM, BN, NT>(p, acc, smem, m0, n0, wm * WTM, wn * WTN, r, h, tid);
    else conv_epilogue<Map32, ElemTwoWay>(p, acc, m0 + wm * WTM, n0 + wn * WTN, r, h);
    return;
  }
  // steady state (K-steps kt+1 and kt+2 exist), unrolled by two so the register sets are static
  int kt = 0;
  for (; kt + 3 < KT; kt += 2) {
    compute(kt, T_{}, T_{}, ra[1], rbh[1], rbl[1], ra[0], rbh[0], rbl[0]);
    compute(kt + 1, T_{}, T_{}, ra[0], rbh[0], rbl[0], ra[1], rbh[1], rbl[1]);
  }
  // tail: at most three K-steps left; set parity continues from the loop (kt is even)
  if (kt + 2 < KT) {        // three left: kt, kt+1, kt+2
    compute(kt, T_{}, T_{}, ra[1], rbh[1], rbl[1], ra[0], rbh[0], rbl[0]);
    compute(kt + 1, T_{}, F_{}, ra[0], rbh[0], rbl[0], ra[1], rbh[1], rbl[1]);
    compute(kt + 2, F_{}, F_{}, ra[1], rbh[1], rbl[1], ra[0], rbh[0], rbl[0]);
  } else if (kt + 1 < KT) { // two left
    compute(kt, T_{}, F_{}, ra[1], rbh[1], rbl[1], ra[0], rbh[0], rbl[0]);
    compute(kt + 1, F_{}, F_{}, ra[0], rbh[0], rbl[0], ra[1], rbh[1], rbl[1]);
  } else if (kt < KT) {     // one left
    compute(kt, F_{}, F_{}, ra[1], rbh[1], rbl[1], ra[0], rbh[0], rbl[0]);
  }
  if (wide_epilogue_full_ok(p)) conv_epilogue_tile<Epi::full, BM, BN, NT>(p, acc, smem, m0, n0, wm * WTM, wn * WTN, r, h, tid);
  else conv_epilogue<Map32, ElemTwoWay>(p, acc, m0 + wm * WTM, n0 + wn * WTN, r, h);
}

// ---------------------------------------------------------------------------
// Split-activation kernel with LDS-DMA staging (conv_dma.h).  The input arrives as split-bf16 records written by the
// producing layer's epilogue (conv_common.h plane_idx), so staging A is a pure 16-byte copy like B: no
// conversion and almost no address arithmetic in the K loop (the on-the-fly variant above spends ~5 VALU
// instructions per MFMA on it).  Per output row a 16-bit validity mask over the filter taps and a signed
// element offset are computed once (rec_row); every wave copies its own 16-row pieces of the four planes.
// ---------------------------------------------------------------------------
// F16 (ConvP::f16, fp16x2 mode): the A records hold fp16 in their hi half (no lo plane is staged or read), the weight planes
// are fp16 hi / lo, a product is x * w_lo + x * w_hi on v_mfma_f32_32x32x16_f16
template <int BM, int BN, int WM, bool F16 = false>  // wave grid WM x 2
struct conv_bf16x3g_body {
  static constexpr int NW = WM * 2, NT = NW * 64;
  static constexpr int WTM = BM / WM, WTN = BN / 2;
  static constexpr int MI = WTM / 32, NJ = WTN / 32;
  using Issuer = DmaIssuer<APlanes<!F16>, BM, BN, NW, false>;  // (a second input: the pipelined kernel only)
  static constexpr int PLANE_A = Issuer::PLANE_A, PLANE_B = Issuer::PLANE_B, STAGE = Issuer::STAGE;
  static constexpr int SMEM = 2 * STAGE;
  static_assert(BM * BN * 4 <= SMEM, "the fp32 tile must fit in the staging area");

  static __device__ __forceinline__ void run(const ConvP& p, unsigned char* smem) {
    const int nt = (p.Cout + BN - 1) / BN;
    const int ntiles = nt * ((p.M + BM - 1) / BM);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;  // (wave-uniform: wm / wn and the piece offsets stay scalar)
    // Persistent over tiles: the grid may be smaller than the tile count (p.max_blocks), which leaves
    // block slots free for the latency-bound decode kernels of the previous batch (pipelined mode).
    // Tile order: in every round the blocks that share an XCD (blockIdx % 8) take consecutive tiles.
    const int G = gridDim.x, gx = G >> 3;
    for (int tile0 = 0; tile0 < ntiles; tile0 += G) {
      int logical = tile0 + blockIdx.x;
      if ((G & 7) == 0) logical = tile0 + (blockIdx.x & 7) * gx + (blockIdx.x >> 3);
      if (logical >= ntiles) break;  // block-uniform
      const int m0 = (logical / nt) * BM;
      const int n0 = (logical % nt) * BN;
      Issuer dma(p, m0, n0, wave, lane);
      const int KT = p.K / XBK;

      const int wm = wave >> 1, wn = wave & 1;
      const int r = lane & 31, h = lane >> 5;
      f32x16 acc[MI][NJ];
      zero_acc(acc);

      dma.issue(p, smem, 0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();

      for (int kt = 0; kt < KT; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < KT) dma.issue(p, smem, kt + 1, cur ^ 1);  // DMA for the next K-step flies under this step's MFMAs
        __builtin_amdgcn_sched_barrier(0);                      // keep the DMA issue ahead of the ds_reads / MFMAs
        const unsigned char* ah = smem + cur * STAGE;
        const unsigned char* al = ah + PLANE_A;
        const unsigned char* bh = al + PLANE_A;
        const unsigned char* bl = bh + PLANE_B;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int c = 2 * kk + h;
          bf16x8 fah[MI], fal[MI], fbh[NJ], fbl[NJ];
          read_frags32<!F16>(ah, al, wm * WTM + r, c, fah, fal);
          read_frags32(bh, bl, wn * WTN + r, c, fbh, fbl);
#pragma unroll
          for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = product<F16>(acc[i][j], fah[i], fal[i], fbh[j], fbl[j]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces have landed
        __syncthreads();                                   // ... and everyone else's; reads of `cur` are done
      }
      if (wide_epilogue_ok(p)) {  // block-uniform
        if (p.pool2) conv_epilogue_tile<Epi::pool, BM, BN, NT>(p, acc, smem, m0, n0, wm * WTM, wn * WTN, r, h, tid);
        else conv_epilogue_tile<Epi::lean, BM, BN, NT>(p, acc, smem, m0, n0, wm * WTM, wn * WTN, r, h, tid);
      } else {
        conv_epilogue<Map32, ElemTwoWay>(p, acc, m0 + wm * WTM, n0 + wn * WTN, r, h);
      }
    }  // tile loop
  }
};

// 8 waves per 128 x 128 tile (wave tile 32 x 64); the dominant GEMM shape (512 -> 512 channels, 3x3: K = 4608) runs the same
// code under its own symbol, so that rocprofv3's per-kernel rows separate it from the other layers
D2T_CONV_ENTRY(conv_bf16x3g_128x128_w8, 4, conv_bf16x3g_body<128, 128, 4>)
D2T_CONV_ENTRY(conv_bf16x3g_128x128_w8_k4608, 4, conv_bf16x3g_body<128, 128, 4>)
D2T_CONV_ENTRY(conv_bf16x3g_128x64, 3, conv_bf16x3g_body<128, 64, 2>)
// fp16x2 builds (ConvP::f16)
D2T_CONV_ENTRY(conv_f16x2g_128x64, 3, conv_bf16x3g_body<128, 64, 2, true>)
D2T_CONV_ENTRY(conv_f16x2g_128x128_w8, 4, conv_bf16x3g_body<128, 128, 4, true>)

hipError_t launch_conv_bf16x3(const ConvP& p, hipStream_t s) {
  if (p.M <= 0 || p.Cout <= 0) return hipSuccess;
  if (p.pool2) {  // fused 2x2 max-pool: split-record LDS-DMA kernels with the wide epilogue only (g body, 16x16x32 pipelined body)
    if (!p.in_hi || !wide_epilogue_ok(p) || p.res || p.res_hi || (p.M & 3) || p.M != 4 * p.B * (p.OH / 2) * (p.OW / 2) ||
        (p.Cout >= 128 && p.pipelined != 3) || (p.Cout > 64 && p.Cout < 128))
      return hipErrorInvalidValue;
  }
  if (!p.w_hi || !p.w_lo || p.Cin % XBK != 0 || p.K != p.KH * p.KW * p.Cin + p.Cin2 || p.m_base != 0) return hipErrorInvalidValue;
  // a second (1x1) input along K: the DMA issuer of the pipelined 16x16x32 kernel only, its 64 x 128 tail build included
  // (launch_conv_bf16x3p hands over as for any layer); not the patch forms
  if (p.Cin2 && (!p.in_hi || !p.in2_hi || p.Cin2 % XBK || p.Cout < 128 || p.pipelined != 3 || p.pool2 || p.OH != p.H || p.OW != p.W))
    return hipErrorInvalidValue;
  if (p.f16 && (!p.in_hi || (p.Cout >= 128 && p.pipelined != 3))) return hipErrorInvalidValue;  // fp16 records: split-record kernels only
  const int mt = (p.M + 127) / 128;
  if (p.in_hi) {  // split-bf16 input planes
    if (!p.zero16 || p.KH * p.KW > 16 || (long long)p.B * p.H * p.W * p.Cin * 2 > 0x7fffffffLL) return hipErrorInvalidValue;
    // layers with >= 128 output channels: the pipelined 256x128 kernel (one block per CU, three LDS stages); dispatch by
    // layer shape only (never by the row count), so a sample's results do not depend on its batch
    if (p.pipelined && p.Cout >= 128) return launch_conv_bf16x3p(p, s);
    // the 32x32 bodies honour ConvP::out_fmt / res_fmt in their tile epilogue (store_rec / add_rec); their element-wise
    // epilogue (ElemTwoWay: a row remap or a positional table) knows the input's format only
    if (!wide_epilogue_ok(p) && ((p.out_hi && p.out_fmt && p.out_fmt - 1 != p.f16) || (p.res_hi && p.res_fmt && p.res_fmt - 1 != p.f16)))
      return hipErrorInvalidValue;
    int tiles = mt * ((p.Cout + (p.Cout <= 64 ? 63 : 127)) / (p.Cout <= 64 ? 64 : 128));
    const int grid = (p.max_blocks > 0 && tiles > p.max_blocks) ? p.max_blocks : tiles;
    if (p.Cout <= 64) {
      // 48 KB of LDS and 4 waves per block: three blocks fit on a CU (launch bounds 256 x 3), which this short-K layer
      // (conv0_2: 9 K-steps per tile) uses to overlap one tile's prologue / epilogue with another's MFMAs whenever the
      // grid is not capped (no slots reserved for the decode stream): 1.35 -> 0.96 ms alone.  With a cap it stays at
      // the cap (three per CU measured 0.5 % slower end to end in pipelined serving).
      if (p.f16) hipLaunchKernelGGL(conv_f16x2g_128x64, dim3(grid), dim3(256), 0, s, p);
      else hipLaunchKernelGGL(conv_bf16x3g_128x64, dim3(grid), dim3(256), 0, s, p);
    } else {
      // 8 waves per tile (4 per SIMD at two blocks per CU) measured 1-2 % faster end to end than 4 waves
      if (p.f16) hipLaunchKernelGGL(conv_f16x2g_128x128_w8, dim3(grid), dim3(512), 0, s, p);
      else if (p.K == 4608 && p.Cout == 512) hipLaunchKernelGGL(conv_bf16x3g_128x128_w8_k4608, dim3(grid), dim3(512), 0, s, p);
      else hipLaunchKernelGGL(conv_bf16x3g_128x128_w8, dim3(grid), dim3(512), 0, s, p);
    }
    return hipGetLastError();
  }
  // fp32 rows in (the ViT encoder's linears, M = B * 261: one to two rounds of 128 x 128 tiles): eight waves per tile measured
  // 15-20 % faster there than four (round 4, tools/probe/conv_per_launch.py: 229 -> 194 us per ViT block)
  if (p.Cout <= 64) {
    hipLaunchKernelGGL((conv_bf16x3_kernel<128, 64, 2, 2, true>), dim3(mt * ((p.Cout + 63) / 64)), dim3(256), 0, s, p);
  } else {
    // 8 waves per 128x128 tile (wave tile 32x64): 4 waves per SIMD at 2 blocks/CU keep the matrix pipe fed
    hipLaunchKernelGGL((conv_bf16x3_kernel<128, 128, 4, 2, false>), dim3(mt * ((p.Cout + 127) / 128)), dim3(512), 0, s, p);
  }
  return hipGetLastError();
}

}  // namespace d2t
