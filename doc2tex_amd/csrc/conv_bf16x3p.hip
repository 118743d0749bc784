// Split-bf16 implicit-GEMM convolution, pipelined form (the roofline kernel of the recognizer's backbone).
//
// Same operand layouts and K order as conv_bf16x3g_body (conv_bf16x3.hip): split-bf16 activation records in, three
// v_mfma_f32_16x16x32_bf16 per product (lo*hi, hi*lo, hi*hi, fp32 accumulate) -- or, on fp16 records (ConvP::f16), two
// v_mfma_f32_16x16x32_f16 (x*w_lo, x*w_hi).  How a CU is kept busy:
//
//   * block tile 256 x 128 x 32, 8 compute waves as 4 (M) x 2 (N), wave tile 64 x 64 = 4 x 4 MFMA blocks: 16 ds_read_b128 and
//     48 MFMAs per wave and K-step, 48 KB of L2 -> LDS traffic per 1536 MFMA cycles of a SIMD;
//   * ONE block per CU holding THREE LDS stages (144 KB): the LDS-DMA of K-step t+2 is issued while K-step t is computed,
//     the issuer waits only for its OWN pieces of step t with a counted `s_waitcnt vmcnt(N)` (the pieces of step t+1 stay
//     in flight), and a K-step costs one raw s_barrier -- no `vmcnt(0)` drain, no second barrier
//     (cdna_hip_programming.md "Pipelining across barriers": the 3-buffer span);
//   * LOADER WAVES: the block is 8 compute waves + 4 loader waves (one per SIMD).  A K-step's 48 KB go through the CU's
//     vector-memory path at 64 B/clk = 768 cycles -- half of the 1536 MFMA cycles a SIMD needs for the step.  When the
//     compute waves issue the LDS-DMA themselves they all sit in that queue at the same time (one block per CU: nobody
//     else has MFMAs to issue) and the two phases add up: measured 3090 cycles per K-step.  Loader waves own the whole
//     vector-memory side (addresses, LDS-DMA, counted waits); compute waves only ds_read and MFMA;
//   * STAGGER (MI355X_MICROARCH.md "Two waves per SIMD", item 9): the two compute waves that share a SIMD (w and w + 4) would
//     reach their fragment reads, their MFMAs and the barrier together -- both wait for LDS, then both want the matrix pipe.
//     Waves 4-7 therefore run half a K-step behind: they load the fragments of a step's second half (two of the four A row
//     blocks) BEFORE the next barrier and issue those MFMAs right AFTER it, while the SIMD partner waits for its first
//     fragments.  Every accumulator still sees the same MFMAs in the same order;
//   * persistent over tiles with a grid of (CUs - reserved), XCD-aware tile order.
//
// Hazards (checked against the rules of the guide):
//   RAW  a stage is read only after every wave has passed the barrier that follows its own counted vmcnt wait for that
//        stage's pieces ("read a staged buffer after the wait that retires it and a barrier the reader has passed");
//   WAR  stage (t+2)%3 == (t-1)%3 is overwritten by DMAs issued after barrier t; every wave has finished the ds_reads of
//        step t-1 before it arrives there (they feed MFMAs that precede the barrier in program order, and the compiler's
//        lgkmcnt waits sit in front of those MFMAs).
//
// Rounds 1-3 built this kernel in several other shapes -- 32x32x16 MFMAs, a patch-resident and a band-resident 3x3 form, a
// 256 x 256 tile on eight waves, a loader-less 8-wave form, Winograd F(2x2,3x3) -- all bit-identical or equally accurate, none
// faster in serving (docs/experiments_r03.md).  They left the tree in round 4 (git history: round 3).

#include <type_traits>

#include "conv_dma.h"

namespace d2t {

namespace {
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field on gfx9");
  // s_waitcnt simm16: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt_hi[15:14]; leave expcnt / lgkmcnt untouched (max)
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}
#ifdef D2T_PROBES
// probe builds: thread 0 of block 0 (a compute wave that is not staggered) adds the time between consecutive marks of a tile
// (s_memrealtime, 10 ns ticks) to d2t_conv_phase[k]; [15] counts tiles.  tools/probe/conv_phases.py
__device__ unsigned long long d2t_conv_phase[16];
#define CONV_PHASE(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); \
    atomicAdd(&d2t_conv_phase[k], now_ - cphase_t_); cphase_t_ = now_; } } while (0)
#define CONV_PHASE_INIT() unsigned long long cphase_t_ = __builtin_amdgcn_s_memrealtime()
#define CONV_PHASE_TILE() do { if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&d2t_conv_phase[15], 1ull); } while (0)
#else
#define CONV_PHASE(k) do { } while (0)
#define CONV_PHASE_INIT() do { } while (0)
#define CONV_PHASE_TILE() do { } while (0)
#endif
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// The kernel body on v_mfma_f32_16x16x32_bf16 (round 3; rounds 1-2 used 32x32x16): one MFMA consumes the WHOLE K-step of
// 32 for a 16 x 16 output block (16 cycles on a SIMD) instead of half of it for a 32 x 32 block (32 cycles).  Per K-step a
// wave reads the same 16 fragments (8 of A: 4 row blocks x hi / lo; 8 of B) and issues 48 MFMAs with the same FLOPs and
// the same matrix-pipe cycles, but the chip holds a higher clock under this shape on random data (MI355X_MICROARCH.md
// "DVFS give-back" item 7: 1.12-1.15 x the FLOP/s of the 32x32x16 loop with every operand re-read from LDS) -- and this
// kernel is power-bound, not issue-bound (1.57 ms on random operands, 1.27 ms on zeros).
// Per output element still three products per K-step in the order lo*hi, hi*lo, hi*hi, fp32 accumulate; the summation
// INSIDE an MFMA now spans 32 k instead of 16, so results are not bit-identical to the 32x32x16 kernels (they agree to fp32
// rounding; every kernel that may compute rows of the same layer must use the same shape -- see launch_conv_bf16x3p).
// The stagger splits a K-step by ROW BLOCKS (first two of A, then the other two) since it can no longer be split by k:
// waves 4-7 carry the B fragments and the second pair of A fragments across the barrier.
//
// F16 (ConvP::f16, fp16x2 mode): A = the fp16 hi halves of the records only (12 instead of 16 fragment reads, 8 instead of
// 12 LDS-DMA pieces per loader and K-step), B = fp16 hi / lo planes, 32 MFMAs (x * w_lo, x * w_hi) instead of 48
template <int BM, int BN, int WM, int WN, int NL, bool STG, int ABL = 0, bool F16 = false>  // ABL (probe builds): 1 no LDS-DMA, 2 no MFMA, 4 LDS-DMA never awaited
struct conv_bf16x3p16_body {
  static constexpr int NW = WM * WN, NT = (NW + NL) * 64;
  static constexpr int WTM = BM / WM, WTN = BN / WN;
  static constexpr int MI = WTM / 16, NJ = WTN / 16, MH = MI / 2;
  static constexpr int NSTG = 3;  // LDS stages in the ring
  static constexpr bool UPFRONT = ABL != 8;  // (8: the reads as the compiler schedules them, for A/B timing in probe builds)
  static_assert(MI >= 2 && (MI & 1) == 0 && NJ >= 1 && NL > 0, "wave tile / loader configuration");
  using Issuer = DmaIssuer<std::conditional_t<F16, AHalfF16, ARecords>, BM, BN, NL, true, ABL == 1>;
  static constexpr int PLANE_B = Issuer::PLANE_B, STAGE = Issuer::STAGE, PER_STEP = Issuer::PER_STEP, A_BYTES = Issuer::A_BYTES;
  // the ring, or the epilogue's fp32 tile where that is larger (the fp16x2 256 x 128 build: 32 KB stages, a 128 KB tile)
  static constexpr int SMEM = NSTG * STAGE > BM * BN * 4 ? NSTG * STAGE : BM * BN * 4;

  static __device__ __forceinline__ void run(const ConvP& p, unsigned char* smem) {
    const int nt = (p.Cout + BN - 1) / BN;
    const int ntiles = nt * ((p.M - p.m_base + BM - 1) / BM);  // rows [m_base, M): the rows a 256 x 256 launch left over
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const bool loader = wave >= NW;  // wave-uniform
    const int KT = p.K / XBK;
    const int G = gridDim.x, slot = xcd_logical_tile();

    CONV_PHASE_INIT();
    for (int tile = slot; tile < ntiles; tile += G) {
      const int m0 = p.m_base + (tile / nt) * BM;
      const int n0 = (tile % nt) * BN;
      CONV_PHASE(0);  // previous tile's last barrier .. here (loop overhead; the first tile: kernel entry)
      CONV_PHASE_TILE();
      if (loader) {  // (the compute waves below run the same barrier sequence)
        Issuer dma(p, m0, n0, wave - NW, lane);
        dma.issue(p, smem, 0, 0);
        if (KT > 1) dma.issue(p, smem, 1, 1);
        int nxt2 = 2;
        for (int kt = 0; kt < KT; ++kt) {
          if (ABL != 4) { if (kt + 1 < KT) wait_vm<PER_STEP>(); else wait_vm<0>(); }
          __builtin_amdgcn_s_barrier();
          if (kt + 2 < KT) dma.issue(p, smem, kt + 2, nxt2);
          nxt2 = nxt2 == 2 ? 0 : nxt2 + 1;
        }
        if (ABL == 4) wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_barrier();
        if (wide_epilogue_ok(p)) { if (p.pool2) tile_rows_epilogue<Epi::pool, 8, BM, BN, NT>(p, smem, m0, n0, tid); else tile_rows_epilogue<Epi::lean, 8, BM, BN, NT>(p, smem, m0, n0, tid); }
        __builtin_amdgcn_s_barrier();
        continue;
      }
      const int wm = wave / WN, wn = wave % WN;
      const int r = lane & 15, q = lane >> 4;
      f32x4v acc[MI][NJ];
      zero_acc(acc);
      int offa[MI], offal[MI], offb[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wm * WTM + i * 16 + r;
        offa[i] = F16 ? row * XROW + pswz16(row, q) * 16 : row * 128 + aswz(row, q) * 16;
        offal[i] = row * 128 + aswz(row, 4 + q) * 16;  // (unused with F16)
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int row = wn * WTN + j * 16 + r;
        offb[j] = row * XROW + pswz16(row, q) * 16;
      }
      auto read_b = [&](const unsigned char* ah, bf16x8 (&fbh)[NJ], bf16x8 (&fbl)[NJ]) {
        const unsigned char* bh = ah + A_BYTES;
        const unsigned char* bl = bh + PLANE_B;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          fbh[j] = *reinterpret_cast<const bf16x8*>(bh + offb[j]);
          fbl[j] = *reinterpret_cast<const bf16x8*>(bl + offb[j]);
        }
      };
      auto read_a = [&](const unsigned char* ah, auto half_c, bf16x8 (&fah)[MH], bf16x8 (&fal)[MH]) {
        constexpr int half = decltype(half_c)::value;
#pragma unroll
        for (int i = 0; i < MH; ++i) {
          fah[i] = *reinterpret_cast<const bf16x8*>(ah + offa[half * MH + i]);
          if (!F16) fal[i] = *reinterpret_cast<const bf16x8*>(ah + offal[half * MH + i]);
        }
      };
      auto mma = [&](auto half_c, const bf16x8 (&fah)[MH], const bf16x8 (&fal)[MH], const bf16x8 (&fbh)[NJ], const bf16x8 (&fbl)[NJ]) {
        constexpr int half = decltype(half_c)::value;
#pragma unroll
        for (int i = 0; i < MH; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            if (ABL == 2) {  // keep the reads alive, drop the matrix work
              asm volatile("" ::"v"(fal[i]), "v"(fah[i]), "v"(fbh[j]), "v"(fbl[j]));
              continue;
            }
            acc[half * MH + i][j] = product<F16>(acc[half * MH + i][j], fah[i], fal[i], fbh[j], fbl[j]);
          }
      };
      using H0 = std::integral_constant<int, 0>;
      using H1 = std::integral_constant<int, 1>;
      int cur = 0;
      const bool late = STG && wave >= NW / 2;
      if (!late) {
        for (int kt = 0; kt < KT; ++kt) {
          __builtin_amdgcn_s_barrier();  // stage kt (and kt + 1) complete for everyone; nobody reads the stages before
          if (kt == 0) CONV_PHASE(1);  // setup + the first two stages' LDS-DMA landed (pipeline fill)
          const unsigned char* ah = smem + cur * STAGE;
          // all sixteen fragment reads of the K-step go out before the first MFMA (the SIMD partner's carried MFMAs cover
          // their latency); left to itself the compiler interleaves them in three groups, each with its own wait
          bf16x8 fbh[NJ], fbl[NJ], fah[MH], fal[MH], fch[MH], fcl[MH];
          read_b(ah, fbh, fbl);
          read_a(ah, H0{}, fah, fal);
          read_a(ah, H1{}, fch, fcl);
          if (UPFRONT) __builtin_amdgcn_sched_barrier(0);
          mma(H0{}, fah, fal, fbh, fbl);
          mma(H1{}, fch, fcl, fbh, fbl);
          cur = cur == NSTG - 1 ? 0 : cur + 1;
        }
      } else {
        bf16x8 gah[MH], gal[MH], gbh[NJ], gbl[NJ];  // second-half A fragments and the step's B fragments, carried across the barrier
        auto step = [&](auto carried_c, int kt) {
          __builtin_amdgcn_s_barrier();
          const unsigned char* ah = smem + cur * STAGE;
          if (decltype(carried_c)::value) mma(H1{}, gah, gal, gbh, gbl);  // second half of the previous K-step
          __builtin_amdgcn_sched_barrier(0);  // (no reads of this step hoisted above: the carried fragments die first)
          read_b(ah, gbh, gbl);
          {
            bf16x8 fah[MH], fal[MH];
            read_a(ah, H0{}, fah, fal);
            if (UPFRONT) {  // the carried half's fragments are requested before the first half's MFMAs, not after them
              read_a(ah, H1{}, gah, gal);
              __builtin_amdgcn_sched_barrier(0);
            }
            mma(H0{}, fah, fal, gbh, gbl);
          }
          if (!UPFRONT) read_a(ah, H1{}, gah, gal);
          // the reads have returned before this wave arrives at the next barrier (after it the stage may be overwritten)
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          cur = cur == NSTG - 1 ? 0 : cur + 1;
        };
        step(H0{}, 0);  // peeled: nothing carried into K-step 0
        for (int kt = 1; kt < KT; ++kt) step(H1{}, kt);
        mma(H1{}, gah, gal, gbh, gbl);
      }
      CONV_PHASE(2);  // the K loop of this wave
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave is done with the last stages: the staging area becomes the epilogue's fp32 tile
      CONV_PHASE(3);  // waiting for the other waves (staggered partners finish half a K-step later)
      if (wide_epilogue_ok(p)) {  // block-uniform
        acc_to_tile<Map16, BN>(acc, reinterpret_cast<float*>(smem), wm * WTM, wn * WTN, r, q);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        CONV_PHASE(4);  // accumulators to the LDS tile + barrier
        if (p.pool2) tile_rows_epilogue<Epi::pool, 8, BM, BN, NT>(p, smem, m0, n0, tid);
        else tile_rows_epilogue<Epi::lean, 8, BM, BN, NT>(p, smem, m0, n0, tid);
        CONV_PHASE(5);  // this thread's rows: LDS reads, bias / residual / activation / split, stores issued
      } else {  // (row remap, positional add, Cout % 32 != 0)
        __builtin_amdgcn_s_barrier();
        conv_epilogue<Map16, ElemThreeWay>(p, acc, m0 + wm * WTM, n0 + wn * WTN, r, q);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // the tile is staging memory again (next tile's LDS-DMA)
      CONV_PHASE(6);  // waiting for the slowest thread's epilogue
    }
  }
};


// 256 x 128 tile, 8 compute waves as 4 x 2 + 4 loaders, staggered; the dominant GEMM shape (512 -> 512 channels, 3x3:
// K = 4608) under its own symbol, so that rocprofv3's per-kernel rows separate it from the other layers
D2T_CONV_ENTRY(conv_bf16x3p16_256x128_s, 3, conv_bf16x3p16_body<256, 128, 4, 2, 4, true>)
D2T_CONV_ENTRY(conv_bf16x3p16_256x128_s_k4608, 3, conv_bf16x3p16_body<256, 128, 4, 2, 4, true>)
// 64 x 128 tile on the same body (eight 64 x 16 wave tiles + four loaders, 24 KB stages): the rows of a last, sparsely
// filled round of 256-row tiles (launch_conv_bf16x3p).  Same MFMA shape, K order and products: bit-identical to the 256 x 128
// build, so which of the two computes a row never shows in the values.
D2T_CONV_ENTRY(conv_bf16x3p16_64x128_tail, 3, conv_bf16x3p16_body<64, 128, 1, 8, 4, false>)
// fp16x2 builds (ConvP::f16)
D2T_CONV_ENTRY(conv_f16x2p16_64x128_tail, 3, conv_bf16x3p16_body<64, 128, 1, 8, 4, false, 0, true>)
D2T_CONV_ENTRY(conv_f16x2p16_256x128_s, 3, conv_bf16x3p16_body<256, 128, 4, 2, 4, true, 0, true>)
D2T_CONV_ENTRY(conv_f16x2p16_256x128_s_k4608, 3, conv_bf16x3p16_body<256, 128, 4, 2, 4, true, 0, true>)

#ifdef D2T_PROBES  // ablation probes of the 16x16x32 kernel (D2T_CONV_ABL=1|2|4): results are garbage by construction
template <int ABL>
__global__ __launch_bounds__(768, 3) void conv_bf16x3p16_probe(const ConvP p) {
  using Body = conv_bf16x3p16_body<256, 128, 4, 2, 4, true, ABL>;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[Body::SMEM];
  Body::run(p, smem);
}
#endif


static int abl_probe() {
  static const int abl = D2T_PROBE_ENV("D2T_CONV_ABL");
  return abl;
}

// grid of the pipelined kernel: one block per CU on (CUs - reserved) CUs, never more blocks than tiles
hipError_t launch_conv_bf16x3p(const ConvP& p, hipStream_t s) {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
      return hipErrorInvalidDevice;
    cus = n;
  }
  if (p.pipelined != 3 || p.store_mode != STORE_ROWS) return hipErrorInvalidValue;  // (no head-split store in this kernel's epilogues)
  ConvP q = p;
  const int nt = (p.Cout + 127) / 128;
  int grid = cus - (p.reserved_cus > 0 ? p.reserved_cus : 0);
  if (grid < 8) grid = 8;
  int tiles = ((p.M - p.m_base + 255) / 256) * nt;
  // Whole rounds only: when the last round of 256-row tiles would be less than half full (the dominant layer at B = 64: 2064
  // tiles = eight rounds + 16 tiles; at B = 32: 4.03 rounds; config C1: 260 tiles), the rows behind the whole rounds go to the
  // 64 x 128 build of the same body, whose small tiles spread over the chip.  Same MFMA shape, K order and products per output
  // element in both kernels (tests assert bit-identity), so which of them computes a row never shows in the values.  The
  // caller switches it off (split_tail = 0) while decode loops are in flight: their kernels run in exactly that hole.
  static const float tail_frac = D2T_PROBE_ENV_STR("D2T_CONV_TAIL") ? (float)atof(D2T_PROBE_ENV_STR("D2T_CONV_TAIL")) : 0.5f;
  int tail_from = -1;
  if (p.split_tail && p.m_base == 0 && !abl_probe()) {
    const int rounds = tiles / grid, rem = tiles - rounds * grid;
    if (rounds >= 1 && rem > 0 && rem < tail_frac * grid) {
      const int main_mt = rounds * grid / nt;  // whole rows of tiles that fit into the whole rounds
      tail_from = main_mt * 256;
      q.M = tail_from;
      tiles = main_mt * nt;
    }
  }
  if (grid > tiles) grid = tiles;
  const bool dom = p.K == 4608 && p.Cout == 512;
#ifdef D2T_PROBES
  if (abl_probe() && !p.f16) {
    switch (abl_probe()) {
      case 1: hipLaunchKernelGGL(conv_bf16x3p16_probe<1>, dim3(grid), dim3(768), 0, s, q); break;
      case 2: hipLaunchKernelGGL(conv_bf16x3p16_probe<2>, dim3(grid), dim3(768), 0, s, q); break;
      case 8: hipLaunchKernelGGL(conv_bf16x3p16_probe<8>, dim3(grid), dim3(768), 0, s, q); break;
      default: hipLaunchKernelGGL(conv_bf16x3p16_probe<4>, dim3(grid), dim3(768), 0, s, q); break;
    }
    return hipGetLastError();
  }
#endif
  if (p.f16) {  // fp16 records in: two MFMAs per product
    if (dom) hipLaunchKernelGGL(conv_f16x2p16_256x128_s_k4608, dim3(grid), dim3(768), 0, s, q);
    else hipLaunchKernelGGL(conv_f16x2p16_256x128_s, dim3(grid), dim3(768), 0, s, q);
  } else {
    if (dom) hipLaunchKernelGGL(conv_bf16x3p16_256x128_s_k4608, dim3(grid), dim3(768), 0, s, q);
    else hipLaunchKernelGGL(conv_bf16x3p16_256x128_s, dim3(grid), dim3(768), 0, s, q);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || tail_from < 0) return e;
  ConvP t = p;
  t.m_base = tail_from;
  const int tt = ((p.M - tail_from + 63) / 64) * nt;
  if (p.f16) hipLaunchKernelGGL(conv_f16x2p16_64x128_tail, dim3(tt), dim3(768), 0, s, t);
  else hipLaunchKernelGGL(conv_bf16x3p16_64x128_tail, dim3(tt), dim3(768), 0, s, t);
  return hipGetLastError();
}

#ifdef D2T_PROBES
}  // namespace d2t
extern "C" int d2t_debug_conv_phases(unsigned long long* out, int reset) {  // probe builds: read (and clear) d2t_conv_phase
  hipDeviceSynchronize();
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(d2t::d2t_conv_phase), 16 * 8) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(d2t::d2t_conv_phase), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
namespace d2t {
#endif
}  // namespace d2t
