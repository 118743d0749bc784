// LDS-DMA staging of the split-record convolution kernels (conv_bf16x3.hip: conv_bf16x3g_body, conv_bf16x3p.hip:
// conv_bf16x3p16_body): both operands are pure copies, so every 16-byte chunk goes global -> LDS directly
// (global_load_lds_dwordx4: no staging registers, no ds_write).  The LDS destination of a wave instruction is linear
// (base + lane * 16 = one 1 KiB piece), so the XOR swizzle of the k-chunk is applied to the per-lane SOURCE address and again
// on the ds_read side (cdna guide rule 21).  Out-of-image taps and rows beyond M / Cout point the source at a zero page.
#pragma once
#include "conv_common.h"

namespace d2t {

typedef __attribute__((address_space(3))) void* lds_ptr;

// swz_chunk (conv_common.h) for the 16x16x32 fragment pattern (lane -> row lane & 15, 16-byte k-chunk lane >> 4): the 16-lane service groups
// of a ds_read_b128 then pair rows 0-3 / 12-15 at chunk c with rows 4-11 at chunk c ^ 1, and XOR-ing bit 1 of the chunk
// with bit 3 of the row spreads every group over all 64 banks (tools/probe/lds_swizzle_check.py)
__device__ __forceinline__ int pswz16(int row, int c) { return c ^ ((row >> 2) & 2); }
// whole 128-byte records as LDS rows: the eight 16-byte chunks of a row are XOR-ed with (row >> 1) & 7 -- on the source side
// of the DMA and on the ds_read side -- so that the 16-lane groups of a ds_read_b128 hit every bank once
__device__ __forceinline__ int aswz(int row, int c) { return c ^ ((row >> 1) & 7); }

// How a stage holds its operands: A_ROW bytes of LDS per tile row of A, the rows of a 1 KiB piece (one wave instruction), the
// record chunk that belongs at a lane's LDS position, whether a second instruction copies the lo halves into a plane of
// their own -- and the swizzle of the two B planes (64-byte rows, 16 rows per piece), which follows the fragment pattern
// of the kernel's MFMA shape.
//   split planes (32x32x16 kernels): A as a hi and a lo plane of 64-byte rows, swz_chunk.  LO = false (fp16 records): the lo
//   plane keeps its place in the stage and is neither copied nor read
template <bool LO>
struct APlanes {
  static constexpr int A_ROW = 2 * XROW, PIECE_ROWS = 16;
  static constexpr bool LO_PLANE = LO;
  static __device__ __forceinline__ int row(int piece, int lane) { return piece * 16 + (lane >> 2); }
  static __device__ __forceinline__ int chunk(int row, int lane) { return swz_chunk(row, lane & 3); }
  static __device__ __forceinline__ int bchunk(int row, int pos) { return swz_chunk(row, pos); }
};
//   whole records (16x16x32 kernels): one LDS row per tile row holding the record [hi 64 | lo 64]; a piece = 8 rows x 128 B,
//   i.e. a wave's LDS-DMA touches 8 full cache lines instead of 16 half lines (the vector-memory path's cost is per line
//   touched: 32-byte segments measured half the rate of 64-byte ones)
struct ARecords {
  static constexpr int A_ROW = 2 * XROW, PIECE_ROWS = 8;
  static constexpr bool LO_PLANE = false;
  static __device__ __forceinline__ int row(int piece, int lane) { return piece * 8 + (lane >> 3); }
  static __device__ __forceinline__ int chunk(int row, int lane) { return aswz(row, lane & 7); }
  static __device__ __forceinline__ int bchunk(int row, int pos) { return pswz16(row, pos); }
};
//   fp16 hi halves (16x16x32 kernels, ConvP::f16): only the hi half of a record is staged, one plane of 64-byte rows with
//   the B planes' swizzle
struct AHalfF16 {
  static constexpr int A_ROW = XROW, PIECE_ROWS = 16;
  static constexpr bool LO_PLANE = false;
  static __device__ __forceinline__ int row(int piece, int lane) { return piece * 16 + (lane >> 2); }
  static __device__ __forceinline__ int chunk(int row, int lane) { return pswz16(row, lane & 3); }
  static __device__ __forceinline__ int bchunk(int row, int pos) { return pswz16(row, pos); }
};

// The vector-memory side of a tile for ONE of LW issuing waves: which pieces of the A / B planes it copies, their per-lane
// source addresses and the per-row validity mask over the filter taps.  A stage is [A | B hi | B lo].
// SECOND: the launch may carry a second input (ConvP::in2_hi); NODMA (probe builds): addresses only, nothing is copied.
template <class Geom, int BM, int BN, int LW, bool SECOND, bool NODMA = false>
struct DmaIssuer {
  static constexpr int AJ = BM / (Geom::PIECE_ROWS * LW), BJ = BN / (16 * LW);
  static constexpr int PLANE_A = BM * XROW, PLANE_B = BN * XROW;
  static constexpr int A_BYTES = BM * Geom::A_ROW, STAGE = A_BYTES + 2 * PLANE_B;
  static constexpr int PER_STEP = (Geom::LO_PLANE ? 2 : 1) * AJ + 2 * BJ;  // LDS-DMA instructions per K-step
  static_assert(AJ >= 1 && BJ >= 1, "tile too small for the issuing waves");
  static_assert(PER_STEP <= 31, "two K-steps of pieces must fit the 6-bit vmcnt");
  int a_off[AJ];
  unsigned a_mask[AJ];
  int a_off2[SECOND ? AJ : 1];  // second input: element offset of this lane's chunk of the row's first record, -1 = no row
  WeightRow b[BJ];
  TapCursor<SECOND> cur;
  int lw;

  __device__ __forceinline__ DmaIssuer(const ConvP& p, int m0, int n0, int lw_, int lane) : lw(lw_) {
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int row = Geom::row(lw * AJ + j, lane);
      const int c = Geom::chunk(row, lane);  // the chunk of the record that belongs at this lane's LDS position
      const int m = m0 + row;
      rec_row(p, m, c, a_off[j], a_mask[j]);
      if constexpr (SECOND) a_off2[j] = m < p.M && p.Cin2 ? m * p.Cin2 * 2 + c * 8 : -1;
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      const int row = (lw * BJ + j) * 16 + (lane >> 2);
      b[j] = weight_row(p, n0 + row, Geom::bchunk(row, lane & 3));
    }
  }
  // K-steps must be issued in order (the cursor advances)
  __device__ __forceinline__ void issue(const ConvP& p, unsigned char* smem, int kt, int buf) {
    unsigned char* ah = smem + buf * STAGE;
    unsigned char* al = ah + PLANE_A;  // (Geom::LO_PLANE)
    unsigned char* bh = ah + A_BYTES;
    unsigned char* bl = bh + PLANE_B;
    const uint16_t* zero = reinterpret_cast<const uint16_t*>(p.zero16);
    const bool second = cur.second(p);
    const int tap = cur.tap(p);
    const int tapoff = cur.offset(p) * 2;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      bool ok;
      const uint16_t* src;
      if (SECOND && second) {
        ok = a_off2[j] >= 0;
        src = ok ? p.in2_hi + (a_off2[j] + tapoff) : zero;
      } else {
        ok = (a_mask[j] >> tap) & 1u;
        src = ok ? p.in_hi + (a_off[j] + tapoff) : zero;
      }
      const int piece = (lw * AJ + j) * 1024;
      if (NODMA) continue;
      __builtin_amdgcn_global_load_lds(src, (lds_ptr)(ah + piece), 16, 0, 0);
      if (Geom::LO_PLANE) __builtin_amdgcn_global_load_lds(ok ? src + 32 : zero, (lds_ptr)(al + piece), 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      const int piece = (lw * BJ + j) * 1024;
      if (NODMA) continue;
      __builtin_amdgcn_global_load_lds(b[j].hi ? b[j].hi + (size_t)kt * XBK : zero, (lds_ptr)(bh + piece), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(b[j].lo ? b[j].lo + (size_t)kt * XBK : zero, (lds_ptr)(bl + piece), 16, 0, 0);
    }
    cur.advance(p);
  }
};

// A kernel's entry point: launch bounds, the LDS the body asks for, the body.  Non-template on purpose -- the host-side stub
// of a __global__ template that uses the LDS-DMA builtin is not emitted -- and one symbol per use: profilers and
// profiles/*.json tell the layers apart by it.  Body (last argument, may hold commas): a struct with NT, SMEM and run().
#define D2T_CONV_ENTRY(name, blocks_per_cu, ...)                                           \
  using name##_t = __VA_ARGS__;                                                            \
  __global__ __launch_bounds__(name##_t::NT, blocks_per_cu) void name(const ConvP p) {     \
    __shared__ __attribute__((aligned(1024))) unsigned char smem[name##_t::SMEM];          \
    name##_t::run(p, smem);                                                                \
  }

}  // namespace d2t
