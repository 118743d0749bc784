// ViT self-attention of the recognizer path (gfx950, fp32 matrix cores).  It replaces Attention.forward of the reference's
// modules/component/feature_extractor/vision_transformer.py:61-81.
#include "conv_common.h"

namespace d2t {

// ---------------------------------------------------------------------------
// qkv [B,N,3,heads,32] -> y [B,N,heads*32], head_dim = 32.  Wave w of a block owns the 32 queries [32w, 32w+32) of one
// (image, head) and walks the 32-key tiles flash-style: S^T = K (scale Q)^T by 16 v_mfma_f32_32x32x2_f32, running maximum,
// rescale, P = exp(S - max), O += P V by 16 more MFMAs.
// The score product is taken TRANSPOSED (rows = keys, columns = this wave's 32 queries), so a lane holds, for ONE query
// (its column), 16 of the tile's 32 keys in its accumulator registers -- and that is already the A-operand layout of the
// second product when MFMA step kk is made to mean "key acc_row(kk, h)" (the V rows are simply read in that order).  No LDS
// tile for P, and the row maximum is 16 in-register maxima and one lane exchange.
// K rows are padded to 33 floats (conflict-free A-operand reads), V rows are read lane-contiguous.
// Up to 512 tokens the block holds the head's whole K / V in LDS (one chunk; grid = images x heads).  Longer sequences
// (crops beyond about 180 x 720: the shipped configurations allow up to 448 x 960 = 1695 tokens) take the same loop in
// CHUNKS of `kct` key tiles staged one after the other -- the running maximum / sum / O carry over, the keys are visited
// in the same order -- and the queries are split over `qchunks` blocks of up to 16 waves per (image, head).
// MAPS also writes the normalised probabilities (the tensor the reference's attn_drop sees, vision_transformer.py:74-76) to
// maps [B][heads][N][N]: after the loop above a second sweep recomputes every score tile with the same MFMAs and operands
// (bitwise the same S) and writes exp(S - m) / l with the final m and l.  Up to 512 tokens K is still in LDS; chunked
// launches stage K again chunk by chunk (V is not needed).  The V region becomes per-wave scratch (512 floats = 32 queries x
// 16 keys) through which each half-tile is turned from accumulator layout into 64-byte runs of keys per query row.
// ---------------------------------------------------------------------------

// register e of a lane of half h (= lane >> 5) of a 32x32 MFMA result holds row (e & 3) + 8 (e >> 2) + 4 h of the lane's column
__device__ __forceinline__ int acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// One chunk of Np keys from key t0 * 32 on into LDS: Ks [Np][33], with WITH_V also Vs [Np][32]; rows >= N are zero.
// head = the (image, head)'s first K float: K of key j at head + j * 3 C, its V row C floats further.
template <bool WITH_V>
__device__ __forceinline__ void stage_keys(float* Ks, float* Vs, const float* head, int C, int N, int t0, int Np, int tid,
                                           int nthreads) {
  for (int i = tid; i < Np * 8; i += nthreads) {  // 8 float4 per key row
    const int jl = i >> 3, j = t0 * 32 + jl, c = (i & 7) * 4;
    float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
    if (j < N) {
      kv = *reinterpret_cast<const float4*>(head + (size_t)j * 3 * C + c);
      if (WITH_V) vv = *reinterpret_cast<const float4*>(head + (size_t)j * 3 * C + C + c);
    }
    float* kd = Ks + jl * 33 + c;
    kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
    if (WITH_V) *reinterpret_cast<float4*>(Vs + jl * 32 + c) = vv;
  }
}

// S^T of tile tl of the staged chunk: register e of this lane = key acc_row(e, h) of the tile, query q0 + r.
// A operand: lane (row = key r of the tile, k = h) supplies K[tl*32 + r][2 kk + h]; B operand: qb (see the kernel)
__device__ __forceinline__ f32x16 score_tile(const float* Ks, int tl, int r, int h, const float (&qb)[16]) {
  f32x16 sacc;
#pragma unroll
  for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
  const float* ka = Ks + (size_t)(tl * 32 + r) * 33 + h;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[2 * kk], qb[kk], sacc, 0, 0, 0);
  return sacc;
}

template <bool MAPS>
__global__ __launch_bounds__(1024) void vit_attention_mfma_kernel(const float* __restrict__ qkv, float* __restrict__ y,
                                                                  float* __restrict__ maps, int N, int heads, int tiles,
                                                                  int kct, int qchunks) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int Np = kct * 32;                 // keys per staged chunk
  float* Ks = sm;                          // [Np][33]
  float* Vs = Ks + (size_t)Np * 33;        // [Np][32]
  const int bh = blockIdx.x / qchunks, qc = blockIdx.x % qchunks;
  const int b = bh / heads, hh = bh % heads, C = heads * 32;
  const float* base = qkv + (size_t)b * N * 3 * C;
  const float* khead = base + C + hh * 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nthreads = blockDim.x;
  const int r = lane & 31, h = lane >> 5, q0 = (qc * 16 + wave) * 32;
  // B operand of S^T: lane (k = h, column = query r) supplies scale * Q[q0 + r][2 kk + h]
  float qb[16];
  {
    const int row = q0 + r < N ? q0 + r : N - 1;  // clamp: queries beyond N are computed and discarded
    const float* qp = base + (size_t)row * 3 * C + hh * 32;
    const float scale = 0.17677669529663687f;     // 32^-0.5
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) qb[kk] = qp[2 * kk + h] * scale;
  }
  f32x16 o;
#pragma unroll
  for (int e = 0; e < 16; ++e) o[e] = 0.f;
  float mrun = -INFINITY, lrun = 0.f;  // of query q0 + r (both lane halves hold the same values)
  for (int t0 = 0; t0 < tiles; t0 += kct) {
    if (t0) __syncthreads();  // everyone is done with the previous chunk
    stage_keys<true>(Ks, Vs, khead, C, N, t0, Np, tid, nthreads);
    __syncthreads();
    const int tend = t0 + kct < tiles ? t0 + kct : tiles;
    for (int t = t0; t < tend; ++t) {
      const int tl = t - t0;  // tile index inside the staged chunk
      const f32x16 sacc = score_tile(Ks, tl, r, h, qb);
      float sv[16], mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        sv[e] = t * 32 + acc_row(e, h) < N ? sacc[e] : -INFINITY;
        mx = fmaxf(mx, sv[e]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // the other half of the tile's keys
      const float mnew = fmaxf(mrun, mx);      // (every tile holds at least one valid key: finite)
      const float corr = expf(mrun - mnew);    // 0 on the first tile
      float pe[16], ps = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        pe[e] = expf(sv[e] - mnew);
        ps += pe[e];
      }
      lrun = lrun * corr + ps;
      mrun = mnew;
      // O rows are queries acc_row(e, h): their correction lives in the lane of that query
#pragma unroll
      for (int e = 0; e < 16; ++e) o[e] *= __shfl(corr, acc_row(e, h), 64);
      // O += P V_t with MFMA step kk <-> key acc_row(kk, h): A[query r][k = h] = pe[kk], B[k = h][d = r] = V[that key][r]
      const float* vb = Vs + (size_t)(tl * 32 + 4 * h) * 32 + r;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(pe[kk], vb[(size_t)acc_row(kk, 0) * 32], o, 0, 0, 0);
    }
  }
  lrun += __shfl_xor(lrun, 32, 64);  // each half summed its own 16 keys per tile
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int qi = acc_row(e, h);
    const float l = __shfl(lrun, qi, 64);
    const int row = q0 + qi;
    if (row < N) y[((size_t)b * N + row) * C + hh * 32 + r] = o[e] / l;
  }
  if constexpr (MAPS) {
    __syncthreads();  // every wave is past its last P V product: the V region is scratch from here on
    float* ws = Vs + (size_t)wave * 512;       // [32 queries][16 keys], key column XOR (query >> 1): conflict-free both ways
    float* pm = maps + (size_t)bh * N * N;     // this (image, head)'s [N][N]
    const int c = lane & 15;                   // read-back: lane = key column c of query row 4 i + (lane >> 4)
    for (int t0 = 0; t0 < tiles; t0 += kct) {
      if (kct < tiles) {  // chunked launch: stage this chunk's K again
        if (t0) __syncthreads();
        stage_keys<false>(Ks, nullptr, khead, C, N, t0, Np, tid, nthreads);
        __syncthreads();
      }
      const int tend = t0 + kct < tiles ? t0 + kct : tiles;
      for (int t = t0; t < tend; ++t) {
        const f32x16 sacc = score_tile(Ks, t - t0, r, h, qb);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          // registers 8 half + i hold keys t*32 + 16 half + acc_row(i, h) of query q0 + r
#pragma unroll
          for (int i = 0; i < 8; ++i)
            ws[r * 16 + (acc_row(i, h) ^ ((r >> 1) & 15))] = expf(sacc[8 * half + i] - mrun) / lrun;
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the half-tile is visible to the whole wave
          const int key = t * 32 + 16 * half + c;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int qr = 4 * i + (lane >> 4), row = q0 + qr;
            const float p = ws[qr * 16 + (c ^ ((qr >> 1) & 15))];
            if (row < N && key < N) pm[(size_t)row * N + key] = p;  // never the zero-padded keys or the clamped queries
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  }
}

template <bool MAPS>
static hipError_t launch_vit_attention_mfma(const float* qkv, float* y, float* maps, int B, int N, int heads, hipStream_t s) {
  const int tiles = (N + 31) / 32;
  // up to 512 tokens: the whole head in one chunk, one block per (image, head);
  // beyond: 256-key chunks (66 KB: two blocks per CU) and the queries in blocks of sixteen waves
  const int kct = tiles <= 16 ? tiles : 8, qchunks = (tiles + 15) / 16, waves = tiles < 16 ? tiles : 16;
  const size_t lds = ((size_t)kct * 32 * 33 + (size_t)kct * 32 * 32) * sizeof(float);
  static_assert(16 * 32 * (33 + 32) * sizeof(float) <= 160 * 1024, "the largest chunk (kct = 16) fits the CU's LDS");
  static bool attr_set = false;  // one per instantiation: each sets the attribute of its own kernel
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(vit_attention_mfma_kernel<MAPS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL(vit_attention_mfma_kernel<MAPS>, dim3(B * heads * qchunks), dim3(waves * 64), lds, s, qkv, y, maps, N,
                     heads, tiles, kct, qchunks);
  return hipGetLastError();
}

hipError_t launch_vit_attention(const float* qkv, float* y, int B, int N, int heads, hipStream_t s) {
  return launch_vit_attention_mfma<false>(qkv, y, nullptr, B, N, heads, s);
}

hipError_t launch_vit_attention_probs(const float* qkv, float* y, float* maps, int B, int N, int heads, hipStream_t s) {
  if (!maps) return launch_vit_attention(qkv, y, B, N, heads, s);
  return launch_vit_attention_mfma<true>(qkv, y, maps, B, N, heads, s);
}

}  // namespace d2t
