// Shared between the engine*.hip files: constants and small host helpers that more than one of them needs, and the functions
// of engine_weights.hip that engine.hip calls.  Internal to libd2t.
#pragma once
#include "ctx.h"

// (hidden: these functions cross two files, but none of their symbols belongs to the library's surface)
#pragma GCC visibility push(hidden)
namespace eng {
// engine_weights.hip: the fp16 hi / lo planes of a packed convolution weight, made on the first launch that needs them
int f16_planes(d2t_ctx* c, ConvW& w, hipStream_t s);
// engine_weights.hip: frees every packed buffer and leaves the context unfinalized (re-finalize, destroy)
void free_packed(d2t_ctx* c);
// engine_weights.hip: two packed weight sets of the same Cout concatenated along K for a launch with a second input
// (ConvP::in2_hi) -- w [Co][K1 + K2] = [w1 row | w2 row], bias = b1 + b2 -- and the bf16 hi / lo planes of the result.
// pack_block's conv2 | shortcut, and the operator entry d2t_op_conv_records
hipError_t concat_k(const float* w1, const float* b1, int K1, const float* w2, const float* b2, int K2, int Co, float* w,
                    float* bias, uint16_t* w_hi, uint16_t* w_lo, hipStream_t s);
}  // namespace eng
#pragma GCC visibility pop

namespace {

// decode-group bookkeeping words behind the per-row `ended` flags of the device state array:
// [0, MAXB) per-batch end counters, [MAXB, 2 MAXB) per-batch "steps done", [2 MAXB] batches done, [2 MAXB + 1] stop-at step
constexpr int GRP_MAXB = 64, GRP_WORDS = 2 * GRP_MAXB + 2;

// Longest encoder memory a decode can attend over: 4096 tokens (the shipped max_dimension [800, 800] gives 2526).  The TFM row
// kernels walk the keys with a running softmax -- the absorbed form (d_model 256) in 16-key tiles, the projected-K/V form
// (d_model 512) in groups per lane -- and the LSTM-attention decode kernel keeps two alignment rows of that length in LDS
// (recurrent_common.h AD_MAXT).
inline int memory_cap(const d2t_ctx*) { return 4096; }

inline hipError_t linear_big(d2t_ctx* c, hipStream_t s, const float* x, const LinW& w, const float* res, float* y, int M,
                      int act) {
  ConvP p{};
  p.in = x; p.w = w.w; p.bias = w.b; p.res = res; p.out = y;
  if (c && c->conv_bf16x3 && w.w_hi) { p.w_hi = w.w_hi; p.w_lo = w.w_lo; }  // launch_conv picks the bf16x3 GEMM
  linear_shape(p, M, w.K, w.N);
  p.act = act;
  return c ? d2t_internal_conv_timed(c, p, s) : launch_conv(p, s);
}

inline hipError_t linear_any(d2t_ctx* c, hipStream_t s, const float* x, const LinW& w, const float* res, float* y, int M,
                      int act) {
  // always the MFMA GEMM when the shape allows it (not only for M > 64): a row's result must not depend on how many
  // rows share the launch, or a sample would decode differently alone and inside a batch
  if (w.K % 32 == 0) return linear_big(c, s, x, w, res, y, M, act);
  SkinnyP p{};
  p.x = x; p.w = w.w; p.bias = w.b; p.res = res; p.y = y;
  p.M = M; p.K = w.K; p.N = w.N; p.ldx = w.K; p.ldy = w.N; p.ldres = w.N; p.act = act;
  return launch_skinny(p, s);
}

// Serving ticket of an asynchronous decode whose last work is enqueued on s: its outputs are complete once the ticket's event
// has fired.  nb > 0: an early-exit decode of nb batches whose step counts lie at steps_dev (readable through d2t_decode_steps
// once the ticket is complete); nb < 0: not an early-exit decode, every batch runs -nb steps.
inline int issue_ticket(d2t_ctx* c, hipStream_t s, int nb, const int* steps_dev) {
  const int64_t t = ++c->last_ticket;
  c->decode_in_flight = true;
  const int slot = (int)(t % d2t_ctx::TICKET_RING);
  if (!c->h_steps) HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_steps), (size_t)d2t_ctx::TICKET_RING * GRP_MAXB * 4, hipHostMallocDefault));
  c->ticket_batches[slot] = nb;
  if (nb > 0) HIPCHK(c, hipMemcpyAsync(c->h_steps + (size_t)slot * GRP_MAXB, steps_dev, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
  hipEvent_t& ev = c->ticket_ev[slot];
  if (!ev) HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(ev, s));
  return D2T_OK;
}

// The pinned host staging buffer of the beam searches (c->h_beam), grown on demand.  Every search synchronises its stream
// before it returns, so the buffer is idle between calls.
inline int ensure_host_beam(d2t_ctx* c, size_t bytes) {
  if (c->h_beam_cap >= bytes) return D2T_OK;
  if (c->h_beam) hipHostFree(c->h_beam);
  c->h_beam = nullptr; c->h_beam_cap = 0;
  if (hipHostMalloc(reinterpret_cast<void**>(&c->h_beam), bytes, hipHostMallocDefault) != hipSuccess)
    return fail(c, D2T_ENOMEM, "hipHostMalloc failed");
  c->h_beam_cap = bytes;
  return D2T_OK;
}

}  // namespace
