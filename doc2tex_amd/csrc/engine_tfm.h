// Shared between engine_tfm.hip (the decode step, the captured-loop cache, the greedy decodes) and engine_tfm_beam.hip (the
// beam searches): the step and its argument structs, buffer preparation, memory staging, the graph cache and its key, and the
// refusals every TFM entry opens with.  Internal to libd2t.
#pragma once
#include "engine_impl.h"
#include "carve.h"
#include <functional>

// (hidden: these functions cross two files, but none of their symbols belongs to the library's surface)
#pragma GCC visibility push(hidden)
namespace tfm {

// the step workspace of a decode of B rows, carved out of the chain's dws
struct DecBufs {
  float* x;    // normalised layer input (x0 embedding, or LN3 of the previous layer)
  float *y1, *x1, *y2, *x2, *y3;  // pre-LayerNorm sums y* and their normalised forms x*
  float *q2, *a, *qkv, *f;
};

// device side of a ragged decode group (absorbed form): per-row tables, and where the slot keeps the bf16 planes of the packed
// memory rows -- hi at ckv + plane_elems floats, lo plane_elems elements behind it: fixed by the slot's capacity, not by the
// group's memory total, so that one captured loop serves every layout
struct RaggedDev { const int* row0; const int* len; size_t plane_elems; };
inline size_t plane_elems(const d2t_ctx* c, int slot) { return ((c->ckv2_cap[slot] - 64) / 8) & ~(size_t)255; }

// What one decode step works on (decode_step): zero-initialised, the callers set fields by name.
struct StepArgs {
  int rows = 0, T = 0;     // rows of this launch, each attending over T memory tokens (ragged: T unused)
  int kvB = 0, ckvB = 0;   // row capacity of the self-attention cache; batched beam search: ckvB samples' cross K/V (0: one per row)
  float* logits = nullptr;
  long long logit_row_stride = 0, logit_step_stride = 0;
  const int* row_map = nullptr;  // beam search: row b attends over sample row_map[b]
  const int* stop = nullptr;     // device-side early exit: the stop-at step
  int beam = 0;                  // > 0: beam search with that many hypotheses per sample, their row segments in seg
  const int *seg = nullptr, *anc = nullptr, *rows_ptr = nullptr;
  RaggedDev rg = {};             // row0 != nullptr: ragged memories
  float* ckv = nullptr;          // the memory slot this decode reads
  float* skv = nullptr;          // the self-attention cache it reads / appends
  const int* step = nullptr;     // the chain's state block: the device step counter
  // maps != nullptr (the replay of d2t_decode_cross_attention only; every decode leaves it null and enqueues what it always
  // has): the row work runs the projected-K/V one-row build that keeps its cross-attention query, and for every layer in
  // layer_mask cross_attn_probs writes this step's probabilities -- k-th chosen layer of row b at maps + b * maps_row_stride +
  // k * maps_layer_stride (+ head * maps_head_stride; 0: the head mean) + step * T.  logits == nullptr then skips the vocabulary
  struct Maps { float* maps = nullptr; long long row_stride = 0, layer_stride = 0, head_stride = 0; uint32_t layer_mask = 0; } maps;
};

// What every TFM decode entry refuses before anything is enqueued: missing arguments (have_args: the entry's own pointers and
// counts), weights not finalized, another decoder (`not_tfm`: the entry's message), a memory longer than the cap (T; 0: the
// entry checks its own lengths).  Each entry adds its extras after it.
int tfm_check(d2t_ctx* c, bool have_args, int T, const char* not_tfm);

// every decode stream has drained
hipError_t sync_chains(d2t_ctx* c);
// Buffers of a decode of B rows on chain ch (and every memory slot) at their size; the chain's workspace carved into bufs.
// mem_rows > 0 (ragged decode group, absorbed form): the slot holds that many packed memory rows instead of B * T
int dec_prepare(d2t_ctx* c, d2t_ctx::Chain& ch, int B, int T, DecBufs* bufs, size_t mem_rows = 0);
// a packed memory of n floats into a slot: the fp32 rows, and plane floats behind the slot's start their bf16 hi | lo planes
hipError_t stage_memory(float* ckv, size_t plane, const float* memory, size_t n, hipStream_t s);
// cross-attention K,V of every layer into the slot ckv, once per batch: [layers*2][B][heads][T][hd] (absorbed form: the
// memory itself and its planes)
hipError_t cross_kv(d2t_ctx* c, hipStream_t s, const float* memory, int B, int T, float* ckv);
// the projected form of it, whatever the context decodes with; exact: the fp32 GEMM even where the context's convolution
// arithmetic is split-bf16 (the replay of d2t_decode_cross_attention: scores of wide-ranged memories move by 1e-4 otherwise)
hipError_t cross_kv_projected(d2t_ctx* c, hipStream_t s, const float* memory, int B, int T, float* ckv, bool exact = false);
// one decode step for a.rows rows up to the vocabulary logits; bf.x holds the embedded input of this step
hipError_t decode_step(d2t_ctx* c, hipStream_t s, const DecBufs& bf, const StepArgs& a);
unsigned long long* trace_slot(d2t_ctx* c);

// The key of a captured loop on chain ch reading memory slot ckv: zeroed first (compared with memcmp: the padding must be
// defined), then the engine addresses; the caller adds its loop kind, outputs and (ragged) tables by name.
void graph_key(d2t_ctx::GraphKey* k, const d2t_ctx::Chain& ch, const float* ckv, int B, int T, int steps);
// The context's graph of `k` (a small cache, most recently used last); on a miss `enqueue` is captured on s, instantiated and
// cached, evicting the least recently used of 40.  `what` names the loop in an error message.
int cached_graph(d2t_ctx* c, hipStream_t s, const d2t_ctx::GraphKey& k, const char* what,
                 const std::function<hipError_t(hipStream_t)>& enqueue, hipGraphExec_t* out);

}  // namespace tfm
#pragma GCC visibility pop
