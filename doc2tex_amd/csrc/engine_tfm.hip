// libd2t engine, TFM head: the decode step, captured step loops, greedy decodes (plain, grouped, ragged), the device-side and
// host-side beam searches and the ticket / wait / query entries of the C-ABI.  Host code only: the kernels are decode.hip's.
#include "engine_impl.h"
#include <functional>

extern "C" {

namespace {
struct DecBufs {
  float *x;    // normalised layer input (x0 embedding, or LN3 of the previous layer)
  float *y1, *x1, *y2, *x2, *y3;  // pre-LayerNorm sums y* and their normalised forms x*
  float *qkv, *q2, *a, *f;
};

// every decode stream has drained
hipError_t sync_chains(d2t_ctx* c) {
  hipError_t e = hipSuccess;
  for (int i = 0; i < d2t_ctx::MAXC && e == hipSuccess; ++i)
    if (c->chains[i].stream) e = hipStreamSynchronize(c->chains[i].stream);
  return e;
}

// Buffers of a decode of B rows on chain ch (and every memory slot) at their size; the chain's workspace carved into bufs.
// mem_rows > 0 (ragged decode group, absorbed form): the slot holds that many packed memory rows instead of B * T
int dec_prepare(d2t_ctx* c, d2t_ctx::Chain& ch, int B, int T, DecBufs* bufs, size_t mem_rows = 0) {
  const d2t_config& g = c->cfg;
  const int d = g.dec_dim, Lmax = g.max_seq_len + 2;
  int rc;
  // a slot holds the encoder memory copy [B][T][d] (absorbed cross-attention) or the projected K/V of every layer
  // (absorbed form: the fp32 rows, and behind them the same rows as bf16 hi / lo planes for the greedy two-row kernel)
  const size_t slot_rows = mem_rows ? mem_rows : (size_t)B * T;
  const size_t slot_bytes = c->dec_absorbed ? slot_rows * d * 8 + 64 : (size_t)g.dec_layers * 2 * slot_rows * d * 4;
  for (int i = 0; i < (c->n_chains > 2 ? c->n_chains : 2); ++i)
    if ((rc = ensure(c, &c->ckv2[i], &c->ckv2_cap[i], slot_bytes))) return rc;
  if ((rc = ensure(c, &ch.skv, &ch.skv_cap, (size_t)g.dec_layers * 2 * B * Lmax * d * 4))) return rc;
  const size_t per = (size_t)B * (8 * d + 3 * d + g.dec_ff);
  if ((rc = ensure(c, &ch.dws, &ch.dws_cap, per * 4))) return rc;
  if ((rc = ensure(c, &ch.dstate, &ch.dstate_cap, (size_t)(4 + B + GRP_WORDS) * 4))) return rc;
  // beam search, absorbed form: absorbed queries / context rows [B][8][d] and LN1 outputs [B][d] between the row kernel's halves
  if (c->dec_absorbed && (rc = ensure(c, &c->beam_qp, &c->beam_qp_cap, (size_t)B * 9 * d * 4))) return rc;
  float* p = ch.dws;
  float** six[] = {&bufs->x, &bufs->y1, &bufs->x1, &bufs->y2, &bufs->x2, &bufs->y3, &bufs->q2, &bufs->a};
  for (float** q : six) { *q = p; p += (size_t)B * d; }
  bufs->qkv = p; p += (size_t)B * 3 * d;
  bufs->f = p;
  return D2T_OK;
}

// device side of a ragged decode group (absorbed form): per-row tables, and where the slot keeps the bf16 planes of the packed
// memory rows -- hi at ckv + plane_elems floats, lo plane_elems elements behind it: fixed by the slot's capacity, not by the
// group's memory total, so that one captured loop serves every layout
struct RaggedDev { const int* row0; const int* len; size_t plane_elems; };
// (static, like the other new helpers: a function of an unnamed namespace inside extern "C" would still export its C name)
static size_t plane_elems(const d2t_ctx* c, int slot) { return ((c->ckv2_cap[slot] - 64) / 8) & ~(size_t)255; }

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
};

struct Lin { const float* x; int ldx; const LinW* w; const float* res; float* y; int ldy; int act; };

unsigned long long* trace_slot(d2t_ctx* c) {
  if (!c->dtrace || c->dtrace_next >= d2t_ctx::DTRACE_SLOTS) return nullptr;
  return c->dtrace + 2 * (size_t)(c->dtrace_next++);
}

hipError_t skinny(hipStream_t s, const Lin& l, int M, const LNW* ln = nullptr, float* ln_out = nullptr,
                  const int* step_ptr = nullptr, long long step_stride = 0, unsigned long long* trace = nullptr,
                  const int* stop_at = nullptr, const int* cur_step = nullptr) {
  SkinnyP p{};
  p.trace = trace;
  p.stop_at = stop_at; p.cur_step = cur_step;
  p.x = l.x; p.w = l.w->w; p.bias = l.w->b; p.res = l.res; p.y = l.y;
  p.M = M; p.K = l.w->K; p.N = l.w->N; p.ldx = l.ldx; p.ldy = l.ldy; p.ldres = l.w->N; p.act = l.act;
  p.step_ptr = step_ptr; p.out_step_stride = step_stride;
  if (ln) { p.ln_g = ln->g; p.ln_b = ln->b; p.ln_eps = 1e-5f; p.ln_out = ln_out; }
  return launch_skinny(p, s);
}

// a packed memory of n floats into a slot: the fp32 rows, and plane floats behind the slot's start their bf16 hi | lo planes
static hipError_t stage_memory(float* ckv, size_t plane, const float* memory, size_t n, hipStream_t s) {
  hipError_t e = hipMemcpyAsync(ckv, memory, n * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;
  uint16_t* hi = reinterpret_cast<uint16_t*>(ckv + plane);
  return launch_split_bf16(memory, hi, hi + plane, n, s);  // the planes of the split-bf16 cross-attention (decode.hip)
}

// cross-attention K,V of every layer into the slot ckv, once per batch: [layers*2][B][heads][T][hd]
hipError_t cross_kv(d2t_ctx* c, hipStream_t s, const float* memory, int B, int T, float* ckv) {
  const d2t_config& g = c->cfg;
  const int d = g.dec_dim;
  // absorbed form: no projection at all -- the step loop reads the memory rows; the slot keeps a copy so that the captured
  // loop holds an engine address and the caller's tensor is free again as soon as this copy has run
  if (c->dec_absorbed) return stage_memory(ckv, (size_t)B * T * d, memory, (size_t)B * T * d, s);
  ConvP p{};
  p.in = memory; p.w = c->ckv_w; p.bias = c->ckv_b; p.out = ckv;
  if (c->conv_bf16x3 && c->ckv_hi) { p.w_hi = c->ckv_hi; p.w_lo = c->ckv_lo; }
  linear_shape(p, B * T, d, g.dec_layers * 2 * d);
  p.store_mode = STORE_KV; p.kv_T = T; p.kv_heads = g.dec_heads; p.kv_hd = d / g.dec_heads; p.kv_B = B;
  return launch_conv(p, s);
}

// One decode step for M rows up to the vocabulary logits (greedy: M = B rows).
// bf.x holds the embedded input of this step.  Post-norm decoder layer
// (nn.TransformerDecoderLayer, norm_first=False): every LayerNorm is evaluated as
// the prologue of the GEMM that consumes it (which also writes the normalised rows
// needed later as the residual), so a layer is 4 launches:
//   [LN3 prev] qkv GEMM | fused row kernel (self-attn, out-proj+res, LN1, q-proj, cross-attn, out-proj+res)
//   | [LN2] ff1+ReLU GEMM | ff2+res GEMM
// All position-dependent values come from the device step counter (graph-replayable).
// beam > 0 (beam search with at most 6 hypotheses per sample, absorbed form): the row work runs as pre / per-SAMPLE cross /
// post (launch_decoder_row_beam) with the samples' row segments in `seg`.
hipError_t decode_step(d2t_ctx* c, hipStream_t s, const DecBufs& bf, const StepArgs& a) {
  const d2t_config& g = c->cfg;
  const int d = g.dec_dim, heads = g.dec_heads, hd = d / heads, Lmax = g.max_seq_len + 2;
  const int M = a.rows, T = a.T, kvB = a.kvB, ckvB = a.ckvB, beam = a.beam;
  const int *step = a.step, *stop = a.stop, *row_map = a.row_map;
  const RaggedDev* rg = a.rg.row0 ? &a.rg : nullptr;
  hipError_t e;
#define TRY(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)
  const size_t skv_layer = (size_t)kvB * heads * Lmax * hd;
  // batched beam search: ckvB samples' cross K/V, row b attends over sample row_map[b]
  const size_t ckv_slab = (size_t)(ckvB > 0 ? ckvB : kvB) * heads * T * hd;
  for (int l = 0; l < g.dec_layers; ++l) {
    const DecLayer& L = c->dec[l];
    if (l == 0) {
      TRY(skinny(s, Lin{bf.x, d, &L.sa_in, nullptr, bf.qkv, 3 * d, ACT_NONE}, M, nullptr, nullptr, nullptr, 0, trace_slot(c), stop, step));
    } else {
      TRY(skinny(s, Lin{bf.y3, d, &L.sa_in, nullptr, bf.qkv, 3 * d, ACT_NONE}, M, &c->dec[l - 1].n3, bf.x, nullptr, 0, trace_slot(c), stop, step));
    }
    DecRowP r{};
    r.qkv = bf.qkv; r.qkv_stride = 3 * d; r.xres = bf.x;
    r.sk = a.skv + (size_t)(2 * l) * skv_layer; r.sv = a.skv + (size_t)(2 * l + 1) * skv_layer;
    r.s_batch_stride = (long long)heads * Lmax * hd; r.s_Lmax = Lmax;
    r.ck = a.ckv + (size_t)(2 * l) * ckv_slab; r.cv = a.ckv + (size_t)(2 * l + 1) * ckv_slab;
    r.c_batch_stride = (long long)heads * T * hd;
    r.c_row_map = row_map;
    r.T = T;
    r.wo_t = L.sa_out_t; r.bo = L.sa_out.b; r.ln1_g = L.n1.g; r.ln1_b = L.n1.b; r.eps = 1e-5f;
    r.wq_t = L.ca_q_t; r.bq = L.ca_q.b; r.wco_t = L.ca_out_t; r.bco = L.ca_out.b;
    r.y2 = bf.y2; r.step_ptr = step; r.M = M; r.D = d; r.heads = heads;
    r.trace = trace_slot(c);
    r.stop_at = stop;
    r.anc = a.anc; r.anc_stride = Lmax; r.one_row = beam > 0;
    r.rows_ptr = a.rows_ptr;
    if (c->dec_absorbed && c->beam_shared_tile && beam > 0 && beam <= 6 && c->beam_qp && row_map)
      TRY(launch_decoder_row_beam(r, a.ckv, (long long)T * d, L.ca_wk, L.ca_v_t, L.ca_bv, c->beam_qp,
                                  c->beam_qp + (size_t)kvB * 8 * d, a.seg, ckvB, s));
    else if (c->dec_absorbed && rg) {
      const uint16_t* mhi = c->cross_fp32 ? nullptr : reinterpret_cast<const uint16_t*>(a.ckv + rg->plane_elems);
      TRY(launch_decoder_row_absorbed(r, a.ckv, 0, L.ca_wk, L.ca_v_t, L.ca_bv, s, mhi, mhi ? mhi + rg->plane_elems : nullptr, rg->row0, rg->len));
    }
    else if (c->dec_absorbed) {
      // the split-bf16 cross-attention reads the planes behind the slot's fp32 rows (cross_kv): greedy rows (two per block) and beam
      // rows (one per block, ancestry) alike
      const size_t memn = (size_t)(ckvB > 0 ? ckvB : kvB) * T * d;
      const uint16_t* mhi = c->cross_fp32 ? nullptr : reinterpret_cast<const uint16_t*>(a.ckv + memn);
      TRY(launch_decoder_row_absorbed(r, a.ckv, (long long)T * d, L.ca_wk, L.ca_v_t, L.ca_bv, s, mhi, mhi ? mhi + memn : nullptr));
    }
    else TRY(launch_decoder_row(r, s));
    TRY(skinny(s, Lin{bf.y2, d, &L.l1, nullptr, bf.f, g.dec_ff, ACT_RELU}, M, &L.n2, bf.x2, nullptr, 0, trace_slot(c), stop, step));
    TRY(skinny(s, Lin{bf.f, g.dec_ff, &L.l2, bf.x2, bf.y3, d, ACT_NONE}, M, nullptr, nullptr, nullptr, 0, trace_slot(c), stop, step));
  }
  TRY(skinny(s, Lin{bf.y3, d, &c->out_proj, nullptr, a.logits, (int)a.logit_row_stride, ACT_NONE}, M,
             &c->dec[g.dec_layers - 1].n3, nullptr, step, a.logit_step_stride, trace_slot(c), stop, step));
#undef TRY
  return hipSuccess;
}
// The context's graph of `k` (a small cache, most recently used last); on a miss `enqueue` is captured on s, instantiated and
// cached, evicting the least recently used of 40.  `what` names the loop in an error message.
int cached_graph(d2t_ctx* c, hipStream_t s, const d2t_ctx::GraphKey& k, const char* what,
                 const std::function<hipError_t(hipStream_t)>& enqueue, hipGraphExec_t* out) {
  for (size_t i = 0; i < c->graphs.size(); ++i)
    if (memcmp(&k, &c->graphs[i].key, sizeof k) == 0) {
      *out = c->graphs[i].exec;
      if (i + 1 != c->graphs.size()) std::swap(c->graphs[i], c->graphs.back());
      return D2T_OK;
    }
  c->dtrace_next = 0;  // debug timeline (D2T_DECODE_TRACE): the kernel nodes of THIS captured loop get slots 0 .. n-1
  hipGraph_t gr = nullptr;
  HIPCHK(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  hipError_t e = enqueue(s);
  hipError_t e2 = hipStreamEndCapture(s, &gr);
  if (e != hipSuccess || e2 != hipSuccess) {
    if (gr) hipGraphDestroy(gr);
    return fail(c, D2T_EHIP, "%s graph capture: %s", what, hipGetErrorString(e != hipSuccess ? e : e2));
  }
  hipGraphExec_t exec = nullptr;
  e = hipGraphInstantiate(&exec, gr, nullptr, nullptr, 0);
  hipGraphDestroy(gr);
  if (e != hipSuccess) return fail(c, D2T_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  if (c->graphs.size() >= 40) {  // evict the least recently used; it may still be queued on a decode stream
    HIPCHK(c, sync_chains(c));
    hipGraphExecDestroy(c->graphs.front().exec);
    c->graphs.erase(c->graphs.begin());
  }
  c->graphs.push_back({k, exec});
  *out = exec;
  return D2T_OK;
}

// The key of a captured loop on chain ch reading memory slot ckv: zeroed first (compared with memcmp: the padding must be
// defined), then the engine addresses; the caller adds its outputs, variant and (ragged) tables.
static void graph_key(d2t_ctx::GraphKey* k, const d2t_ctx::Chain& ch, const float* ckv, int B, int T, int steps) {
  memset(k, 0, sizeof *k);
  k->B = B; k->T = T; k->steps = steps; k->ckv = ckv; k->dws = ch.dws; k->skv = ch.skv; k->dstate = ch.dstate;
}

// Greedy decode.  The cross-attention K/V projection runs on the caller's stream into one of two slots;
// the step loop runs on the internal stream, ordered after it.  async != 0: return right after
// enqueueing (always max_seq_len+1 steps); the caller orders later work with d2t_decode_wait.
// rows_per_batch > 0 (async only): the B rows are rows_per_batch-row encoder batches decoded by one loop (a decode group);
// with is_test every batch gets its own "first step at which all ITS rows had ended", and the captured loop stops working
// once every batch has one (device-side early exit: the remaining kernels of the graph return at their first instruction).
// rg != nullptr (async only, absorbed form): a RAGGED group -- the B rows are rg->n batches of rg->rows[i] rows whose memories of
// rg->T[i] tokens lie packed in `memory` ([sum rows_i T_i][d]); T and rows_per_batch are unused.  Lengths, offsets and the
// batch layout reach the kernels through per-slot device tables, so the captured loop depends on the row total alone.
struct RaggedGroup { int n; const int32_t* rows; const int32_t* T; size_t mem_rows; };

// Fill slot `slot`'s tables for the group (host side, then one asynchronous copy on the caller's stream, which the decode
// stream is ordered behind).  The caller's stream already waits for the decode that last read this slot.
int ragged_tables(d2t_ctx* c, int slot, int B, const RaggedGroup& rg, hipStream_t user, int** tab_out) {
  if (c->rg_cap < B) {  // grow all slots together (fixed addresses between growths: they are part of the graph key)
    int cap = 1024;
    while (cap < B) cap *= 2;
    HIPCHK(c, hipDeviceSynchronize());
    for (int i = 0; i < d2t_ctx::MAXC; ++i) {
      if (c->rg_tab[i]) hipFree(c->rg_tab[i]);
      if (c->rg_host[i]) hipHostFree(c->rg_host[i]);
      c->rg_tab[i] = nullptr; c->rg_host[i] = nullptr; c->rg_ev_valid[i] = false;
    }
    c->rg_cap = 0;
    const size_t bytes = ((size_t)3 * cap + GRP_MAXB + 1) * 4;
    for (int i = 0; i < d2t_ctx::MAXC; ++i) {
      int rc = dev_alloc(c, reinterpret_cast<void**>(&c->rg_tab[i]), bytes);
      if (rc) return rc;
      if (hipHostMalloc(reinterpret_cast<void**>(&c->rg_host[i]), bytes, hipHostMallocDefault) != hipSuccess)
        return fail(c, D2T_ENOMEM, "hipHostMalloc failed");
    }
    c->rg_cap = cap;
  }
  const int cap = c->rg_cap;
  if (c->rg_ev_valid[slot]) HIPCHK(c, hipEventSynchronize(c->rg_ev[slot]));  // the previous copy out of this host buffer has run
  int* h = c->rg_host[slot];
  int *row0 = h, *len = h + cap, *row_batch = h + 2 * cap, *batch_rows = h + 3 * cap;
  int b = 0;
  long long mrow = 0;
  for (int k = 0; k < rg.n; ++k) {
    for (int i = 0; i < rg.rows[k]; ++i, ++b) {
      row0[b] = (int)(mrow + (long long)i * rg.T[k]);
      len[b] = rg.T[k];
      row_batch[b] = k;
    }
    mrow += (long long)rg.rows[k] * rg.T[k];
    batch_rows[k] = rg.rows[k];
  }
  for (int k = rg.n; k < GRP_MAXB; ++k) batch_rows[k] = 0;
  batch_rows[GRP_MAXB] = rg.n;
  HIPCHK(c, hipMemcpyAsync(c->rg_tab[slot], h, ((size_t)3 * cap + GRP_MAXB + 1) * 4, hipMemcpyHostToDevice, user));
  if (!c->rg_ev[slot]) HIPCHK(c, hipEventCreateWithFlags(&c->rg_ev[slot], hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->rg_ev[slot], user));
  c->rg_ev_valid[slot] = true;
  *tab_out = c->rg_tab[slot];
  return D2T_OK;
}

int greedy_impl(d2t_ctx* c, const float* memory, int B, int T, const int64_t* start_tokens, int is_test,
                int64_t* tokens, float* logits, int* steps_out, hipStream_t user, bool async, int rows_per_batch = 0,
                const RaggedGroup* rg = nullptr) {
  const d2t_config& g = c->cfg;
  const int S = g.max_seq_len + 1, V = g.vocab;
  if (rows_per_batch <= 0 || B % rows_per_batch) rows_per_batch = B;
  const int n_batches = rg ? rg->n : B / rows_per_batch;
  if (n_batches > GRP_MAXB) return fail(c, D2T_EINVAL, "a decode group holds at most %d batches", GRP_MAXB);  // (nothing enqueued yet)
  // memory slots rotate (at least two: the next batch's copy is written while the previous decode still reads its own);
  // async decodes rotate over the chains (chain == slot); everything else runs on chain 0
  const int nslots = c->n_chains > 2 ? c->n_chains : 2;
  const int slot = (int)(c->decode_seq++ % (unsigned)nslots);
  d2t_ctx::Chain& ch = c->chains[(async && c->n_chains > 1) ? slot % c->n_chains : 0];
  hipStream_t s = ch.stream;
  DecBufs bf;
  int rc = dec_prepare(c, ch, B, T, &bf, rg ? rg->mem_rows : 0);
  if (rc) return rc;
  float* const ckv = c->ckv2[slot];
  const bool use_graph = D2T_PROBE_ENV_STR("D2T_NO_GRAPH") == nullptr;
  int64_t* const user_tokens = tokens;
  float* const user_logits = logits;
  const size_t tok_bytes = (size_t)B * S * sizeof(int64_t), log_bytes = (size_t)B * S * V * sizeof(float);
  if (use_graph) {  // engine-owned staging [logits | tokens] on both paths: the graph key holds engine addresses only, so a
                    // caller that allocates fresh output tensors per call (Model.forward does) never forces a re-capture
    if ((rc = ensure(c, &ch.out, &ch.out_cap, log_bytes + tok_bytes))) return rc;
    logits = ch.out;
    tokens = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(ch.out) + log_bytes);
  }
  // the decode that last read this K/V slot must be finished before it is overwritten
  if (c->ev_done_valid[slot]) HIPCHK(c, hipStreamWaitEvent(user, c->ev_done[slot], 0));
  RaggedDev rgd{};
  int* rtab = nullptr;
  if (rg) {  // tables first, then the packed rows and their bf16 planes at the slot's capacity-fixed offsets
    if ((rc = ragged_tables(c, slot, B, *rg, user, &rtab))) return rc;
    rgd.row0 = rtab; rgd.len = rtab + c->rg_cap;
    rgd.plane_elems = plane_elems(c, slot);
    HIPCHK(c, stage_memory(ckv, rgd.plane_elems, memory, rg->mem_rows * g.dec_dim, user));
  } else {
    HIPCHK(c, cross_kv(c, user, memory, B, T, ckv));
  }
  // order the internal stream after the caller's work (K/V slot, start tokens, a ragged group's tables)
  HIPCHK(c, hipEventRecord(c->ev_in, user));
  HIPCHK(c, hipStreamWaitEvent(s, c->ev_in, 0));
  int* const dstate = ch.dstate;
  HIPCHK(c, hipMemsetAsync(dstate, 0, (size_t)(4 + B + GRP_WORDS) * 4, s));
  const bool dev_exit = async && is_test;  // early exit decided on the device inside the whole-loop graph
  int* grp = dstate + 4 + B;
  const int* stop = dev_exit ? grp + 2 * GRP_MAXB + 1 : nullptr;
  // step 0 input: Embedding([GO]) * sqrt(d) + pe[0]; later inputs are written by argmax_embed
  HIPCHK(c, launch_embed(c->word_embed, c->word_pe, start_tokens, tokens, S, dstate, bf.x, B, g.dec_dim, s));

  ArgmaxP am{};
  am.logits = logits; am.row_stride = (long long)S * V; am.step_stride = V;
  am.tokens = tokens; am.tok_stride = S;
  am.ended = dstate + 4; am.end_count = dstate + 1; am.steps_done = dstate + 2; am.step_ptr = dstate;
  am.B = B; am.V = V; am.end_token = TOK_END;
  am.emb = c->word_embed; am.pe = c->word_pe; am.x = bf.x; am.d = g.dec_dim;
  am.done_count = dstate + 3;
  am.rows_per_batch = rows_per_batch; am.n_batches = n_batches;
  am.batch_end_count = grp; am.batch_steps_done = grp + GRP_MAXB; am.batches_done = grp + 2 * GRP_MAXB;
  am.stop_at = dev_exit ? grp + 2 * GRP_MAXB + 1 : nullptr;
  if (rg) {  // the layout is read from the slot's tables at run time; nothing of it is baked into the captured launch
    // ArgmaxP::n_batches > 0 only says "grouped" here (ARGMAX_GROUPED): the group's real batch count is *n_batches_ptr
    am.rows_per_batch = 0; am.n_batches = ARGMAX_GROUPED;
    am.row_batch = rtab + 2 * c->rg_cap; am.batch_rows = rtab + 3 * c->rg_cap; am.n_batches_ptr = rtab + 3 * c->rg_cap + GRP_MAXB;
  }
  StepArgs sa;
  sa.rows = B; sa.T = rg ? 1 : T; sa.kvB = B;
  sa.logits = logits; sa.logit_row_stride = (long long)S * V; sa.logit_step_stride = V;
  sa.stop = stop; sa.rg = rgd; sa.ckv = ckv; sa.skv = ch.skv; sa.step = dstate;
  auto one_step = [&](hipStream_t st) -> hipError_t {
    hipError_t e = decode_step(c, st, bf, sa);
    if (e != hipSuccess) return e;
    am.trace = trace_slot(c);
    return launch_argmax_embed(am, st);
  };

  // With early exit the host polls between steps, so one captured graph = one step, replayed.  Without it
  // (async, or is_test == 0) the whole max_seq_len+1 step loop is ONE graph: a single launch per batch keeps
  // the host free to enqueue the next batch's encoder while this one decodes.
  const int steps_per_graph = (!is_test || dev_exit) ? S : 1;
  hipGraphExec_t exec = nullptr;
  if (use_graph) {
    d2t_ctx::GraphKey k;
    graph_key(&k, ch, ckv, B, T, steps_per_graph);
    k.tok = tokens; k.logits = logits;
    k.variant = (dev_exit ? 1 : 0) | ((long long)rows_per_batch << 1);
    if (rg) {  // row total + the "ragged" bit; neither T nor the batch layout
      k.T = 0; k.variant = (dev_exit ? 1 : 0) | ((long long)c->rg_cap << 8) | (1LL << 62); k.rtab = rtab; k.aux = (long long)rgd.plane_elems;
    }
    if (D2T_PROBE_ENV_STR("D2T_DECODE_TRACE") && !c->dtrace)  // debug timeline of the kernel nodes of a captured loop
      HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->dtrace), (size_t)d2t_ctx::DTRACE_SLOTS * 16));
    rc = cached_graph(c, s, k, "decode", [&](hipStream_t st) {
      hipError_t e = hipSuccess;
      for (int t = 0; t < steps_per_graph && e == hipSuccess; ++t) e = one_step(st);
      return e;
    }, &exec);
    if (rc) return rc;
  }
  int steps = S;
  // device-side early exit: the loop stops writing at the group's stop step, so define everything past it (PAD ids, zero
  // logits) instead of handing the caller whatever an earlier decode left in the staging buffer
  if (dev_exit) {
    HIPCHK(c, hipMemsetAsync(logits, 0, log_bytes, s));
    HIPCHK(c, hipMemsetAsync(tokens, 0, tok_bytes, s));
  }
  d2t_ctx::ProfRec drec{-1, B, S, nullptr, nullptr};  // profiling: the decode loop as ONE record (M = -1, N = rows, K = steps)
  if (c->profiling && hipEventCreate(&drec.a) == hipSuccess && hipEventCreate(&drec.b) == hipSuccess) HIPCHK(c, hipEventRecord(drec.a, s));
  for (int t = 0; t < S; t += (use_graph ? steps_per_graph : 1)) {
    if (use_graph) HIPCHK(c, hipGraphLaunch(exec, s));
    else HIPCHK(c, one_step(s));
    if (!async && is_test && ((t & 7) == 7 || t == S - 1)) {
      HIPCHK(c, hipMemcpyAsync(c->h_pinned, dstate + 2, 4, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipStreamSynchronize(s));
      if (c->h_pinned[0] > 0) { steps = c->h_pinned[0]; break; }
    }
  }
  if (drec.b) {
    HIPCHK(c, hipEventRecord(drec.b, s));
    c->prof.push_back(drec);
  }
  // a ragged group's batches are consumed one by one: each gets PAD / zeros from ITS OWN exit step on, as its single-batch
  // decode leaves them (the loop itself ran every row until the last batch had ended)
  if (rg && dev_exit) HIPCHK(c, launch_ragged_finalize(tokens, logits, am.row_batch, grp + GRP_MAXB, B, S, V, s));
  if (tokens != user_tokens) {
    HIPCHK(c, hipMemcpyAsync(user_logits, logits, log_bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(user_tokens, tokens, tok_bytes, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(c, hipEventRecord(c->ev_done[slot], s));
  c->ev_done_valid[slot] = true;
  if (async) {
    if ((rc = issue_ticket(c, s, dev_exit ? n_batches : -S, grp + GRP_MAXB))) return rc;
  } else {
    HIPCHK(c, hipStreamSynchronize(s));
  }
  if (steps_out) *steps_out = steps;
  return D2T_OK;
}
}  // namespace

int d2t_decode_greedy(d2t_ctx* c, const float* memory, int32_t B, int32_t T, const int64_t* start_tokens,
                      int32_t is_test, int64_t* tokens, float* logits, int32_t* steps_out, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !memory || !start_tokens || !tokens || !logits || !steps_out || B < 1 || T < 1)
    return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  if (T > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d > %d unsupported", T, memory_cap(c));
  if (c->cfg.decoder != D2T_DEC_TFM) return fail(c, D2T_ESTATE, "context was not created with the TFM decoder");
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, logits, "logits")) return rc;
  return greedy_impl(c, memory, B, T, start_tokens, is_test, tokens, logits, steps_out, (hipStream_t)stream, false);
}

int d2t_decode_greedy_async(d2t_ctx* c, const float* memory, int32_t B, int32_t T, const int64_t* start_tokens,
                            int64_t* tokens, float* logits, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !memory || !start_tokens || !tokens || !logits || B < 1 || T < 1) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  if (T > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d > %d unsupported", T, memory_cap(c));
  if (c->cfg.decoder != D2T_DEC_TFM) return fail(c, D2T_ESTATE, "context was not created with the TFM decoder");
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, logits, "logits")) return rc;
  return greedy_impl(c, memory, B, T, start_tokens, 0, tokens, logits, nullptr, (hipStream_t)stream, true);
}

int d2t_decode_greedy_submit(d2t_ctx* c, const float* memory, int32_t B, int32_t T, const int64_t* start_tokens,
                             int32_t is_test, int32_t rows_per_batch, int64_t* tokens, float* logits, d2t_stream stream,
                             int64_t* ticket_out) {
  DevGuard dg_(c);
  if (!c || !memory || !start_tokens || !tokens || !logits || B < 1 || T < 1) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  if (T > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d > %d unsupported", T, memory_cap(c));
  if (c->cfg.decoder != D2T_DEC_TFM) return fail(c, D2T_ESTATE, "context was not created with the TFM decoder");
  if (rows_per_batch < 0 || (rows_per_batch > 0 && B % rows_per_batch)) return fail(c, D2T_EINVAL, "rows_per_batch must divide the row count");
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, logits, "logits")) return rc;
  const int rc = greedy_impl(c, memory, B, T, start_tokens, is_test, tokens, logits, nullptr, (hipStream_t)stream, true, rows_per_batch);
  if (rc == D2T_OK && ticket_out) *ticket_out = c->last_ticket;
  return rc;
}

int d2t_decode_greedy_submit_ragged(d2t_ctx* c, const float* memory, int32_t n_batches, const int32_t* batch_rows,
                                    const int32_t* batch_T, const int64_t* start_tokens, int32_t is_test, int64_t* tokens,
                                    float* logits, d2t_stream stream, int64_t* ticket_out) {
  DevGuard dg_(c);
  if (!c || !memory || !batch_rows || !batch_T || !start_tokens || !tokens || !logits) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  if (c->cfg.decoder != D2T_DEC_TFM) return fail(c, D2T_ESTATE, "context was not created with the TFM decoder");
  if (n_batches > GRP_MAXB) return fail(c, D2T_EINVAL, "a decode group holds at most %d batches", GRP_MAXB);
  long long B = 0, mem_rows = 0;
  for (int k = 0; k < n_batches; ++k) {
    if (batch_rows[k] < 1) return fail(c, D2T_EINVAL, "batch %d of the group has %d rows", k, batch_rows[k]);
    if (batch_T[k] < 1) return fail(c, D2T_EINVAL, "batch %d of the group has memory length %d", k, batch_T[k]);
    if (batch_T[k] > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d > %d unsupported", batch_T[k], memory_cap(c));
    B += batch_rows[k];
    mem_rows += (long long)batch_rows[k] * batch_T[k];
  }
  if (n_batches < 1 || B < 1) return fail(c, D2T_EINVAL, "a decode group needs at least one row");
  if (B > 65535 || mem_rows > 0x7fffffffLL / 256) return fail(c, D2T_EINVAL, "decode group too large (%lld rows, %lld memory rows)", B, mem_rows);
  if (!c->dec_absorbed)
    return fail(c, D2T_ESTATE, "ragged decode groups need the absorbed cross-attention (d_model 256, 8 heads): this decoder lays its "
                               "projected cross K/V out by memory length, so batches of different lengths cannot share a loop");
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, logits, "logits")) return rc;
  if (int rc = check_dev_ptr(c, tokens, "tokens")) return rc;
  if (int rc = check_dev_ptr(c, start_tokens, "start_tokens")) return rc;
  const RaggedGroup rg{n_batches, batch_rows, batch_T, (size_t)mem_rows};
  const int rc = greedy_impl(c, memory, (int)B, 0, start_tokens, is_test, tokens, logits, nullptr, (hipStream_t)stream, true, 0, &rg);
  if (rc == D2T_OK && ticket_out) *ticket_out = c->last_ticket;
  return rc;
}

// 1: this context decodes ragged groups (TFM decoder on the absorbed cross-attention); 0: d2t_decode_greedy_submit_ragged refuses
int32_t d2t_decode_supports_ragged(const d2t_ctx* c) { return c && c->cfg.decoder == D2T_DEC_TFM && c->dec_absorbed ? 1 : 0; }

// captured decode loops the context holds (tests: a ragged group re-uses one loop for every layout with the same row total)
int32_t d2t_decode_graph_count(const d2t_ctx* c) { return c ? (int32_t)c->graphs.size() : 0; }

int d2t_decode_wait(d2t_ctx* c, d2t_stream stream, int32_t host_sync) {
  DevGuard dg_(c);
  if (!c) return D2T_EINVAL;
  for (int i = 0; i < d2t_ctx::MAXC; ++i)
    if (c->ev_done_valid[i]) HIPCHK(c, hipStreamWaitEvent((hipStream_t)stream, c->ev_done[i], 0));
  if (host_sync) {
    HIPCHK(c, sync_chains(c));
    c->decode_in_flight = false;
  }
  return D2T_OK;
}

int64_t d2t_decode_last_ticket(const d2t_ctx* c) { return c ? c->last_ticket : 0; }

// debug (undocumented, env D2T_DECODE_TRACE): reset / read the per-kernel-node timeline of the most recently captured loop
int d2t_debug_trace(d2t_ctx* c, unsigned long long* out, int32_t max_slots, int32_t reset) {
  DevGuard dg_(c);
  if (!c || !c->dtrace) return 0;
  hipDeviceSynchronize();
  const int n = std::min<int>(max_slots, c->dtrace_next);
  if (out && n > 0) hipMemcpy(out, c->dtrace, (size_t)n * 16, hipMemcpyDeviceToHost);
  if (reset) {
    std::vector<unsigned long long> init((size_t)d2t_ctx::DTRACE_SLOTS * 2);
    for (size_t i = 0; i < init.size(); i += 2) { init[i] = ~0ull; init[i + 1] = 0; }
    hipMemcpy(c->dtrace, init.data(), init.size() * 8, hipMemcpyHostToDevice);
  }
  return n;
}

// 1: the decode with this ticket has completed; 0: still running; < 0: error.  Tickets older than the event ring are
// complete by construction: a chain is an in-order stream and the ring holds TICKET_RING >> 2 chains' worth of decodes.
int d2t_decode_query(d2t_ctx* c, int64_t ticket) {
  DevGuard dg_(c);
  if (!c || ticket < 1 || ticket > c->last_ticket) return -D2T_EINVAL;
  if (ticket + d2t_ctx::TICKET_RING <= c->last_ticket) return 1;
  const hipError_t e = hipEventQuery(c->ticket_ev[ticket % d2t_ctx::TICKET_RING]);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
  fail(c, D2T_EHIP, "hipEventQuery: %s", hipGetErrorString(e));
  return -D2T_EHIP;
}

// Decode steps of the batches of one asynchronous decode (blocks until that decode is complete): for an is_test decode the
// first step at which all rows of batch k had emitted [s] (max_seq_len + 1 if that never happened); otherwise max_seq_len + 1.
// n_out receives the number of batches in the decode's group.
int d2t_decode_steps(d2t_ctx* c, int64_t ticket, int32_t* steps_out, int32_t max_batches, int32_t* n_out) {
  DevGuard dg_(c);
  if (!c || !steps_out || ticket < 1 || ticket > c->last_ticket) return fail(c, D2T_EINVAL, "unknown decode ticket %lld", (long long)ticket);
  if (ticket + d2t_ctx::TICKET_RING <= c->last_ticket) return fail(c, D2T_ESTATE, "decode ticket %lld is too old", (long long)ticket);
  const int slot = (int)(ticket % d2t_ctx::TICKET_RING);
  HIPCHK(c, hipEventSynchronize(c->ticket_ev[slot]));
  const int nb = c->ticket_batches[slot];
  const int S = c->cfg.max_seq_len + 1;
  if (nb < 0) {  // not an early-exit decode: one entry, all steps (-nb: the step count of that decode's head)
    if (max_batches < 1) return fail(c, D2T_EINVAL, "steps_out too small");
    steps_out[0] = -nb;
    if (n_out) *n_out = 1;
    return D2T_OK;
  }
  if (nb > max_batches) return fail(c, D2T_EINVAL, "steps_out holds %d entries, the decode has %d batches", max_batches, nb);
  for (int k = 0; k < nb; ++k) {
    const int v = c->h_steps[(size_t)slot * GRP_MAXB + k];
    steps_out[k] = v > 0 ? v : S;
  }
  if (n_out) *n_out = nb;
  return D2T_OK;
}

int d2t_decode_wait_ticket(d2t_ctx* c, int64_t ticket, d2t_stream stream, int32_t host_sync) {
  DevGuard dg_(c);
  if (!c || ticket < 1 || ticket > c->last_ticket) return fail(c, D2T_EINVAL, "unknown decode ticket %lld", (long long)ticket);
  if (ticket + d2t_ctx::TICKET_RING <= c->last_ticket) return D2T_OK;  // long since complete
  hipEvent_t ev = c->ticket_ev[ticket % d2t_ctx::TICKET_RING];
  HIPCHK(c, hipStreamWaitEvent((hipStream_t)stream, ev, 0));
  if (host_sync) HIPCHK(c, hipEventSynchronize(ev));
  return D2T_OK;
}


// Host arithmetic of the ragged beam search's per-sample tables: sample i's memory occupies the T[i] packed rows from
// row0[i] = T[0] + .. + T[i-1] on.  Returns the packed row total (no device, no context: also the tests' reference point).
int64_t d2t_ragged_beam_tables(int32_t N, const int32_t* T, int32_t* row0_out, int32_t* len_out) {
  int64_t at = 0;
  for (int i = 0; i < N; ++i) {
    if (row0_out) row0_out[i] = (int32_t)at;
    if (len_out) len_out[i] = T[i];
    at += T[i];
  }
  return at;
}

namespace {
// forward_beam (tfm.py:145-186) + Beam (tools/beam.py:38-140) for N samples with the bookkeeping ON THE DEVICE (round 4):
// the hypotheses of all samples are rows of one step loop, every kernel of a step is launched for the full N x beam row slots
// and reads the live row count / the stop step from the state block (kernels.h BeamDev), beam_dev_advance_kernel does
// Beam.advance for every sample after the per-sample top-k -- no host round trip in the loop, which is therefore ONE captured
// graph per (N, T, beam).  The host walks the (parent, token) history back once at the end.  Needs the absorbed row kernel
// with ancestry rows (no cache copy).  Row results are those of the host-side loop bit for bit (same kernels per row).
//
// Ts != nullptr (host [N]): the RAGGED search -- sample i's memory has Ts[i] tokens and `memory` holds the N memories packed
// ([sum Ts][d]); T is unused.  The only kernel of the loop that knows a memory length is the row kernel's cross-attention, and
// its per-sample ragged build reads (first packed row, length) of row b's sample map[b] from the context's beam tables
// (d2t_ctx::brg_tab), so the captured loop depends on N and the beam width alone and every sample's rows compute what its own
// d2t_decode_beam call computes.  The tables are written on the caller's stream in front of ev_in; the search synchronises
// before it returns, so no loop in flight ever sees them change.
constexpr int BEAM_MAX_N = 1024;
int beam_device_impl(d2t_ctx* c, const float* memory, int N, int T, int beam_size, int64_t* seq_out, int32_t* len_out,
                     float* score_out, hipStream_t user, const int32_t* Ts = nullptr) {
  const d2t_config& g = c->cfg;
  const int S = g.max_seq_len + 1, V = g.vocab, d = g.dec_dim, cap = N * beam_size, Lmax = g.max_seq_len + 2;
  if (N > BEAM_MAX_N) return fail(c, D2T_EINVAL, "batched beam search takes at most 1024 samples per call");
  d2t_ctx::Chain& ch = c->chains[0];
  hipStream_t s = ch.stream;
  DecBufs bf;
  size_t mem_rows = 0;
  for (int i = 0; Ts && i < N; ++i) mem_rows += (size_t)Ts[i];
  int rc = dec_prepare(c, ch, cap, Ts ? 1 : T, &bf, mem_rows);
  if (rc) return rc;
  float* const ckv = c->ckv2[0];  // the internal stream is in order, so earlier decodes are done with the slot
  int* const dstate = ch.dstate;
  if (Ts && !c->brg_cap) {  // [row0 | len] for the largest N, allocated once: the address is part of the graph key
    if (!c->brg_tab && (rc = dev_alloc(c, reinterpret_cast<void**>(&c->brg_tab), (size_t)2 * BEAM_MAX_N * 4))) return rc;
    if (hipHostMalloc(reinterpret_cast<void**>(&c->brg_host), (size_t)2 * BEAM_MAX_N * 4, hipHostMallocDefault) != hipSuccess) {
      c->brg_host = nullptr;
      return fail(c, D2T_ENOMEM, "hipHostMalloc failed");
    }
    memset(c->brg_host, 0, (size_t)2 * BEAM_MAX_N * 4);
    c->brg_cap = BEAM_MAX_N;
  }
  // workspace (4-byte words unless noted): logits [cap][V] | topv [cap] | topi [cap] | tok [cap] i64 | scores | map | prev [cap]
  // | seg [N][3] | ctrl [8] | comp_n, fin [N] | comp_t, comp_par, comp_score [N][beam] | hist_par, hist_tok [S][cap] | anc [2][cap][Lmax]
  size_t w = 0;
  auto take = [&](size_t words) { const size_t at = w; w += (words + 3) & ~(size_t)3; return at; };
  const size_t o_logits = take((size_t)cap * V), o_topv = take(cap), o_topi = take(cap), o_tok = take(2 * (size_t)cap);
  const size_t o_res = w;  // ---- from here to o_anc: the block copied back to the host at the end ----
  const size_t o_scores = take(cap), o_seg = take(3 * (size_t)N), o_ctrl = take(8), o_compn = take(N), o_fin = take(N);
  const size_t o_ct = take(cap), o_cp = take(cap), o_cs = take(cap), o_hp = take((size_t)S * cap), o_ht = take((size_t)S * cap);
  const size_t o_map = take(cap), o_prev = take(cap);
  const size_t res_words = o_map - o_res;
  const size_t o_anc = take(2 * (size_t)cap * Lmax);
  if ((rc = ensure(c, &c->beam_ws, &c->beam_ws_cap, w * 4 + 64))) return rc;
  float* base = c->beam_ws;
  float* d_logits = base + o_logits;
  BeamDev b{};
  b.ctrl = reinterpret_cast<int*>(base + o_ctrl);
  b.tok = reinterpret_cast<int64_t*>(base + o_tok);
  b.scores = base + o_scores;
  b.map = reinterpret_cast<int*>(base + o_map);
  b.prev = reinterpret_cast<int*>(base + o_prev);
  b.seg = reinterpret_cast<int*>(base + o_seg);
  b.comp_n = reinterpret_cast<int*>(base + o_compn);
  b.fin = reinterpret_cast<int*>(base + o_fin);
  b.comp_t = reinterpret_cast<int*>(base + o_ct);
  b.comp_par = reinterpret_cast<int*>(base + o_cp);
  b.comp_score = base + o_cs;
  b.hist_par = reinterpret_cast<int*>(base + o_hp);
  b.hist_tok = reinterpret_cast<int*>(base + o_ht);
  b.topv = base + o_topv;
  b.topi = reinterpret_cast<const int*>(base + o_topi);
  b.N = N; b.beam = beam_size; b.cap = cap; b.V = V; b.S = S; b.end_token = TOK_END;
  int* d_anc[2] = {reinterpret_cast<int*>(base + o_anc), reinterpret_cast<int*>(base + o_anc) + (size_t)cap * Lmax};
  const int* rows_ptr = b.ctrl + 1;
  const int* stop = b.ctrl + 2;
  if ((rc = ensure_host_beam(c, res_words * 4))) return rc;
  RaggedDev rgd{};
  if (Ts) {  // (the previous search has synchronised: neither copy of the tables is in use)
    d2t_ragged_beam_tables(N, Ts, c->brg_host, c->brg_host + c->brg_cap);
    HIPCHK(c, hipMemcpyAsync(c->brg_tab, c->brg_host, (size_t)2 * c->brg_cap * 4, hipMemcpyHostToDevice, user));
    rgd.row0 = c->brg_tab; rgd.len = c->brg_tab + c->brg_cap;
    rgd.plane_elems = plane_elems(c, 0);
  }
  HIPCHK(c, hipEventRecord(c->ev_in, user));
  HIPCHK(c, hipStreamWaitEvent(s, c->ev_in, 0));
  // ragged: the packed rows once, their bf16 planes at the slot's capacity-fixed offsets (as a ragged greedy group)
  if (Ts) HIPCHK(c, stage_memory(ckv, rgd.plane_elems, memory, mem_rows * d, s));
  else HIPCHK(c, cross_kv(c, s, memory, N, T, ckv));
  StepArgs sa;
  sa.rows = cap; sa.T = Ts ? 1 : T; sa.kvB = cap; sa.ckvB = N;
  sa.logits = d_logits; sa.logit_row_stride = V;
  sa.row_map = b.map; sa.stop = stop; sa.beam = beam_size; sa.seg = b.seg; sa.rows_ptr = rows_ptr;
  sa.rg = rgd; sa.ckv = ckv; sa.skv = ch.skv; sa.step = dstate;
  auto enqueue_loop = [&](hipStream_t st) -> hipError_t {
    hipError_t e;
#define LTRY(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)
    LTRY(hipMemsetAsync(dstate, 0, (size_t)(4 + cap) * 4, st));
    LTRY(launch_beam_dev_init(b, TOK_GO, st));
    for (int step = 0; step < S; ++step) {
      LTRY(launch_beam_ancestry(d_anc[(step + 1) & 1], d_anc[step & 1], b.prev, cap, Lmax, b.ctrl, dstate, st, rows_ptr, stop));
      LTRY(launch_embed_tokens(c->word_embed, c->word_pe, b.tok, dstate, bf.x, cap, d, st, rows_ptr, stop));
      sa.anc = d_anc[step & 1];
      LTRY(decode_step(c, st, bf, sa));
      LTRY(launch_beam_topk_batch(d_logits, b.scores, b.seg, N, V, beam_size, base + o_topv, reinterpret_cast<int*>(base + o_topi), st,
                                  dstate, stop));
      LTRY(launch_beam_dev_advance(b, st));
    }
#undef LTRY
    return hipSuccess;
  };
  const bool use_graph = D2T_PROBE_ENV_STR("D2T_NO_GRAPH") == nullptr;
  if (use_graph) {
    d2t_ctx::GraphKey k;
    graph_key(&k, ch, ckv, cap, T, S);
    k.logits = base;
    k.variant = 3 | ((long long)N << 8) | ((long long)beam_size << 40);  // (bits 0-1 = 3: the device-side beam loop)
    if (Ts) {  // N, beam and the "ragged" bit; no memory length
      k.T = 0; k.variant |= 1LL << 62; k.rtab = c->brg_tab; k.aux = (long long)rgd.plane_elems;
    }
    hipGraphExec_t exec = nullptr;
    if ((rc = cached_graph(c, s, k, "beam", enqueue_loop, &exec))) return rc;
    HIPCHK(c, hipGraphLaunch(exec, s));
  } else {
    HIPCHK(c, enqueue_loop(s));
  }
  HIPCHK(c, hipMemcpyAsync(c->h_beam, base + o_res, res_words * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  // ---- host: pick every sample's best hypothesis (beam.py:107-140) and walk its tokens back through the history ----
  const char* hb = c->h_beam;
  auto hw = [&](size_t off) { return reinterpret_cast<const int*>(hb + (off - o_res) * 4); };
  const float* h_scores = reinterpret_cast<const float*>(hw(o_scores));
  const int *h_seg = hw(o_seg), *h_ctrl = hw(o_ctrl), *h_compn = hw(o_compn), *h_ct = hw(o_ct), *h_cp = hw(o_cp);
  const float* h_cs = reinterpret_cast<const float*>(hw(o_cs));
  const int *h_hp = hw(o_hp), *h_ht = hw(o_ht);
  const int steps_run = h_ctrl[3];
  for (int i = 0; i < N; ++i) {
    int64_t* out = seq_out + (size_t)i * S;
    const int nc = h_compn[i];
    int row, last_step, n;  // the hypothesis ends with the history record (last_step, row); n tokens are returned
    float score;
    if (nc > 0) {
      int best = 0;
      for (int j = 1; j < nc; ++j)
        if ((double)h_cs[(size_t)i * beam_size + j] / (double)(h_ct[(size_t)i * beam_size + j] + 1) >
            (double)h_cs[(size_t)i * beam_size + best] / (double)(h_ct[(size_t)i * beam_size + best] + 1))
          best = j;
      const int t = h_ct[(size_t)i * beam_size + best];
      n = std::min(t + 1, S);
      for (int j = 0; j < n; ++j) out[j] = TOK_PAD;
      if (t < n) out[t] = TOK_END;
      row = h_cp[(size_t)i * beam_size + best];
      last_step = t - 1;
      score = h_cs[(size_t)i * beam_size + best];
    } else {  // Beam.set_hypothesis (beam.py:132-140): the first live hypothesis, padded to max_seq_len + 1
      n = S;
      for (int j = 0; j < n; ++j) out[j] = TOK_PAD;
      if (h_seg[3 * i + 1] > 0) { row = h_seg[3 * i]; last_step = steps_run - 1; score = h_scores[row]; }
      else { row = -1; last_step = -1; score = 0.f; }
    }
    for (int p = last_step; p >= 0 && row >= 0; --p) {
      if (p < n) out[p] = h_ht[(size_t)p * cap + row];
      row = h_hp[(size_t)p * cap + row];
    }
    len_out[i] = n;
    score_out[i] = score;
  }
  return D2T_OK;
}
}  // namespace

// 1: d2t_decode_beam_batch_ragged serves this context (the device-side beam loop: TFM decoder, absorbed cross-attention, one
// row per block with ancestry rows); 0: it refuses with D2T_ESTATE
int32_t d2t_decode_supports_ragged_beam(const d2t_ctx* c) {
  return c && c->cfg.decoder == D2T_DEC_TFM && c->dec_absorbed && !c->beam_shared_tile && c->cfg.max_seq_len + 2 <= 512 ? 1 : 0;
}

int d2t_decode_beam_batch_ragged(d2t_ctx* c, const float* memory, int32_t N, const int32_t* T, int32_t beam_size, int64_t* seq_out,
                                 int32_t* len_out, float* score_out, d2t_stream stream) {
  DevGuard dg_(c);
  // d2t_decode_beam_batch for N samples whose memories have DIFFERENT lengths, packed in `memory` -- one step loop, one captured
  // graph per (N, beam).  Everything is checked before anything is enqueued; the context stays usable after a refusal.
  if (!c || !memory || !T || !seq_out || !len_out || !score_out) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  if (c->cfg.decoder != D2T_DEC_TFM) return fail(c, D2T_ESTATE, "beam search is implemented for the TFM decoder only");
  if (N < 1 || N > BEAM_MAX_N) return fail(c, D2T_EINVAL, "ragged beam search takes 1 to %d samples per call, got %d", BEAM_MAX_N, N);
  if (beam_size < 1 || beam_size > 16) return fail(c, D2T_EINVAL, "beam_size must be in [1,16]");
  for (int i = 0; i < N; ++i)
    if (T[i] < 1 || T[i] > memory_cap(c))
      return fail(c, D2T_EINVAL, "sample %d has memory length %d, supported are 1 to %d", i, T[i], memory_cap(c));
  if ((long long)beam_size * c->cfg.vocab > 16 * 4096) return fail(c, D2T_EINVAL, "beam_size * vocab too large");
  if (!d2t_decode_supports_ragged_beam(c))
    return fail(c, D2T_ESTATE, "ragged beam search needs the device-side beam loop (d_model 256 with 8 heads on the absorbed "
                               "cross-attention, no beam_shared_tile, max_seq_len + 2 <= 512): call d2t_decode_beam_batch once per "
                               "memory length instead");
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  return beam_device_impl(c, memory, N, 0, beam_size, seq_out, len_out, score_out, (hipStream_t)stream, T);
}

int d2t_decode_beam(d2t_ctx* c, const float* memory, int32_t T, int32_t beam_size, int64_t* seq_out, int32_t* len_out,
                    float* score_out, d2t_stream stream) {
  DevGuard dg_(c);
  // TransformerPrediction.forward_beam (tfm.py:145-186) with tools/beam.py:38-140 bookkeeping, a fresh beam per call (demo
  // reset_beam semantics): the batched search with N = 1.
  return d2t_decode_beam_batch(c, memory, 1, T, beam_size, seq_out, len_out, score_out, stream);
}

int d2t_decode_beam_batch(d2t_ctx* c, const float* memory, int32_t N, int32_t T, int32_t beam_size, int64_t* seq_out,
                          int32_t* len_out, float* score_out, d2t_stream stream) {
  DevGuard dg_(c);
  // forward_beam (tfm.py:145-186) + Beam (tools/beam.py) for N samples AT ONCE: the hypotheses of all samples are rows
  // of one step loop (each row attends over its own sample's cross K/V through a row map), log_softmax + top-k run per
  // sample segment, the bookkeeping of every sample is the single-sample one (d2t_decode_beam is this search with N = 1).
  // The absorbed d_model-256 decoder runs it on the device (beam_device_impl); the others (d_model 512) and
  // beam_shared_tile keep this host-side loop with one round trip per step.
  if (!c || !memory || !seq_out || !len_out || !score_out || N < 1 || T < 1) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  if (beam_size < 1 || beam_size > 16) return fail(c, D2T_EINVAL, "beam_size must be in [1,16]");
  if (c->cfg.decoder != D2T_DEC_TFM) return fail(c, D2T_ESTATE, "beam search is implemented for the TFM decoder only");
  if (T > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d > %d unsupported", T, memory_cap(c));
  const d2t_config& g = c->cfg;
  const int S = g.max_seq_len + 1, V = g.vocab, d = g.dec_dim, cap = N * beam_size;
  const int heads = g.dec_heads, hd = d / heads, Lmax = g.max_seq_len + 2;
  if ((long long)beam_size * V > 16 * 4096) return fail(c, D2T_EINVAL, "beam_size * vocab too large");
  if (c->dec_absorbed && !c->beam_shared_tile && Lmax <= 512 && N <= 1024 && D2T_PROBE_ENV_STR("D2T_BEAM_HOST") == nullptr)
    return beam_device_impl(c, memory, N, T, beam_size, seq_out, len_out, score_out, (hipStream_t)stream);
  d2t_ctx::Chain& ch = c->chains[0];
  hipStream_t user = (hipStream_t)stream, s = ch.stream;
  DecBufs bf;
  int rc = dec_prepare(c, ch, cap, T, &bf);
  if (rc) return rc;
  int* const dstate = ch.dstate;
  // Round 3: with the absorbed row kernel the self-attention cache is never copied -- every hypothesis keeps an ancestry row
  // (which cache row holds each of its earlier positions, launch_beam_ancestry); otherwise the survivors' caches are gathered
  // into the other buffer as before.
  const bool use_anc = c->dec_absorbed && !c->beam_shared_tile && Lmax <= 512 && D2T_PROBE_ENV_STR("D2T_BEAM_CACHE_COPY") == nullptr;
  const size_t skv_bytes = (size_t)g.dec_layers * 2 * cap * Lmax * d * 4;
  if (!use_anc && (rc = ensure(c, &c->skv_alt, &c->skv_alt_cap, skv_bytes))) return rc;
  // workspace: logits [cap][V] | topv [cap] | topi [cap] | step pack (one host -> device copy per step):
  //   tok [cap] i64 | scores [cap] | rowmap [cap] | prev [cap] | seg [N][3] | step [4] | ancestry [2][cap][Lmax]
  const size_t pack_off = (((size_t)cap * V + 2 * (size_t)cap) * 4 + 15) & ~(size_t)15;
  const size_t pack_bytes = ((size_t)cap * (8 + 3 * 4) + (size_t)N * 12 + 16 + 15) & ~(size_t)15;
  const size_t anc_words = use_anc ? 2 * (size_t)cap * Lmax : 0;
  const size_t ws_bytes = pack_off + pack_bytes + anc_words * 4 + 64;
  if ((rc = ensure(c, &c->beam_ws, &c->beam_ws_cap, ws_bytes))) return rc;
  float* d_logits = c->beam_ws;
  float* d_topv = d_logits + (size_t)cap * V;
  int* d_topi = reinterpret_cast<int*>(d_topv + cap);
  char* d_pack = reinterpret_cast<char*>(c->beam_ws) + pack_off;
  int64_t* d_tok = reinterpret_cast<int64_t*>(d_pack);
  float* d_scores = reinterpret_cast<float*>(d_tok + cap);
  int* d_map = reinterpret_cast<int*>(d_scores + cap);
  int* d_prev = d_map + cap;
  int* d_seg = d_prev + cap;
  int* d_step = d_seg + 3 * (size_t)N;
  int* d_anc[2] = {reinterpret_cast<int*>(d_pack + pack_bytes), reinterpret_cast<int*>(d_pack + pack_bytes) + (size_t)cap * Lmax};
  if ((rc = ensure_host_beam(c, pack_bytes + 2 * (size_t)cap * 4))) return rc;
  char* hp = c->h_beam;
  int64_t* h_tok = reinterpret_cast<int64_t*>(hp);
  float* h_scores = reinterpret_cast<float*>(h_tok + cap);
  int* h_map = reinterpret_cast<int*>(h_scores + cap);
  int* h_prev = h_map + cap;
  int* h_seg = h_prev + cap;
  int* h_step = h_seg + 3 * (size_t)N;
  float* h_topv = reinterpret_cast<float*>(hp + pack_bytes);  // [topv | topi]: one device -> host copy per step
  int* h_topi = reinterpret_cast<int*>(h_topv + cap);
  HIPCHK(c, hipEventRecord(c->ev_in, user));
  HIPCHK(c, hipStreamWaitEvent(s, c->ev_in, 0));
  HIPCHK(c, hipMemsetAsync(dstate, 0, (size_t)(4 + cap) * 4, s));
  HIPCHK(c, cross_kv(c, s, memory, N, T, c->ckv2[0]));
  StepArgs sa;
  sa.T = T; sa.kvB = cap; sa.ckvB = N;
  sa.logits = d_logits; sa.logit_row_stride = V;
  sa.row_map = d_map; sa.beam = beam_size; sa.seg = d_seg;
  sa.ckv = c->ckv2[0]; sa.skv = ch.skv; sa.step = dstate;
  float* skv_other = c->skv_alt;

  // Beam bookkeeping (tools/beam.py:68-105) on a token trie: a hypothesis is (score, node); its sequence is the path to the
  // root, written out once at the end (the reference concatenates the sequences every step)
  struct Node { int parent; int64_t tok; int len; };
  struct Hyp { int node; float score; };
  std::vector<Node> trie;
  trie.reserve((size_t)cap * S);
  auto seq_len = [&](int node) { return node < 0 ? 0 : trie[(size_t)node].len; };
  std::vector<std::vector<Hyp>> hyps((size_t)N, std::vector<Hyp>(1, Hyp{-1, 0.f})), completed((size_t)N);
  std::vector<std::vector<int64_t>> last((size_t)N, std::vector<int64_t>{TOK_GO});
  std::vector<char> finished((size_t)N, 0);
  int nprev = 0;  // survivors of the previous step, in this step's row order: h_prev[0 .. nprev)
  for (int step = 0; step < S; ++step) {
    int rows = 0;
    for (int i = 0; i < N; ++i) {
      const int M = finished[i] ? 0 : (int)hyps[i].size();
      h_seg[3 * i] = rows; h_seg[3 * i + 1] = M; h_seg[3 * i + 2] = finished[i] ? 0 : beam_size - (int)completed[i].size();
      for (int j = 0; j < M; ++j) { h_tok[rows + j] = last[i][j]; h_scores[rows + j] = hyps[i][j].score; h_map[rows + j] = i; }
      rows += M;
    }
    if (!rows) break;
    if (step > 0 && nprev != rows) return fail(c, D2T_ESTATE, "beam bookkeeping: %d survivors, %d rows", nprev, rows);
    *h_step = step;
    HIPCHK(c, hipMemcpyAsync(d_pack, hp, pack_bytes, hipMemcpyHostToDevice, s));
    if (use_anc) {
      HIPCHK(c, launch_beam_ancestry(d_anc[(step + 1) & 1], d_anc[step & 1], d_prev, rows, Lmax, d_step, dstate, s));
    } else {
      HIPCHK(c, launch_beam_ancestry(nullptr, nullptr, d_prev, 1, 0, d_step, dstate, s));  // publishes the step only
      if (step > 0) {  // the survivors' caches move to their new row positions
        HIPCHK(c, launch_cache_gather(sa.skv, skv_other, d_prev, g.dec_layers * 2, cap, rows, heads, Lmax, hd, step, s));
        std::swap(sa.skv, skv_other);
      }
    }
    HIPCHK(c, launch_embed_tokens(c->word_embed, c->word_pe, d_tok, dstate, bf.x, rows, d, s));
    sa.rows = rows; sa.anc = use_anc ? d_anc[step & 1] : nullptr;
    HIPCHK(c, decode_step(c, s, bf, sa));
    HIPCHK(c, launch_beam_topk_batch(d_logits, d_scores, d_seg, N, V, beam_size, d_topv, d_topi, s));
    HIPCHK(c, hipMemcpyAsync(h_topv, d_topv, 2 * (size_t)cap * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    nprev = 0;
    for (int i = 0; i < N; ++i) {  // Beam.advance (tools/beam.py:68-105) per sample
      if (finished[i]) continue;
      const int off = h_seg[3 * i], live = h_seg[3 * i + 2];
      std::vector<Hyp> next;
      std::vector<int64_t> nl;
      const int first_prev = nprev;
      for (int r = 0; r < live; ++r) {
        const int idx = h_topi[(size_t)i * beam_size + r], prev = idx / V, word = idx % V;
        const int parent = hyps[i][prev].node;
        trie.push_back(Node{parent, (int64_t)word, seq_len(parent) + 1});
        const Hyp h{(int)trie.size() - 1, h_topv[(size_t)i * beam_size + r]};
        if (word == TOK_END) {
          completed[i].push_back(h);
        } else {
          nl.push_back(word);
          h_prev[nprev++] = off + prev;
          next.push_back(h);
        }
      }
      hyps[i].swap(next);
      last[i].swap(nl);
      if ((int)completed[i].size() == beam_size) { finished[i] = 1; nprev = first_prev; }  // Beam.done: its rows drop out
    }
  }
  HIPCHK(c, hipStreamSynchronize(s));
  for (int i = 0; i < N; ++i) {
    std::vector<Hyp>& comp = completed[i];
    bool padded = false;
    if (comp.empty()) {  // Beam.set_hypothesis (beam.py:132-140): the first live hypothesis, padded to max_seq_len + 1
      comp.push_back(hyps[i].empty() ? Hyp{-1, 0.f} : hyps[i][0]);
      padded = true;
    }
    auto len_of = [&](const Hyp& h) { return padded ? (size_t)g.max_seq_len + 1 : (size_t)seq_len(h.node); };
    size_t best = 0;
    for (size_t j = 1; j < comp.size(); ++j)
      if ((double)comp[j].score / (double)std::max<size_t>(1, len_of(comp[j])) >
          (double)comp[best].score / (double)std::max<size_t>(1, len_of(comp[best])))
        best = j;
    const Hyp& bh = comp[best];
    const int have = seq_len(bh.node), n = (int)std::min<size_t>(len_of(bh), (size_t)S);
    for (int j = 0; j < n; ++j) seq_out[(size_t)i * S + j] = TOK_PAD;
    int node = bh.node;
    for (int j = have - 1; j >= 0; --j, node = trie[(size_t)node].parent)
      if (j < n) seq_out[(size_t)i * S + j] = trie[(size_t)node].tok;
    len_out[i] = n;
    score_out[i] = bh.score;
  }
  return D2T_OK;
}

}  // extern "C"
