// libd2t engine, TFM head: the decode step, captured step loops, greedy decodes (plain, grouped, ragged) and the ticket /
// wait / query entries of the C-ABI.  The beam searches are engine_tfm_beam.hip's; what the two share is engine_tfm.h's.
// Host code only: the kernels are decode.hip's, decode_gemm.hip's and decode_row.hip's.
#include "engine_tfm.h"

// (LinOpts is filled with designated initializers: C++20, which hipcc's clang takes in C++17 too)
#pragma clang diagnostic ignored "-Wc++20-designator"

namespace tfm {

int tfm_check(d2t_ctx* c, bool have_args, int T, const char* not_tfm) {
  if (!c || !have_args) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  if (c->cfg.decoder != D2T_DEC_TFM) return fail(c, D2T_ESTATE, "%s", not_tfm);
  if (T > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d > %d unsupported", T, memory_cap(c));
  return D2T_OK;
}

hipError_t sync_chains(d2t_ctx* c) {
  hipError_t e = hipSuccess;
  for (int i = 0; i < d2t_ctx::MAXC && e == hipSuccess; ++i)
    if (c->chains[i].stream) e = hipStreamSynchronize(c->chains[i].stream);
  return e;
}

// the step workspace: eight [B][d] row buffers | qkv [B][3d] | f [B][ff]; returns its bytes
static size_t dec_bufs_carve(Carver cv, int B, int d, int ff, DecBufs* b) {
  float** rows[] = {&b->x, &b->y1, &b->x1, &b->y2, &b->x2, &b->y3, &b->q2, &b->a};
  for (float** q : rows) *q = cv.take<float>((size_t)B * d);
  b->qkv = cv.take<float>((size_t)B * 3 * d);
  b->f = cv.take<float>((size_t)B * ff);
  return cv.total();
}

int dec_prepare(d2t_ctx* c, d2t_ctx::Chain& ch, int B, int T, DecBufs* bufs, size_t mem_rows) {
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
  if ((rc = ensure(c, &ch.dws, &ch.dws_cap, dec_bufs_carve(Carver(), B, d, g.dec_ff, bufs)))) return rc;
  if ((rc = ensure(c, &ch.dstate, &ch.dstate_cap, (size_t)(4 + B + GRP_WORDS) * 4))) return rc;
  // beam search, absorbed form: absorbed queries / context rows [B][8][d] and LN1 outputs [B][d] between the row kernel's halves
  if (c->dec_absorbed && (rc = ensure(c, &c->beam_qp, &c->beam_qp_cap, (size_t)B * 9 * d * 4))) return rc;
  dec_bufs_carve(Carver(ch.dws), B, d, g.dec_ff, bufs);
  return D2T_OK;
}

unsigned long long* trace_slot(d2t_ctx* c) {
  if (!c->dtrace || c->dtrace_next >= d2t_ctx::DTRACE_SLOTS) return nullptr;
  return c->dtrace + 2 * (size_t)(c->dtrace_next++);
}

// Where a slot keeps the bf16 planes of its memory rows: hi `plane` floats behind the slot's start, lo `plane` elements behind
// hi (stage_memory writes them there, the absorbed row kernels read them).
struct Planes { uint16_t *hi, *lo; };
static Planes slot_planes(float* ckv, size_t plane) {
  uint16_t* hi = reinterpret_cast<uint16_t*>(ckv + plane);
  return {hi, hi + plane};
}

hipError_t stage_memory(float* ckv, size_t plane, const float* memory, size_t n, hipStream_t s) {
  hipError_t e = hipMemcpyAsync(ckv, memory, n * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;
  const Planes pl = slot_planes(ckv, plane);
  return launch_split_bf16(memory, pl.hi, pl.lo, n, s);  // the planes of the split-bf16 cross-attention (decode_row.hip)
}

hipError_t cross_kv(d2t_ctx* c, hipStream_t s, const float* memory, int B, int T, float* ckv) {
  const d2t_config& g = c->cfg;
  const int d = g.dec_dim;
  // absorbed form: no projection at all -- the step loop reads the memory rows; the slot keeps a copy so that the captured
  // loop holds an engine address and the caller's tensor is free again as soon as this copy has run
  if (c->dec_absorbed) return stage_memory(ckv, (size_t)B * T * d, memory, (size_t)B * T * d, s);
  return cross_kv_projected(c, s, memory, B, T, ckv);
}

hipError_t cross_kv_projected(d2t_ctx* c, hipStream_t s, const float* memory, int B, int T, float* ckv, bool exact) {
  const d2t_config& g = c->cfg;
  const int d = g.dec_dim;
  ConvP p{};
  p.in = memory; p.w = c->ckv_w; p.bias = c->ckv_b; p.out = ckv;
  if (!exact && c->conv_bf16x3 && c->ckv_hi) { p.w_hi = c->ckv_hi; p.w_lo = c->ckv_lo; }
  linear_shape(p, B * T, d, g.dec_layers * 2 * d);
  p.store_mode = STORE_KV; p.kv_T = T; p.kv_heads = g.dec_heads; p.kv_hd = d / g.dec_heads; p.kv_B = B;
  return launch_conv(p, s);
}

namespace {
// What every GEMM launch of one step shares, and what a launch may differ in (named, the rest defaults).
struct StepLaunch { d2t_ctx* c; hipStream_t s; int M; const int *stop, *step; };
struct LinOpts {
  const float* res = nullptr;  // residual rows added in the epilogue
  int act = ACT_NONE;
  const LNW* ln = nullptr;     // LayerNorm of the input rows as the GEMM's prologue ...
  float* ln_out = nullptr;     // ... which also writes the normalised rows here (the residual of a later launch)
  bool out_by_step = false;    // the output advances by out_step_stride per decode step (the logits of a greedy loop)
  long long out_step_stride = 0;
};
// y[M][w.N] (row stride ldy) = act(LN?(x)[M][w.K] (row stride ldx) . w + b) + res
hipError_t lin(const StepLaunch& L, const float* x, int ldx, const LinW& w, float* y, int ldy, const LinOpts& o = {}) {
  SkinnyP p{};
  p.trace = trace_slot(L.c);
  p.stop_at = L.stop; p.cur_step = L.step;
  p.x = x; p.w = w.w; p.bias = w.b; p.res = o.res; p.y = y;
  p.M = L.M; p.K = w.K; p.N = w.N; p.ldx = ldx; p.ldy = ldy; p.ldres = w.N; p.act = o.act;
  p.step_ptr = o.out_by_step ? L.step : nullptr; p.out_step_stride = o.out_step_stride;
  if (o.ln) { p.ln_g = o.ln->g; p.ln_b = o.ln->b; p.ln_eps = 1e-5f; p.ln_out = o.ln_out; }
  return launch_skinny(p, L.s);
}
}  // namespace

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
  const StepLaunch sl{c, s, M, stop, step};
  // absorbed form: the planes lie behind the slot's capacity-fixed offset (ragged) or right behind the fp32 rows (cross_kv)
  const Planes pl = slot_planes(a.ckv, rg ? rg->plane_elems : (size_t)(ckvB > 0 ? ckvB : kvB) * T * d);
  const uint16_t *mhi = c->cross_fp32 ? nullptr : pl.hi, *mlo = c->cross_fp32 ? nullptr : pl.lo;
  hipError_t e;
#define TRY(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)
  const size_t skv_layer = (size_t)kvB * heads * Lmax * hd;
  // batched beam search: ckvB samples' cross K/V, row b attends over sample row_map[b]
  const size_t ckv_slab = (size_t)(ckvB > 0 ? ckvB : kvB) * heads * T * hd;
  for (int l = 0; l < g.dec_layers; ++l) {
    const DecLayer& L = c->dec[l];
    if (l == 0) TRY(lin(sl, bf.x, d, L.sa_in, bf.qkv, 3 * d));
    else TRY(lin(sl, bf.y3, d, L.sa_in, bf.qkv, 3 * d, {.ln = &c->dec[l - 1].n3, .ln_out = bf.x}));
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
    if (a.maps.maps) {  // the replay: a.ckv holds projected K / V whatever the context decodes with
      TRY(launch_decoder_row_maps(r, bf.q2, s));
      if (a.maps.layer_mask >> l & 1u) {
        const int k = __builtin_popcount(a.maps.layer_mask & ((1u << l) - 1u));
        CrossProbsP cp{};
        cp.q = bf.q2; cp.q_stride = d; cp.ck = r.ck; cp.c_batch_stride = r.c_batch_stride; cp.M = M; cp.D = d; cp.T = T;
        cp.out = a.maps.maps + (size_t)k * a.maps.layer_stride; cp.out_row_stride = a.maps.row_stride;
        cp.out_head_stride = a.maps.head_stride; cp.step_ptr = step;
        TRY(launch_cross_attn_probs(cp, s));
      }
    } else if (c->dec_absorbed && c->beam_shared_tile && beam > 0 && beam <= 6 && c->beam_qp && row_map)
      TRY(launch_decoder_row_beam(r, a.ckv, (long long)T * d, L.ca_wk, L.ca_v_t, L.ca_bv, c->beam_qp,
                                  c->beam_qp + (size_t)kvB * 8 * d, a.seg, ckvB, s));
    else if (c->dec_absorbed && rg)
      TRY(launch_decoder_row_absorbed(r, a.ckv, 0, L.ca_wk, L.ca_v_t, L.ca_bv, s, mhi, mlo, rg->row0, rg->len));
    else if (c->dec_absorbed)  // greedy rows (two per block) and beam rows (one per block, ancestry) alike
      TRY(launch_decoder_row_absorbed(r, a.ckv, (long long)T * d, L.ca_wk, L.ca_v_t, L.ca_bv, s, mhi, mlo));
    else TRY(launch_decoder_row(r, s));
    TRY(lin(sl, bf.y2, d, L.l1, bf.f, g.dec_ff, {.act = ACT_RELU, .ln = &L.n2, .ln_out = bf.x2}));
    TRY(lin(sl, bf.f, g.dec_ff, L.l2, bf.y3, d, {.res = bf.x2}));
  }
  if (a.logits)
    TRY(lin(sl, bf.y3, d, c->out_proj, a.logits, (int)a.logit_row_stride,
            {.ln = &c->dec[g.dec_layers - 1].n3, .out_by_step = true, .out_step_stride = a.logit_step_stride}));
#undef TRY
  return hipSuccess;
}

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

void graph_key(d2t_ctx::GraphKey* k, const d2t_ctx::Chain& ch, const float* ckv, int B, int T, int steps) {
  memset(k, 0, sizeof *k);
  k->B = B; k->T = T; k->steps = steps; k->ckv = ckv; k->dws = ch.dws; k->skv = ch.skv; k->dstate = ch.dstate;
}

}  // namespace tfm

using namespace tfm;

namespace {

// Greedy decode.  The cross-attention K/V projection runs on the caller's stream into one of two slots;
// the step loop runs on the internal stream, ordered after it.  What a call asks for is a GreedyCall:
// async: return right after enqueueing (always max_seq_len+1 steps); the caller orders later work with d2t_decode_wait.
// rows_per_batch > 0 (async only): the B rows are rows_per_batch-row encoder batches decoded by one loop (a decode group);
// with is_test every batch gets its own "first step at which all ITS rows had ended", and the captured loop stops working
// once every batch has one (device-side early exit: the remaining kernels of the graph return at their first instruction).
// rg != nullptr (async only, absorbed form): a RAGGED group -- the B rows are rg->n batches of rg->rows[i] rows whose memories of
// rg->T[i] tokens lie packed in `memory` ([sum rows_i T_i][d]); T and rows_per_batch are unused.  Lengths, offsets and the
// batch layout reach the kernels through per-slot device tables, so the captured loop depends on the row total alone.
struct RaggedGroup { int n; const int32_t* rows; const int32_t* T; size_t mem_rows; };
// One greedy call as its entry point describes it: zero-initialised, set by field name.
struct GreedyCall {
  bool async = false;
  int is_test = 0;
  int rows_per_batch = 0;
  const RaggedGroup* rg = nullptr;
  int64_t* tokens = nullptr;  // the caller's outputs [B][S], [B][S][V]
  float* logits = nullptr;
  int* steps_out = nullptr;   // synchronous: the steps run
};

struct RaggedTab { int *row0, *len, *row_batch, *batch_rows, *n_batches; };
// a slot's tables (device copy or pinned host copy): row0 | len | row_batch [cap] | batch_rows [GRP_MAXB] | n_batches
RaggedTab ragged_tab(int* base, int cap) {
  Carver cv(base);
  RaggedTab t;
  t.row0 = cv.take<int>(cap); t.len = cv.take<int>(cap); t.row_batch = cv.take<int>(cap);
  t.batch_rows = cv.take<int>(GRP_MAXB); t.n_batches = cv.take<int>(1);
  return t;
}
// Fill slot `slot`'s tables for the group (host side, then one asynchronous copy on the caller's stream, which the decode
// stream is ordered behind).  The caller's stream already waits for the decode that last read this slot.
int ragged_tables(d2t_ctx* c, int slot, int B, const RaggedGroup& rg, hipStream_t user) {
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
  const RaggedTab t = ragged_tab(h, cap);
  int *row0 = t.row0, *len = t.len, *row_batch = t.row_batch, *batch_rows = t.batch_rows;
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
  *t.n_batches = rg.n;
  HIPCHK(c, hipMemcpyAsync(c->rg_tab[slot], h, ((size_t)3 * cap + GRP_MAXB + 1) * 4, hipMemcpyHostToDevice, user));
  if (!c->rg_ev[slot]) HIPCHK(c, hipEventCreateWithFlags(&c->rg_ev[slot], hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->rg_ev[slot], user));
  c->rg_ev_valid[slot] = true;
  return D2T_OK;
}

// What the phases of one greedy decode share: the call as planned (greedy_plan) and its buffers (greedy_buffers).
struct Greedy {
  int B = 0, T = 0, S = 0, V = 0;
  int rows_per_batch = 0, n_batches = 0;
  bool dev_exit = false;    // early exit decided on the device inside the whole-loop graph
  bool use_graph = true;
  // With early exit the host polls between steps, so one captured graph = one step, replayed.  Without it (async, or
  // is_test == 0) the whole max_seq_len+1 step loop is ONE graph: a single launch per batch keeps the host free to enqueue
  // the next batch's encoder while this one decodes.
  int steps_per_graph = 0;
  int slot = 0;
  d2t_ctx::Chain* ch = nullptr;
  hipStream_t s = nullptr;  // the chain's stream
  DecBufs bf = {};
  float* ckv = nullptr;     // the memory slot
  float* logits = nullptr;  // where the loop writes: the chain's staging, or the caller's outputs
  int64_t* tokens = nullptr;
  size_t log_bytes = 0, tok_bytes = 0;
  int *dstate = nullptr, *grp = nullptr;  // the chain's state block and the decode-group words in it
  int* stop = nullptr;                    // dev_exit: the stop-at step
};

// Slot and chain.  Memory slots rotate (at least two: the next batch's copy is written while the previous decode still reads
// its own); async decodes rotate over the chains (chain == slot); everything else runs on chain 0.
int greedy_plan(d2t_ctx* c, const GreedyCall& call, int B, int T, Greedy* p) {
  const d2t_config& g = c->cfg;
  p->B = B; p->T = T; p->S = g.max_seq_len + 1; p->V = g.vocab;
  p->rows_per_batch = (call.rows_per_batch <= 0 || B % call.rows_per_batch) ? B : call.rows_per_batch;
  p->n_batches = call.rg ? call.rg->n : B / p->rows_per_batch;
  if (p->n_batches > GRP_MAXB) return fail(c, D2T_EINVAL, "a decode group holds at most %d batches", GRP_MAXB);  // (nothing enqueued yet)
  p->dev_exit = call.async && call.is_test;
  p->steps_per_graph = (!call.is_test || p->dev_exit) ? p->S : 1;
  p->use_graph = D2T_PROBE_ENV_STR("D2T_NO_GRAPH") == nullptr;
  const int nslots = c->n_chains > 2 ? c->n_chains : 2;
  p->slot = (int)(c->decode_seq++ % (unsigned)nslots);
  p->ch = &c->chains[(call.async && c->n_chains > 1) ? p->slot % c->n_chains : 0];
  p->s = p->ch->stream;
  return D2T_OK;
}

// the chain's output staging: logits [rows][S][V] | tokens [rows][S]; returns its bytes
size_t out_carve(Carver cv, size_t rows_S, int V, float** logits, int64_t** tokens) {
  *logits = cv.take<float>(rows_S * V);
  *tokens = cv.take<int64_t>(rows_S, 4);
  return cv.total();
}

// Buffers at their size; the outputs redirected to the chain's staging.
int greedy_buffers(d2t_ctx* c, const GreedyCall& call, Greedy* p) {
  d2t_ctx::Chain& ch = *p->ch;
  const size_t rows_S = (size_t)p->B * p->S;
  int rc = dec_prepare(c, ch, p->B, p->T, &p->bf, call.rg ? call.rg->mem_rows : 0);
  if (rc) return rc;
  p->ckv = c->ckv2[p->slot];
  p->logits = call.logits; p->tokens = call.tokens;
  p->log_bytes = rows_S * p->V * sizeof(float); p->tok_bytes = rows_S * sizeof(int64_t);
  if (p->use_graph) {  // engine-owned staging [logits | tokens] on both paths: the graph key holds engine addresses only, so a
                       // caller that allocates fresh output tensors per call (Model.forward does) never forces a re-capture
    if ((rc = ensure(c, &ch.out, &ch.out_cap, out_carve(Carver(), rows_S, p->V, &p->logits, &p->tokens)))) return rc;
    out_carve(Carver(ch.out), rows_S, p->V, &p->logits, &p->tokens);
  }
  p->dstate = ch.dstate;
  p->grp = ch.dstate + 4 + p->B;
  p->stop = p->dev_exit ? p->grp + 2 * GRP_MAXB + 1 : nullptr;
  return D2T_OK;
}

// The memory into the slot, on the caller's stream: the cross K/V (absorbed form: the rows and their planes) of a uniform
// decode, or a ragged group's tables first, then its packed rows and their bf16 planes at the slot's capacity-fixed offsets.
// *rgd: the ragged view the step reads (row0 == nullptr: uniform).
int greedy_stage(d2t_ctx* c, const GreedyCall& call, const Greedy& p, const float* memory, hipStream_t user, RaggedDev* rgd) {
  *rgd = {};
  // the decode that last read this K/V slot must be finished before it is overwritten
  if (c->ev_done_valid[p.slot]) HIPCHK(c, hipStreamWaitEvent(user, c->ev_done[p.slot], 0));
  if (!call.rg) {
    HIPCHK(c, cross_kv(c, user, memory, p.B, p.T, p.ckv));
    return D2T_OK;
  }
  if (int rc = ragged_tables(c, p.slot, p.B, *call.rg, user)) return rc;
  const RaggedTab tab = ragged_tab(c->rg_tab[p.slot], c->rg_cap);
  rgd->row0 = tab.row0; rgd->len = tab.len;
  rgd->plane_elems = plane_elems(c, p.slot);
  HIPCHK(c, stage_memory(p.ckv, rgd->plane_elems, memory, call.rg->mem_rows * c->cfg.dec_dim, user));
  return D2T_OK;
}

// The argmax + next-embedding launch of every step, for the uniform, grouped or ragged layout.
ArgmaxP greedy_argmax(const d2t_ctx* c, const Greedy& p, bool ragged) {
  int* const dstate = p.dstate;
  ArgmaxP am{};
  am.logits = p.logits; am.row_stride = (long long)p.S * p.V; am.step_stride = p.V;
  am.tokens = p.tokens; am.tok_stride = p.S;
  am.ended = dstate + 4; am.end_count = dstate + 1; am.steps_done = dstate + 2; am.step_ptr = dstate;
  am.B = p.B; am.V = p.V; am.end_token = TOK_END;
  am.emb = c->word_embed; am.pe = c->word_pe; am.x = p.bf.x; am.d = c->cfg.dec_dim;
  am.done_count = dstate + 3;
  am.batch_end_count = p.grp; am.batch_steps_done = p.grp + GRP_MAXB; am.batches_done = p.grp + 2 * GRP_MAXB;
  am.stop_at = p.stop;
  if (ragged) {  // the layout is read from the slot's tables at run time; nothing of it is baked into the captured launch
    // ArgmaxP::n_batches > 0 only says "grouped" here (ARGMAX_GROUPED): the group's real batch count is *n_batches_ptr
    const RaggedTab tab = ragged_tab(c->rg_tab[p.slot], c->rg_cap);
    am.rows_per_batch = 0; am.n_batches = ARGMAX_GROUPED;
    am.row_batch = tab.row_batch; am.batch_rows = tab.batch_rows; am.n_batches_ptr = tab.n_batches;
  } else {
    am.rows_per_batch = p.rows_per_batch; am.n_batches = p.n_batches;
  }
  return am;
}

StepArgs greedy_step_args(const Greedy& p, const RaggedDev& rgd) {
  StepArgs sa;
  sa.rows = p.B; sa.T = rgd.row0 ? 1 : p.T; sa.kvB = p.B;
  sa.logits = p.logits; sa.logit_row_stride = (long long)p.S * p.V; sa.logit_step_stride = p.V;
  sa.stop = p.stop; sa.rg = rgd; sa.ckv = p.ckv; sa.skv = p.ch->skv; sa.step = p.dstate;
  return sa;
}

// The key of the decode's captured loop.  Uniform: rows, memory length, dev_exit, rows_per_batch.  Ragged: the row total and
// the tables -- neither T nor the batch layout.
d2t_ctx::GraphKey greedy_key(const d2t_ctx* c, const Greedy& p, const RaggedDev& rgd) {
  d2t_ctx::GraphKey k;
  graph_key(&k, *p.ch, p.ckv, p.B, rgd.row0 ? 0 : p.T, p.steps_per_graph);
  k.loop = p.steps_per_graph == p.S ? d2t_ctx::LOOP_GREEDY_WHOLE : d2t_ctx::LOOP_GREEDY_STEP;
  k.tok = p.tokens; k.logits = p.logits;
  k.dev_exit = p.dev_exit;
  if (rgd.row0) { k.ragged = 1; k.rg_cap = c->rg_cap; k.rtab = rgd.row0; k.plane_elems = (long long)rgd.plane_elems; }
  else k.rows_per_batch = p.rows_per_batch;
  return k;
}

// one step: the decoder layers up to the logits, then argmax and the next step's embedded input
struct GreedyLoop { d2t_ctx* c; const Greedy* p; const StepArgs* sa; ArgmaxP* am; };
hipError_t greedy_step(const GreedyLoop& lp, hipStream_t st) {
  hipError_t e = decode_step(lp.c, st, lp.p->bf, *lp.sa);
  if (e != hipSuccess) return e;
  lp.am->trace = trace_slot(lp.c);
  return launch_argmax_embed(*lp.am, st);
}

// The step loop: the captured graph (steps_per_graph steps per launch) or plain launches; a synchronous is_test decode polls
// "all rows ended" every 8 steps and leaves the loop there.  *steps: the steps run.
int greedy_run(d2t_ctx* c, const GreedyCall& call, const GreedyLoop& lp, const d2t_ctx::GraphKey& key, int* steps) {
  const Greedy& p = *lp.p;
  hipStream_t s = p.s;
  hipGraphExec_t exec = nullptr;
  if (p.use_graph) {
    if (D2T_PROBE_ENV_STR("D2T_DECODE_TRACE") && !c->dtrace)  // debug timeline of the kernel nodes of a captured loop
      HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->dtrace), (size_t)d2t_ctx::DTRACE_SLOTS * 16));
    int rc = cached_graph(c, s, key, "decode", [&lp](hipStream_t st) {
      hipError_t e = hipSuccess;
      for (int t = 0; t < lp.p->steps_per_graph && e == hipSuccess; ++t) e = greedy_step(lp, st);
      return e;
    }, &exec);
    if (rc) return rc;
  }
  // device-side early exit: the loop stops writing at the group's stop step, so define everything past it (PAD ids, zero
  // logits) instead of handing the caller whatever an earlier decode left in the staging buffer
  if (p.dev_exit) {
    HIPCHK(c, hipMemsetAsync(p.logits, 0, p.log_bytes, s));
    HIPCHK(c, hipMemsetAsync(p.tokens, 0, p.tok_bytes, s));
  }
  d2t_ctx::ProfRec drec{-1, p.B, p.S, nullptr, nullptr};  // profiling: the decode loop as ONE record (M = -1, N = rows, K = steps)
  if (c->profiling && hipEventCreate(&drec.a) == hipSuccess && hipEventCreate(&drec.b) == hipSuccess) HIPCHK(c, hipEventRecord(drec.a, s));
  *steps = p.S;
  for (int t = 0; t < p.S; t += (p.use_graph ? p.steps_per_graph : 1)) {
    if (p.use_graph) HIPCHK(c, hipGraphLaunch(exec, s));
    else HIPCHK(c, greedy_step(lp, s));
    if (!call.async && call.is_test && ((t & 7) == 7 || t == p.S - 1)) {
      HIPCHK(c, hipMemcpyAsync(c->h_pinned, p.dstate + 2, 4, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipStreamSynchronize(s));
      if (c->h_pinned[0] > 0) { *steps = c->h_pinned[0]; break; }
    }
  }
  if (drec.b) {
    HIPCHK(c, hipEventRecord(drec.b, s));
    c->prof.push_back(drec);
  }
  return D2T_OK;
}

// Behind the loop, on the chain's stream: a ragged early-exit group's per-batch tails, the copy out of the staging, the
// slot's "decode done" event, and the ticket (async) or the wait for it all.
int greedy_finish(d2t_ctx* c, const GreedyCall& call, const Greedy& p) {
  hipStream_t s = p.s;
  // a ragged group's batches are consumed one by one: each gets PAD / zeros from ITS OWN exit step on, as its single-batch
  // decode leaves them (the loop itself ran every row until the last batch had ended)
  if (call.rg && p.dev_exit)
    HIPCHK(c, launch_ragged_finalize(p.tokens, p.logits, ragged_tab(c->rg_tab[p.slot], c->rg_cap).row_batch, p.grp + GRP_MAXB, p.B, p.S, p.V, s));
  if (p.tokens != call.tokens) {
    HIPCHK(c, hipMemcpyAsync(call.logits, p.logits, p.log_bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(call.tokens, p.tokens, p.tok_bytes, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(c, hipEventRecord(c->ev_done[p.slot], s));
  c->ev_done_valid[p.slot] = true;
  if (call.async) return issue_ticket(c, s, p.dev_exit ? p.n_batches : -p.S, p.grp + GRP_MAXB);
  HIPCHK(c, hipStreamSynchronize(s));
  return D2T_OK;
}

// The decode, in the order everything is enqueued.
int greedy_impl(d2t_ctx* c, const float* memory, int B, int T, const int64_t* start_tokens, hipStream_t user, const GreedyCall& call) {
  Greedy p;
  RaggedDev rgd;
  int rc, steps;
  if ((rc = greedy_plan(c, call, B, T, &p))) return rc;
  if ((rc = greedy_buffers(c, call, &p))) return rc;
  // the caller's stream: behind the slot's last reader, then (ragged) the tables, then the memory
  if ((rc = greedy_stage(c, call, p, memory, user, &rgd))) return rc;
  // the chain's stream, ordered after the caller's work (K/V slot, start tokens, a ragged group's tables)
  HIPCHK(c, hipEventRecord(c->ev_in, user));
  HIPCHK(c, hipStreamWaitEvent(p.s, c->ev_in, 0));
  HIPCHK(c, hipMemsetAsync(p.dstate, 0, (size_t)(4 + B + GRP_WORDS) * 4, p.s));
  // step 0 input: Embedding([GO]) * sqrt(d) + pe[0]; later inputs are written by argmax_embed
  HIPCHK(c, launch_embed(c->word_embed, c->word_pe, start_tokens, p.tokens, p.S, p.dstate, p.bf.x, B, c->cfg.dec_dim, p.s));
  ArgmaxP am = greedy_argmax(c, p, rgd.row0 != nullptr);
  const StepArgs sa = greedy_step_args(p, rgd);
  // (capture on a miss) | dev_exit: outputs zeroed | the steps, polled when synchronous with is_test
  if ((rc = greedy_run(c, call, GreedyLoop{c, &p, &sa, &am}, greedy_key(c, p, rgd), &steps))) return rc;
  // (ragged dev_exit: per-batch tails) | copy-out | ev_done | ticket or synchronise
  if ((rc = greedy_finish(c, call, p))) return rc;
  if (call.steps_out) *call.steps_out = steps;
  return D2T_OK;
}

// The replay's workspace (d2t_ctx::maps_ws): the step workspace | self-attention cache | projected cross K / V of every layer |
// the fed tokens by step [S][B] | its step counter; returns its bytes
struct MapsWs { DecBufs bf; float *skv, *ckv; int64_t* tok; int* step; };
size_t maps_ws_carve(void* base, const d2t_config& g, int B, int T, int S, MapsWs* w) {
  const int d = g.dec_dim, Lmax = g.max_seq_len + 2;
  Carver cv(base);
  cv.at = dec_bufs_carve(Carver(base), B, d, g.dec_ff, &w->bf);
  w->skv = cv.take<float>((size_t)g.dec_layers * 2 * B * Lmax * d, 256);
  w->ckv = cv.take<float>((size_t)g.dec_layers * 2 * B * T * d, 256);
  w->tok = cv.take<int64_t>((size_t)S * B, 256);
  w->step = cv.take<int>(4, 256);
  return cv.total();
}

// Teacher-forced replay of the step loop: step t is fed tokens_in[b][t] and writes the cross-attention probabilities of its
// query as row t of the maps.  Everything runs on the caller's stream in the replay's own buffers, with plain launches: no
// chain, memory slot or captured loop of the context is touched.  Always the projected-K/V row work (decode_step, a.maps).
int cross_attention_impl(d2t_ctx* c, const float* memory, int B, int T, const int64_t* tokens_in, int S, uint32_t layer_mask,
                         int per_head, float* maps, hipStream_t user) {
  const d2t_config& g = c->cfg;
  const int d = g.dec_dim, nl = __builtin_popcount(layer_mask), H = g.dec_heads;
  const size_t n_tok = (size_t)B * S;
  int rc;
  // the fed tokens index the embedding table: read them back, refuse ids outside the vocabulary, lay them out by step
  if ((rc = ensure_host_beam(c, 2 * n_tok * sizeof(int64_t)))) return rc;
  int64_t *h_in = reinterpret_cast<int64_t*>(c->h_beam), *h_by_step = h_in + n_tok;
  HIPCHK(c, hipMemcpyAsync(h_in, tokens_in, n_tok * sizeof(int64_t), hipMemcpyDeviceToHost, user));
  HIPCHK(c, hipStreamSynchronize(user));
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < S; ++t) {
      const int64_t tok = h_in[(size_t)b * S + t];
      if (tok < 0 || tok >= g.vocab) return fail(c, D2T_EINVAL, "tokens_in[%d][%d] = %lld is outside the vocabulary of %d", b, t, (long long)tok, g.vocab);
      h_by_step[(size_t)t * B + b] = tok;
    }
  MapsWs w;
  if ((rc = ensure(c, &c->maps_ws, &c->maps_ws_cap, maps_ws_carve(nullptr, g, B, T, S, &w)))) return rc;
  maps_ws_carve(c->maps_ws, g, B, T, S, &w);
  HIPCHK(c, hipMemcpyAsync(w.tok, h_by_step, n_tok * sizeof(int64_t), hipMemcpyHostToDevice, user));
  HIPCHK(c, cross_kv_projected(c, user, memory, B, T, w.ckv, true));  // fp32 whatever the context's convolution arithmetic
  StepArgs sa;
  sa.rows = B; sa.T = T; sa.kvB = B; sa.ckv = w.ckv; sa.skv = w.skv; sa.step = w.step;
  sa.maps.maps = maps; sa.maps.layer_mask = layer_mask;
  sa.maps.head_stride = per_head ? (long long)S * T : 0;
  sa.maps.layer_stride = (long long)(per_head ? H : 1) * S * T;
  sa.maps.row_stride = sa.maps.layer_stride * nl;
  for (int t = 0; t < S; ++t) {
    HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.step), t, 1, user));
    HIPCHK(c, launch_embed_tokens(c->word_embed, c->word_pe, w.tok + (size_t)t * B, w.step, w.bf.x, B, d, user));
    HIPCHK(c, decode_step(c, user, w.bf, sa));
  }
  HIPCHK(c, hipStreamSynchronize(user));  // the pinned staging and the workspace are idle again; the maps are complete
  return D2T_OK;
}
}  // namespace

extern "C" {

static const char NOT_TFM[] = "context was not created with the TFM decoder";

int d2t_decode_greedy(d2t_ctx* c, const float* memory, int32_t B, int32_t T, const int64_t* start_tokens,
                      int32_t is_test, int64_t* tokens, float* logits, int32_t* steps_out, d2t_stream stream) {
  DevGuard dg_(c);
  if (int rc = tfm_check(c, memory && start_tokens && tokens && logits && steps_out && B >= 1 && T >= 1, T, NOT_TFM)) return rc;
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, logits, "logits")) return rc;
  GreedyCall call;
  call.is_test = is_test; call.tokens = tokens; call.logits = logits; call.steps_out = steps_out;
  return greedy_impl(c, memory, B, T, start_tokens, (hipStream_t)stream, call);
}

int d2t_decode_greedy_async(d2t_ctx* c, const float* memory, int32_t B, int32_t T, const int64_t* start_tokens,
                            int64_t* tokens, float* logits, d2t_stream stream) {
  DevGuard dg_(c);
  if (int rc = tfm_check(c, memory && start_tokens && tokens && logits && B >= 1 && T >= 1, T, NOT_TFM)) return rc;
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, logits, "logits")) return rc;
  GreedyCall call;
  call.async = true; call.tokens = tokens; call.logits = logits;
  return greedy_impl(c, memory, B, T, start_tokens, (hipStream_t)stream, call);
}

int d2t_decode_greedy_submit(d2t_ctx* c, const float* memory, int32_t B, int32_t T, const int64_t* start_tokens,
                             int32_t is_test, int32_t rows_per_batch, int64_t* tokens, float* logits, d2t_stream stream,
                             int64_t* ticket_out) {
  DevGuard dg_(c);
  if (int rc = tfm_check(c, memory && start_tokens && tokens && logits && B >= 1 && T >= 1, T, NOT_TFM)) return rc;
  if (rows_per_batch < 0 || (rows_per_batch > 0 && B % rows_per_batch)) return fail(c, D2T_EINVAL, "rows_per_batch must divide the row count");
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, logits, "logits")) return rc;
  GreedyCall call;
  call.async = true; call.is_test = is_test; call.rows_per_batch = rows_per_batch; call.tokens = tokens; call.logits = logits;
  const int rc = greedy_impl(c, memory, B, T, start_tokens, (hipStream_t)stream, call);
  if (rc == D2T_OK && ticket_out) *ticket_out = c->last_ticket;
  return rc;
}

int d2t_decode_greedy_submit_ragged(d2t_ctx* c, const float* memory, int32_t n_batches, const int32_t* batch_rows,
                                    const int32_t* batch_T, const int64_t* start_tokens, int32_t is_test, int64_t* tokens,
                                    float* logits, d2t_stream stream, int64_t* ticket_out) {
  DevGuard dg_(c);
  if (int rc = tfm_check(c, memory && batch_rows && batch_T && start_tokens && tokens && logits, 0, NOT_TFM)) return rc;
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
  GreedyCall call;
  call.async = true; call.is_test = is_test; call.rg = &rg; call.tokens = tokens; call.logits = logits;
  const int rc = greedy_impl(c, memory, (int)B, 0, start_tokens, (hipStream_t)stream, call);
  if (rc == D2T_OK && ticket_out) *ticket_out = c->last_ticket;
  return rc;
}

int d2t_decode_cross_attention(d2t_ctx* c, const float* memory, int32_t B, int32_t T, const int64_t* tokens_in, int32_t S,
                               uint32_t layer_mask, int32_t per_head, float* maps, d2t_stream stream) {
  DevGuard dg_(c);
  if (int rc = tfm_check(c, memory && tokens_in && maps && B >= 1 && T >= 1, T, NOT_TFM)) return rc;
  const d2t_config& g = c->cfg;
  if (g.dec_heads != 8) return fail(c, D2T_ESTATE, "cross-attention maps need the 8-head decoder (this one has %d heads)", g.dec_heads);
  if (S < 1 || S > g.max_seq_len + 1) return fail(c, D2T_EINVAL, "%d replay steps: 1 .. max_seq_len + 1 = %d", S, g.max_seq_len + 1);
  if (B > 65535) return fail(c, D2T_EINVAL, "%d rows: at most 65535 per call", B);
  if (!layer_mask || (g.dec_layers < 32 && (layer_mask >> g.dec_layers)))
    return fail(c, D2T_EINVAL, "layer_mask 0x%x: at least one layer, none at or above dec_layers = %d", layer_mask, g.dec_layers);
  const unsigned long long bytes = 4ull * B * __builtin_popcount(layer_mask) * (per_head ? g.dec_heads : 1) * S * T;
  if (bytes > D2T_ATTN_MAP_BUDGET)
    return fail(c, D2T_EINVAL, "cross-attention maps of %llu bytes exceed the %llu-byte budget: split the batch", bytes,
                (unsigned long long)D2T_ATTN_MAP_BUDGET);
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, tokens_in, "tokens_in")) return rc;
  if (int rc = check_dev_ptr(c, maps, "maps")) return rc;
  return cross_attention_impl(c, memory, B, T, tokens_in, S, layer_mask, per_head != 0, maps, (hipStream_t)stream);
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


}  // extern "C"
