// libd2t engine, TFM head: the beam searches of the C-ABI -- the device-side step loop (absorbed d_model-256 decoder) and the
// host-side one (everything else), which keep one bookkeeping record and share one final selection (beam_host.h).  The
// decode step, its buffers and the captured-loop cache are engine_tfm.hip's (engine_tfm.h).  Host code only.
#include "engine_tfm.h"
#pragma GCC visibility push(hidden)  // (its inline functions are not part of the library's surface)
#include "beam_host.h"
#pragma GCC visibility pop

using namespace tfm;

namespace {
constexpr int BEAM_MAX_N = 1024;

// Every sample's best hypothesis out of a record on the host (both loops end here)
void beam_select_all(const BeamRec& r, int64_t* seq_out, int32_t* len_out, float* score_out) {
  for (int i = 0; i < r.N; ++i) beam_select(r, i, TOK_PAD, seq_out + (size_t)i * r.S, &len_out[i], &score_out[i]);
}

// ---- the device-side loop ----
// Its workspace: logits [cap][V] | topv [cap] | topi [cap] | tok [cap] i64 | the result block (beam_result_carve: copied back
// to the host at the end) | map | prev [cap] | anc [2][cap][Lmax], each from a 16-byte boundary; returns its bytes.
struct BeamDevWs {
  float *logits, *topv;
  int* topi;
  BeamRec rec;
  char* res; size_t res_bytes;
  int* anc[2];
};
size_t beam_dev_ws_carve(Carver cv, int Lmax, BeamDevWs* w) {
  BeamRec& r = w->rec;
  w->logits = cv.take<float>((size_t)r.cap * r.V, 16);
  w->topv = cv.take<float>(r.cap, 16);
  w->topi = cv.take<int>(r.cap, 16);
  r.tok = cv.take<int64_t>(r.cap, 16);
  cv.align(16);
  w->res = cv.here();
  beam_result_carve(cv, r);
  w->res_bytes = (size_t)(cv.here() - w->res);
  r.map = cv.take<int>(r.cap, 16);
  r.prev = cv.take<int>(r.cap, 16);
  w->anc[0] = cv.take<int>(2 * (size_t)r.cap * Lmax, 16);
  w->anc[1] = w->anc[0] + (size_t)r.cap * Lmax;
  cv.align(16);
  return cv.total() + 64;
}
// the record as the kernels take it
BeamDev beam_dev(const BeamDevWs& w) {
  const BeamRec& r = w.rec;
  BeamDev b{};
  b.ctrl = r.ctrl; b.tok = r.tok; b.scores = r.scores; b.map = r.map; b.prev = r.prev; b.seg = r.seg;
  b.comp_n = r.comp_n; b.fin = r.fin; b.comp_t = r.comp_t; b.comp_par = r.comp_par; b.comp_score = r.comp_score;
  b.hist_par = r.hist_par; b.hist_tok = r.hist_tok;
  b.topv = w.topv; b.topi = w.topi;
  b.N = r.N; b.beam = r.beam; b.cap = r.cap; b.V = r.V; b.S = r.S; b.end_token = r.end_token;
  return b;
}

// forward_beam (tfm.py:145-186) + Beam (tools/beam.py:38-140) for N samples with the bookkeeping ON THE DEVICE:
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
  BeamDevWs ws{};
  ws.rec.N = N; ws.rec.beam = beam_size; ws.rec.cap = cap; ws.rec.V = V; ws.rec.S = S; ws.rec.end_token = TOK_END;
  if ((rc = ensure(c, &c->beam_ws, &c->beam_ws_cap, beam_dev_ws_carve(Carver(), Lmax, &ws)))) return rc;
  beam_dev_ws_carve(Carver(c->beam_ws), Lmax, &ws);
  const BeamDev b = beam_dev(ws);
  const int* rows_ptr = b.ctrl + 1;
  const int* stop = b.ctrl + 2;
  if ((rc = ensure_host_beam(c, ws.res_bytes))) return rc;
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
  sa.logits = ws.logits; sa.logit_row_stride = V;
  sa.row_map = b.map; sa.stop = stop; sa.beam = beam_size; sa.seg = b.seg; sa.rows_ptr = rows_ptr;
  sa.rg = rgd; sa.ckv = ckv; sa.skv = ch.skv; sa.step = dstate;
  auto enqueue_loop = [&](hipStream_t st) -> hipError_t {
    hipError_t e;
#define LTRY(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)
    LTRY(hipMemsetAsync(dstate, 0, (size_t)(4 + cap) * 4, st));
    LTRY(launch_beam_dev_init(b, TOK_GO, st));
    for (int step = 0; step < S; ++step) {
      LTRY(launch_beam_ancestry(ws.anc[(step + 1) & 1], ws.anc[step & 1], b.prev, cap, Lmax, b.ctrl, dstate, st, rows_ptr, stop));
      LTRY(launch_embed_tokens(c->word_embed, c->word_pe, b.tok, dstate, bf.x, cap, d, st, rows_ptr, stop));
      sa.anc = ws.anc[step & 1];
      LTRY(decode_step(c, st, bf, sa));
      LTRY(launch_beam_topk_batch(ws.logits, b.scores, b.seg, N, V, beam_size, ws.topv, ws.topi, st, dstate, stop));
      LTRY(launch_beam_dev_advance(b, st));
    }
#undef LTRY
    return hipSuccess;
  };
  const bool use_graph = D2T_PROBE_ENV_STR("D2T_NO_GRAPH") == nullptr;
  if (use_graph) {
    d2t_ctx::GraphKey k;
    graph_key(&k, ch, ckv, cap, Ts ? 0 : T, S);  // ragged: N, beam and the tables; no memory length
    k.loop = d2t_ctx::LOOP_BEAM_DEV;
    k.logits = c->beam_ws;
    k.N = N; k.beam = beam_size;
    if (Ts) { k.ragged = 1; k.rtab = c->brg_tab; k.plane_elems = (long long)rgd.plane_elems; }
    hipGraphExec_t exec = nullptr;
    if ((rc = cached_graph(c, s, k, "beam", enqueue_loop, &exec))) return rc;
    HIPCHK(c, hipGraphLaunch(exec, s));
  } else {
    HIPCHK(c, enqueue_loop(s));
  }
  HIPCHK(c, hipMemcpyAsync(c->h_beam, ws.res, ws.res_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  // the host's view of the result block: the same layout from the pinned copy's base
  BeamRec hv = ws.rec;
  Carver hc(c->h_beam);
  beam_result_carve(hc, hv);
  beam_select_all(hv, seq_out, len_out, score_out);
  return D2T_OK;
}

// ---- the host-side loop ----
// Its workspace: logits [cap][V] | topv [cap] | topi [cap] | (16-byte boundary) the step pack (beam_pack_carve) | ancestry
// [2][anc_rows]; returns its bytes.  Its pinned mirror: the step pack | topv [cap] | topi [cap] (one device -> host copy per
// step).  The pack is the same layout function in both, so the two views cannot differ.
struct BeamHostWs {
  float *logits, *topv;
  int* topi;
  BeamRec rec;
  char* pack; size_t pack_bytes;
  int* step;
  int* anc[2];
};
void beam_host_pack(Carver& cv, BeamHostWs* w) {
  cv.align(16);
  w->pack = cv.here();
  w->step = beam_pack_carve(cv, w->rec);
  w->pack_bytes = (size_t)(cv.here() - w->pack);
}
size_t beam_host_ws_carve(Carver cv, size_t anc_rows, BeamHostWs* w) {
  const BeamRec& r = w->rec;
  w->logits = cv.take<float>((size_t)r.cap * r.V);
  w->topv = cv.take<float>(r.cap);
  w->topi = cv.take<int>(r.cap);
  beam_host_pack(cv, w);
  w->anc[0] = cv.take<int>(2 * anc_rows);
  w->anc[1] = w->anc[0] + anc_rows;
  return cv.total() + 64;
}
size_t beam_host_mirror_carve(Carver cv, BeamHostWs* w) {
  beam_host_pack(cv, w);
  w->topv = cv.take<float>(w->rec.cap);
  w->topi = cv.take<int>(w->rec.cap);
  return cv.total();
}

// The same search with one host round trip per step (d_model 512, beam_shared_tile, the D2T_BEAM_HOST probe): per-sample
// log_softmax + top-k on the device, Beam.advance on the host (beam_host_advance) in the record the device-side loop keeps.
// The live rows of the record (tok, scores, map, prev, seg) lie in the pinned step pack and go to the device in one copy.
int beam_host_impl(d2t_ctx* c, const float* memory, int N, int T, int beam_size, int64_t* seq_out, int32_t* len_out,
                   float* score_out, hipStream_t user) {
  const d2t_config& g = c->cfg;
  const int S = g.max_seq_len + 1, V = g.vocab, d = g.dec_dim, cap = N * beam_size;
  const int heads = g.dec_heads, hd = d / heads, Lmax = g.max_seq_len + 2;
  d2t_ctx::Chain& ch = c->chains[0];
  hipStream_t s = ch.stream;
  DecBufs bf;
  int rc = dec_prepare(c, ch, cap, T, &bf);
  if (rc) return rc;
  int* const dstate = ch.dstate;
  // With the absorbed row kernel the self-attention cache is never copied -- every hypothesis keeps an ancestry row (which
  // cache row holds each of its earlier positions, launch_beam_ancestry); otherwise the survivors' caches are gathered into
  // the other buffer.
  const bool use_anc = c->dec_absorbed && !c->beam_shared_tile && Lmax <= 512 && D2T_PROBE_ENV_STR("D2T_BEAM_CACHE_COPY") == nullptr;
  const size_t skv_bytes = (size_t)g.dec_layers * 2 * cap * Lmax * d * 4;
  if (!use_anc && (rc = ensure(c, &c->skv_alt, &c->skv_alt_cap, skv_bytes))) return rc;
  BeamHostWs dv{}, hv{};  // the device view and the host's
  dv.rec.N = N; dv.rec.beam = beam_size; dv.rec.cap = cap; dv.rec.V = V; dv.rec.S = S; dv.rec.end_token = TOK_END;
  hv.rec = dv.rec;
  const size_t anc_rows = use_anc ? (size_t)cap * Lmax : 0;
  if ((rc = ensure(c, &c->beam_ws, &c->beam_ws_cap, beam_host_ws_carve(Carver(), anc_rows, &dv)))) return rc;
  beam_host_ws_carve(Carver(c->beam_ws), anc_rows, &dv);
  if ((rc = ensure_host_beam(c, beam_host_mirror_carve(Carver(), &hv)))) return rc;
  beam_host_mirror_carve(Carver(c->h_beam), &hv);
  // the bookkeeping half of the host's record: pageable, only the host reads it
  BeamRec& r = hv.rec;
  Carver measure;
  beam_book_carve(measure, r);
  std::vector<char> book(measure.total());
  Carver bc(book.data());
  beam_book_carve(bc, r);
  HIPCHK(c, hipEventRecord(c->ev_in, user));
  HIPCHK(c, hipStreamWaitEvent(s, c->ev_in, 0));
  HIPCHK(c, hipMemsetAsync(dstate, 0, (size_t)(4 + cap) * 4, s));
  HIPCHK(c, cross_kv(c, s, memory, N, T, c->ckv2[0]));
  StepArgs sa;
  sa.T = T; sa.kvB = cap; sa.ckvB = N;
  sa.logits = dv.logits; sa.logit_row_stride = V;
  sa.row_map = dv.rec.map; sa.beam = beam_size; sa.seg = dv.rec.seg;
  sa.ckv = c->ckv2[0]; sa.skv = ch.skv; sa.step = dstate;
  float* skv_other = c->skv_alt;
  beam_host_init(r, TOK_GO);
  for (int step = 0; step < S; ++step) {
    const int rows = r.ctrl[1];  // the survivors of the previous step, in the order of their parents in prev
    if (!rows) break;
    *hv.step = step;
    HIPCHK(c, hipMemcpyAsync(dv.pack, hv.pack, hv.pack_bytes, hipMemcpyHostToDevice, s));
    if (use_anc) {
      HIPCHK(c, launch_beam_ancestry(dv.anc[(step + 1) & 1], dv.anc[step & 1], dv.rec.prev, rows, Lmax, dv.step, dstate, s));
    } else {
      HIPCHK(c, launch_beam_ancestry(nullptr, nullptr, dv.rec.prev, 1, 0, dv.step, dstate, s));  // publishes the step only
      if (step > 0) {  // the survivors' caches move to their new row positions
        HIPCHK(c, launch_cache_gather(sa.skv, skv_other, dv.rec.prev, g.dec_layers * 2, cap, rows, heads, Lmax, hd, step, s));
        std::swap(sa.skv, skv_other);
      }
    }
    HIPCHK(c, launch_embed_tokens(c->word_embed, c->word_pe, dv.rec.tok, dstate, bf.x, rows, d, s));
    sa.rows = rows; sa.anc = use_anc ? dv.anc[step & 1] : nullptr;
    HIPCHK(c, decode_step(c, s, bf, sa));
    HIPCHK(c, launch_beam_topk_batch(dv.logits, dv.rec.scores, dv.rec.seg, N, V, beam_size, dv.topv, dv.topi, s));
    HIPCHK(c, hipMemcpyAsync(hv.topv, dv.topv, 2 * (size_t)cap * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    beam_host_advance(r, hv.topv, hv.topi);
  }
  HIPCHK(c, hipStreamSynchronize(s));
  beam_select_all(r, seq_out, len_out, score_out);
  return D2T_OK;
}

const char BEAM_NOT_TFM[] = "beam search is implemented for the TFM decoder only";
}  // namespace

extern "C" {

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
  if (int rc = tfm_check(c, memory && T && seq_out && len_out && score_out, 0, BEAM_NOT_TFM)) return rc;
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
  // beam_shared_tile keep the host-side loop with one round trip per step (beam_host_impl).
  if (int rc = tfm_check(c, memory && seq_out && len_out && score_out && N >= 1 && T >= 1, T, BEAM_NOT_TFM)) return rc;
  if (beam_size < 1 || beam_size > 16) return fail(c, D2T_EINVAL, "beam_size must be in [1,16]");
  if ((long long)beam_size * c->cfg.vocab > 16 * 4096) return fail(c, D2T_EINVAL, "beam_size * vocab too large");
  const bool on_device = c->dec_absorbed && !c->beam_shared_tile && c->cfg.max_seq_len + 2 <= 512 && N <= BEAM_MAX_N &&
                         D2T_PROBE_ENV_STR("D2T_BEAM_HOST") == nullptr;
  return (on_device ? beam_device_impl(c, memory, N, T, beam_size, seq_out, len_out, score_out, (hipStream_t)stream, nullptr)
                    : beam_host_impl(c, memory, N, T, beam_size, seq_out, len_out, score_out, (hipStream_t)stream));
}

}  // extern "C"
