// libd2t engine, LSTM-attention heads: the greedy decode (synchronous and pipelined) and the beam search of the C-ABI -- its
// host loop and the device-side loop beside it, which keep one bookkeeping record (attn_beam_host.h: the host loop runs its
// host functions, the device-side loop the kernels of attn_beam.hip) in one workspace layout.  Host code only: the kernels
// are recurrent.hip's and attn_beam.hip's.
#include "engine_tfm.h"  // (engine_impl.h, carve.h; the captured-loop cache)

namespace {  // (outside extern "C": what is local here stays out of the library's dynamic symbols)
// The fields of the LSTM-attention decoder launch that every caller sets alike: memory [*][T][H], its key projection kp,
// the weights.  The caller adds its outputs, row count, step count and (beam search) the step-mode fields.
AttnDecP attn_dec_params(const d2t_ctx* c, const float* memory, int T, const float* kp) {
  const d2t_config& g = c->cfg;
  AttnDecP p{};
  p.mem = memory; p.T = T; p.D = g.attn_hidden; p.key_off = g.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0;
  p.init_mode = !g.attn_enc_init ? 0 : (g.attn_keys == D2T_ATTN_KEYS_ALL_INIT_MEAN ? 1 : 2);
  p.kp = kp; p.wq_t = c->attn.wq_t; p.bq = c->attn.bq; p.wloc = c->attn.wloc; p.bloc = c->attn.bloc;
  p.taps = c->attn.taps; p.wscore = c->attn.wscore; p.bscore = c->attn.bscore;
  p.wx_t = c->attn.wx_t; p.bx = c->attn.bx; p.wg_t = c->attn.wg_t; p.bg = c->attn.bg;
  p.wih_t = c->attn.wih_t; p.bih = c->attn.bih; p.wic_t = c->attn.wic_t; p.bic = c->attn.bic;
  p.emb = c->attn.emb; p.tokgate = c->attn.tokgate;
  p.V = g.vocab; p.H = g.attn_hidden; p.E = g.attn_hidden; p.coverage = g.attn_coverage; p.end_token = 1;  // attn_converter.py:8
  return p;
}
// What every greedy call of the LSTM-attention heads refuses, before anything is enqueued.
int attn_greedy_check(d2t_ctx* c, const float* memory, int B, int T, const int64_t* tokens, const float* probs) {
  if (!c || !memory || !tokens || !probs || B < 1 || T < 1) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  const d2t_config& g = c->cfg;
  if (g.decoder != D2T_DEC_ATTN) return fail(c, D2T_ESTATE, "context was not created with the Attn decoder");
  const int key_off = g.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0;
  if (T - key_off < 1 || T - key_off > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d unsupported", T);
  if (g.vocab > D2T_ATTN_MAX_CLASSES) return fail(c, D2T_EINVAL, "Attn decoder supports num_class <= %d, got %d", D2T_ATTN_MAX_CLASSES, g.vocab);
  return D2T_OK;
}

// Greedy decode of the LSTM-attention heads.  Synchronous (async == false): everything on the caller's stream, in chain
// 0's workspace.  Asynchronous: the chains take turns; the key projection, the one-launch step loop and the finalize
// kernel run on the chain's stream, ordered behind the caller's stream by an event, and the call returns once they are
// enqueued (no host synchronisation).  A chain's stream is in order, so its workspace (key projection, state block) is
// never rewritten under a loop that still reads it.
// is_test: the reference's early exit is taken inside the kernel (AttnDecP::exit_state) and the finalize kernel zeroes
// what lies behind it and leaves the step count in the state block: one path for the rule, synchronous or not.
int attn_greedy_impl(d2t_ctx* c, const float* memory, int B, int T, int is_test, int64_t* tokens, float* probs, float* alpha,
                     int* steps_out, hipStream_t user, bool async) {
  const d2t_config& g = c->cfg;
  const int Hh = g.attn_hidden, S = g.batch_max_length + 1, V = g.vocab;
  const int key_off = g.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0;
  const int chain = async ? (int)(c->decode_seq++ % (unsigned)c->n_chains) : 0;
  d2t_ctx::Chain& ch = c->chains[chain];
  hipStream_t s = async ? ch.stream : user;
  int rc;
  // workspace of the chain: key_proj(memory) [B*T][H]; state: exit word | steps | pad (16 bytes) | end_step [B]
  if ((rc = ensure(c, &ch.dws, &ch.dws_cap, ((size_t)B * T * Hh + 16) * 4))) return rc;
  if ((rc = ensure(c, &ch.dstate, &ch.dstate_cap, ((size_t)B + 4) * 4))) return rc;
  float* kp = ch.dws;
  unsigned long long* exit_state = reinterpret_cast<unsigned long long*>(ch.dstate);
  int* steps_dev = ch.dstate + 2;
  int* end_step = ch.dstate + 4;
  if (async) {  // the chain's stream starts behind the caller's work (the memory)
    HIPCHK(c, hipEventRecord(c->ev_in, user));
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_in, 0));
  } else if (c->ev_done_valid[chain]) {  // an asynchronous decode of this chain may still read the workspace
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_done[chain], 0));
  }
  HIPCHK(c, linear_any(nullptr, s, memory, c->attn.key, nullptr, kp, B * T, ACT_NONE));
  HIPCHK(c, hipMemsetAsync(ch.dstate, 0, 16, s));
  HIPCHK(c, hipMemsetAsync(end_step, 0xFF, (size_t)B * 4, s));  // -1 = never emitted [s]
  AttnDecP p = attn_dec_params(c, memory, T, kp);
  p.probs = probs; p.tokens = tokens; p.end_step = end_step;
  p.sv_alpha = alpha;  // optional [B][S][Tk]: the alignment of every step (viz_attn, seq2seq.py:267-272,300-301)
  p.B = B; p.S = S;
  p.exit_state = is_test ? exit_state : nullptr;
  HIPCHK(c, launch_attn_decode(p, s));
  // reference: break after the first step at which every row has emitted [s]; its pre-zeroed outputs keep zeros behind it
  if (is_test) HIPCHK(c, launch_attn_decode_finalize(exit_state, steps_dev, B, S, V, T - key_off, tokens, probs, alpha, s));
  int steps = S;
  if (async) {
    HIPCHK(c, hipEventRecord(c->ev_done[chain], s));
    c->ev_done_valid[chain] = true;
    if ((rc = issue_ticket(c, s, is_test ? 1 : -S, steps_dev))) return rc;  // the ticket counter and ring of the TFM decodes
  } else if (is_test) {
    HIPCHK(c, hipMemcpyAsync(c->h_pinned, steps_dev, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    steps = c->h_pinned[0];
  }
  if (steps_out) *steps_out = steps;
  return D2T_OK;
}

// ---- greedy decode groups: several encoder batches of different sizes in one launch ----
constexpr int ATTN_GRP_MAXROWS = 1024;  // rows of one group (one 1024-thread block each: four rounds of a 256-CU part)
// The chain's state block as a group lays it out (ints): exit words u64 [64] | steps [64] | batch_rows [64] | row0 [B] | len [B]
// | row_batch [B] | end_step [B].  The pinned staging holds the part from batch_rows up to end_step, so the four tables go
// up in one copy.  Every decode of a chain sets its state block up on the chain's in-order stream before it reads it, so the
// uniform layout ([0..1] exit word, [2] steps, [4..] end_step) and this one can take turns.
constexpr int ATTN_GRP_STEPS = 2 * GRP_MAXB, ATTN_GRP_TABS = 3 * GRP_MAXB, ATTN_GRP_ROW0 = 4 * GRP_MAXB;

// d2t_decode_attn_greedy_submit for the rows of nb batches, batch k with rows[k] rows over a memory of Ts[k] tokens, packed in
// `memory` ([mem_rows][H], batch after batch): the next chain in turn, its stream behind the caller's; the tables uploaded
// from one of the chain's two pinned staging slots (rewritten only once its last upload has run); ONE key projection over all packed rows
// (linear_any computes a row from that row alone, so each batch's projection is its uniform call's bit for bit), the state
// block set up, one loop launch over all B rows (the group builds of attn_decode_kernel), one finalize launch, one ticket
// with a step count per batch.  The caller has checked everything: nothing is refused here.
int attn_greedy_group_impl(d2t_ctx* c, const float* memory, int nb, const int32_t* rows, const int32_t* Ts, int B, size_t mem_rows,
                           int Tmax, int is_test, int64_t* tokens, float* probs, hipStream_t user) {
  const d2t_config& g = c->cfg;
  const int Hh = g.attn_hidden, S = g.batch_max_length + 1, V = g.vocab;
  const int chain = (int)(c->decode_seq++ % (unsigned)c->n_chains);
  d2t_ctx::Chain& ch = c->chains[chain];
  hipStream_t s = ch.stream;
  int rc;
  if ((rc = ensure(c, &ch.dws, &ch.dws_cap, (mem_rows * Hh + 16) * 4))) return rc;
  if ((rc = ensure(c, &ch.dstate, &ch.dstate_cap, ((size_t)ATTN_GRP_ROW0 + 4 * (size_t)B + 4) * 4))) return rc;
  // the chain's two staging slots take turns: a slot is rewritten only once its last upload has run, and that upload stands
  // in front of the chain's loop before last, so the host waits here only when three groups of one chain are backed up
  const int slot = (int)(ch.agrp_seq++ & 1u);
  if (!ch.agrp_host[slot]) {
    int* host = nullptr;
    hipEvent_t ev = nullptr;
    if (hipHostMalloc(reinterpret_cast<void**>(&host), ((size_t)GRP_MAXB + 3 * ATTN_GRP_MAXROWS) * 4, hipHostMallocDefault) != hipSuccess)
      return fail(c, D2T_ENOMEM, "hipHostMalloc failed");
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {  // (a slot exists with its event or not at all)
      hipHostFree(host);
      return fail(c, D2T_EHIP, "hipEventCreateWithFlags failed");
    }
    ch.agrp_host[slot] = host;
    ch.agrp_ev[slot] = ev;
  } else {
    HIPCHK(c, hipEventSynchronize(ch.agrp_ev[slot]));
  }
  int* h = ch.agrp_host[slot];
  int *h_rows = h, *h_row0 = h + GRP_MAXB, *h_len = h_row0 + B, *h_rb = h_len + B;
  for (int k = 0, b = 0, base = 0; k < nb; ++k) {
    h_rows[k] = rows[k];
    for (int i = 0; i < rows[k]; ++i, ++b) { h_row0[b] = base + i * Ts[k]; h_len[b] = Ts[k]; h_rb[b] = k; }
    base += rows[k] * Ts[k];
  }
  for (int k = nb; k < GRP_MAXB; ++k) h_rows[k] = 0;
  float* kp = ch.dws;
  unsigned long long* exit_state = reinterpret_cast<unsigned long long*>(ch.dstate);
  int* steps_dev = ch.dstate + ATTN_GRP_STEPS;
  int* tab = ch.dstate + ATTN_GRP_TABS;
  int* end_step = ch.dstate + ATTN_GRP_ROW0 + 3 * (size_t)B;
  // the tables go up first: the upload needs nothing of the caller's stream, so it does not wait for the caller's encoder
  HIPCHK(c, hipMemcpyAsync(tab, h, ((size_t)GRP_MAXB + 3 * (size_t)B) * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(ch.agrp_ev[slot], s));
  HIPCHK(c, hipEventRecord(c->ev_in, user));  // the rest of the chain's work starts behind the caller's (the memory)
  HIPCHK(c, hipStreamWaitEvent(s, c->ev_in, 0));
  HIPCHK(c, linear_any(nullptr, s, memory, c->attn.key, nullptr, kp, (int)mem_rows, ACT_NONE));
  HIPCHK(c, hipMemsetAsync(ch.dstate, 0, (size_t)ATTN_GRP_TABS * 4, s));  // the exit words and the steps
  HIPCHK(c, hipMemsetAsync(end_step, 0xFF, (size_t)B * 4, s));            // -1 = never emitted [s]
  AttnDecP p = attn_dec_params(c, memory, Tmax, kp);
  p.probs = probs; p.tokens = tokens; p.end_step = end_step;
  p.B = B; p.S = S;
  p.exit_state = is_test ? exit_state : nullptr;
  p.grp_row0 = tab + GRP_MAXB; p.grp_len = p.grp_row0 + B; p.grp_row_batch = p.grp_len + B; p.grp_batch_rows = tab;
  HIPCHK(c, launch_attn_decode(p, s));
  if (is_test)
    HIPCHK(c, launch_attn_decode_finalize_group(exit_state, steps_dev, p.grp_row_batch, p.grp_batch_rows, nb, B, S, V, tokens, probs, s));
  HIPCHK(c, hipEventRecord(c->ev_done[chain], s));
  c->ev_done_valid[chain] = true;
  return issue_ticket(c, s, is_test ? nb : -S, steps_dev);
}

// ---- beam search: what the two loops share ----
constexpr int ATTN_BEAM_MAX_N = 1024;  // samples of one ragged search (as the TFM head's ragged search)
// What every beam search of the LSTM-attention heads refuses, behind the entry's own argument check.
int attn_beam_check(d2t_ctx* c, int beam_size) {
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  const d2t_config& g = c->cfg;
  if (g.decoder != D2T_DEC_ATTN) return fail(c, D2T_ESTATE, "context was not created with the Attn decoder");
  if (!g.attn_coverage && g.attn_cell != D2T_ATTN_CELL_BAHDANAU)
    return fail(c, D2T_ESTATE, "LSTM beam search is implemented for the coverage and Bahdanau cells (the reference's 'loc_aware' beam "
                "hands the previous beam's un-reordered alignment to the next step, seq2seq.py:207)");
  if (beam_size < 1 || beam_size > 16) return fail(c, D2T_EINVAL, "beam_size must be in [1,16]");
  return D2T_OK;
}
// What the ragged entries (synchronous and submitted) refuse alike: missing arguments, attn_beam_check, the sample count and
// every sample's memory length.
int attn_beam_ragged_check(d2t_ctx* c, const float* memory, int N, const int32_t* T, int beam_size, const void* seq,
                           const void* len, const void* score) {
  if (!c || !memory || !T || !seq || !len || !score) return fail(c, D2T_EINVAL, "bad argument");
  if (int rc = attn_beam_check(c, beam_size)) return rc;
  if (N < 1 || N > ATTN_BEAM_MAX_N)
    return fail(c, D2T_EINVAL, "ragged beam search takes 1 to %d samples per call, got %d", ATTN_BEAM_MAX_N, N);
  const int key_off = c->cfg.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0;
  for (int i = 0; i < N; ++i)
    if (T[i] - key_off < 1 || T[i] - key_off > memory_cap(c))
      return fail(c, D2T_EINVAL, "sample %d has memory length %d, supported are %d to %d", i, T[i], 1 + key_off, memory_cap(c) + key_off);
  return D2T_OK;
}
// Alignment maps (viz_attn): every step's launch writes its rows' alignments into its own slice of a history; the slices
// [S][N * beam][Tk] of one search must fit the budget.
int attn_beam_hist_check(d2t_ctx* c, int S, int N, int beam_size, int Tk) {
  const size_t hist_bytes = (size_t)S * N * beam_size * Tk * 4;
  if (hist_bytes > D2T_ATTN_MAP_BUDGET)
    return fail(c, D2T_EINVAL, "beam alignment history of %zu bytes (%d steps x %d samples x beam %d x %d keys x 4) exceeds the "
                "%llu-byte budget: decode fewer samples per call", hist_bytes, S, N, beam_size, Tk, (unsigned long long)D2T_ATTN_MAP_BUDGET);
  return D2T_OK;
}
// The memory rows of a search: uniform (Ts == nullptr) N * *T; ragged the sum of Ts [N], and *T becomes the largest.
size_t attn_beam_mem_rows(int N, const int32_t* Ts, int* T) {
  if (!Ts) return (size_t)N * *T;
  size_t rows = 0;
  *T = 0;
  for (int i = 0; i < N; ++i) { rows += (size_t)Ts[i]; *T = std::max(*T, (int)Ts[i]); }
  return rows;
}

// The workspace of a search: logits [cap][V] | topv [cap] | topi [cap] (adjacent: the host loop fetches both in one copy per
// step) | h_in c_in h_out c_out [cap][H] | mem_in mem_out [cap][ld] | end_step [cap] | dummy tokens i64 [cap] | the per-sample
// tables row0 [N] | T [N] | the live rows of the record (attn_beam_rows_carve: the host loop's one upload per step), and for
// the device-side loop the result block seq i64 [N][S] | len [N] | score [N] | ctrl [4] (one device -> host copy at the end
// of a synchronous search; ctrl heads the record's bookkeeping, which follows it).  Every array but topi from a 16-byte
// boundary.  A function of N, beam, V, S and ld alone: no memory length moves it.
struct AttnBeamWs {
  float *logits, *topv, *st[6];  // st: h_in c_in h_out c_out mem_in mem_out
  int *topi, *end, *tab;
  int64_t* dummy;
  AttnBeamDev rec;
  char* rows; size_t rows_bytes;
  char* res; size_t res_bytes;
  int64_t* r_seq; int* r_len; float* r_score;
};
void attn_beam_rows(Carver& cv, AttnBeamWs* w) {
  cv.align(16);
  w->rows = cv.here();
  attn_beam_rows_carve(cv, w->rec);
  w->rows_bytes = (size_t)(cv.here() - w->rows);
}
size_t attn_beam_ws_carve(Carver cv, int Hh, int ld, bool device_book, AttnBeamWs* w) {
  AttnBeamDev& r = w->rec;
  const size_t cap = (size_t)r.cap, N = (size_t)r.N;
  w->logits = cv.take<float>(cap * r.V, 16);
  w->topv = cv.take<float>(cap, 16);
  w->topi = cv.take<int>(cap);
  for (int i = 0; i < 6; ++i) w->st[i] = cv.take<float>(cap * (i < 4 ? Hh : ld), 16);
  w->end = cv.take<int>(cap, 16);
  w->dummy = cv.take<int64_t>(cap, 16);
  w->tab = cv.take<int>(2 * N, 16);
  attn_beam_rows(cv, w);
  if (device_book) {
    w->res = cv.here();
    w->r_seq = cv.take<int64_t>(N * r.S, 16);
    w->r_len = cv.take<int>(N, 16);
    w->r_score = cv.take<float>(N, 16);
    attn_beam_book_carve(cv, r);
    w->res_bytes = (size_t)(reinterpret_cast<char*>(r.ctrl + 4) - w->res);
  }
  r.topv = w->topv; r.topi = w->topi;
  return cv.total() + 64;
}
// The host loop's pinned mirror: the live rows | topv [cap] | topi [cap] | the tables
size_t attn_beam_mirror_carve(Carver cv, AttnBeamWs* w) {
  attn_beam_rows(cv, w);
  w->topv = cv.take<float>(w->rec.cap, 16);
  w->topi = cv.take<int>(w->rec.cap);
  w->tab = cv.take<int>(2 * (size_t)w->rec.N, 16);
  return cv.total();
}
// The step launch of a search, on top of attn_dec_params: one step per launch (the greedy kernel in step mode, one block per
// hypothesis row) from and into the workspace's state buffers, its token and sample per row from the record's live rows.
// ragged: the per-sample tables and the row stride st_ld of the coverage memory (the ragged builds of the step kernel).
AttnDecP attn_beam_step_params(const d2t_ctx* c, const float* memory, int T, const float* kp, const AttnBeamWs& w, bool ragged,
                               int st_ld) {
  AttnDecP p = attn_dec_params(c, memory, T, kp);
  p.probs = w.logits; p.tokens = w.dummy; p.end_step = w.end;
  p.S = 1; p.coverage = 1;
  p.step_mode = 1;
  p.st_h_in = w.st[0]; p.st_c_in = w.st[1]; p.st_mem_in = w.st[4];
  p.st_h_out = w.st[2]; p.st_c_out = w.st[3]; p.st_mem_out = w.st[5];
  p.tok_in = w.rec.tok; p.row_sample = w.rec.map;
  if (ragged) { p.smp_row0 = w.tab; p.smp_T = w.tab + w.rec.N; p.st_ld = st_ld; }
  return p;
}

// Attention / AttentionV2.forward_beam for N samples in one step loop: rows = live hypotheses of all samples, each
// attending over its own sample's keys (row map).  The attention cell + LSTMCell + generator of every live hypothesis run
// as ONE launch per step, log_softmax + top-k per sample segment on the device, the reference's bookkeeping -- with its
// quirks -- on the host in the record of attn_beam_host.h: its live rows lie in the pinned mirror and go to the device in one
// copy per step, its bookkeeping half is pageable (only the host reads it).  Any N: nothing here has the kernels' sample limit.
// Uniform (Ts == nullptr): memory [N][T][H].  Ragged (Ts = host [N], T unused): memory is packed, sample i's Ts[i] rows
// behind sample i-1's; ONE key projection over all packed rows (linear_any computes a row from that row alone, so each
// sample's projection is its uniform call's bit for bit), the per-sample tables [row0 | T] uploaded once in front of the
// loop, and the coverage memory, the alignment history and alpha_out [N][S][st_ld] on the row stride st_ld = the largest Tk.
// The bookkeeping does not know which of the two it serves.  The caller has checked the lengths.
int attn_beam_impl(d2t_ctx* c, const float* memory, int N, int T, const int32_t* Ts, int beam_size, int64_t* seq_out,
                   int32_t* len_out, float* score_out, float* alpha_out, hipStream_t s) {
  const d2t_config& g = c->cfg;
  const int Hh = g.attn_hidden, S = g.batch_max_length + 1, V = g.vocab, cap = N * beam_size;
  const size_t mem_rows = attn_beam_mem_rows(N, Ts, &T);
  const int Tk = T - (g.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0);  // ragged: the largest, = st_ld
  int rc;
  // the alignment history [S][cap][Tk], kept apart from the workspace; the chosen paths [N][S] and lengths [N] follow it
  float* d_hist = nullptr;
  int* d_path = nullptr;
  if (alpha_out) {
    if ((rc = attn_beam_hist_check(c, S, N, beam_size, Tk))) return rc;
    if ((rc = ensure(c, &c->beam_hist, &c->beam_hist_cap, ((size_t)S * cap * Tk + (size_t)N * (S + 1) + 16) * 4))) return rc;
    d_hist = c->beam_hist;
    d_path = reinterpret_cast<int*>(d_hist + (size_t)S * cap * Tk);
  }
  // the key projection lives in chain 0's workspace, like the synchronous greedy call's: behind that chain's last
  // asynchronous greedy decode (d2t_decode_attn_greedy_submit), which may still read it
  d2t_ctx::Chain& ch = c->chains[0];
  if (c->ev_done_valid[0]) HIPCHK(c, hipStreamWaitEvent(s, c->ev_done[0], 0));
  if ((rc = ensure(c, &ch.dws, &ch.dws_cap, (mem_rows * Hh + 16) * 4))) return rc;
  float* kp = ch.dws;
  AttnBeamWs dv{}, hv{};  // the device view and the host's
  dv.rec.N = N; dv.rec.beam = beam_size; dv.rec.cap = cap; dv.rec.V = V; dv.rec.S = S; dv.rec.end_token = 1;  // attn_converter.py:8
  hv.rec = dv.rec;
  if ((rc = ensure(c, &c->beam_ws, &c->beam_ws_cap, attn_beam_ws_carve(Carver(), Hh, Tk, false, &dv)))) return rc;
  attn_beam_ws_carve(Carver(c->beam_ws), Hh, Tk, false, &dv);
  if ((rc = ensure_host_beam(c, attn_beam_mirror_carve(Carver(), &hv)))) return rc;
  attn_beam_mirror_carve(Carver(c->h_beam), &hv);
  AttnBeamDev& r = hv.rec;
  Carver measure;
  attn_beam_book_carve(measure, r);
  std::vector<char> book(measure.total());
  Carver bc(book.data());
  attn_beam_book_carve(bc, r);
  HIPCHK(c, linear_any(nullptr, s, memory, c->attn.key, nullptr, kp, (int)mem_rows, ACT_NONE));
  AttnDecP p = attn_beam_step_params(c, memory, T, kp, dv, Ts != nullptr, Tk);
  if (Ts) {  // (the previous search has synchronised: the mirror is idle)
    d2t_ragged_beam_tables(N, Ts, hv.tab, hv.tab + N);
    HIPCHK(c, hipMemcpyAsync(dv.tab, hv.tab, 2 * (size_t)N * 4, hipMemcpyHostToDevice, s));
  }
  attn_beam_host_init(r, 0);  // [GO] = 0
  HIPCHK(c, hipMemcpyAsync(dv.rows, hv.rows, hv.rows_bytes, hipMemcpyHostToDevice, s));
  for (int step = 0; step < S; ++step) {
    p.B = r.ctrl[1]; p.first = step == 0;
    if (d_hist) p.sv_alpha = d_hist + (size_t)step * cap * Tk;
    HIPCHK(c, launch_attn_decode(p, s));
    HIPCHK(c, launch_beam_topk_batch(dv.logits, dv.rec.scores, dv.rec.seg, N, V, beam_size, dv.topv, dv.topi, s));
    HIPCHK(c, hipMemcpyAsync(hv.topv, dv.topv, 2 * (size_t)cap * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const int rows = attn_beam_host_advance(r, hv.topv, hv.topi);
    if (!rows || step + 1 == S) break;
    HIPCHK(c, hipMemcpyAsync(dv.rows, hv.rows, hv.rows_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_gather_rows(dv.st[2], dv.st[0], dv.rec.idx_h, rows, Hh, s));
    HIPCHK(c, launch_gather_rows(dv.st[3], dv.st[1], dv.rec.idx_h, rows, Hh, s));
    HIPCHK(c, launch_gather_rows(dv.st[5], dv.st[4], dv.rec.idx_m, rows, Tk, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  std::vector<int64_t> seq((size_t)N * S);
  std::vector<int> path(alpha_out ? (size_t)N * (S + 1) : 0);  // maps: [N][S] chosen paths | [N] lengths, uploaded in one copy
  attn_beam_host_finish(r, seq.data(), len_out, score_out, alpha_out ? path.data() : nullptr,
                        alpha_out ? path.data() + (size_t)N * S : nullptr);
  for (int i = 0; i < N; ++i)  // the tokens of the sample's length, nothing behind
    std::copy_n(seq.begin() + (size_t)i * S, len_out[i], seq_out + (size_t)i * S);
  if (alpha_out) {  // seqs_alpha[best][1:] of every sample: one upload, one gather over all samples
    HIPCHK(c, hipMemcpyAsync(d_path, path.data(), path.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_attn_alpha_gather(d_hist, d_path, d_path + (size_t)N * S, alpha_out, N, S, cap, Tk, s));
    HIPCHK(c, hipStreamSynchronize(s));  // path is pageable and local
  }
  return D2T_OK;
}

constexpr int ATTN_BEAM_LD_QUANTUM = 256;  // the device-side loop's row stride of state and history: the largest Tk rounded up to this

// The search of attn_beam_impl with the bookkeeping ON THE DEVICE (attn_beam.hip): the reference's per-step walk is
// attn_beam_dev_advance_kernel behind the per-sample top-k, the three gathers are one launch, the final pick is
// attn_beam_dev_finish_kernel, and the step kernel runs for all N x beam row slots under a guard on the record's control
// words -- no host round trip inside the search, which is therefore ONE captured graph: init, S x (step, top-k, advance,
// gather), finish.  Always the ragged builds of the step kernel (a uniform call fills the tables with row0 = i * T), on the
// row stride ld = the largest Tk rounded up to 256 (held to Tk where the history would otherwise leave the budget), so the
// graph depends on N, beam, ld, maps on / off and the chain's buffers, and on no memory length.  The packed memory is copied
// into the chain's own buffer in front of the key projection: every pointer inside the graph is the engine's.  The results
// land in the chain's result block; the alignment gather and the copies into the caller's buffers follow the graph (they
// name caller addresses, which the graph must not).
// The search runs on its chain's stream, behind the caller's.  Synchronous (async == false): chain 0, one device -> host copy
// of the result block, one synchronisation; seq_out / len_out / score_out are host arrays.  Submitted: the chains take turns,
// the outputs are device buffers, ev_done orders later users of the chain's key-projection workspace, a ticket reports the
// steps executed, and nothing here waits for the device (growing a buffer aside; and a table slot of the ring still waiting
// for its upload, which takes ABEAM_TABS searches in flight).
int attn_beam_dev_impl(d2t_ctx* c, const float* memory, int N, int T, const int32_t* Ts, int beam_size, int64_t* seq_out,
                       int32_t* len_out, float* score_out, float* alpha_out, hipStream_t user, bool async) {
  const d2t_config& g = c->cfg;
  const int Hh = g.attn_hidden, S = g.batch_max_length + 1, V = g.vocab, cap = N * beam_size;
  if (N > ATTN_BEAM_MAX_N)
    return fail(c, D2T_EINVAL, "the device-side beam search takes 1 to %d samples per call, got %d", ATTN_BEAM_MAX_N, N);
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, alpha_out, "alpha")) return rc;
  std::vector<int32_t> uniform;
  if (!Ts) { uniform.assign((size_t)N, T); Ts = uniform.data(); }
  const size_t mem_rows = attn_beam_mem_rows(N, Ts, &T);
  const int Tk = T - (g.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0);  // the largest
  int ld = (Tk + ATTN_BEAM_LD_QUANTUM - 1) / ATTN_BEAM_LD_QUANTUM * ATTN_BEAM_LD_QUANTUM;
  if (alpha_out) {
    if (int rc = attn_beam_hist_check(c, S, N, beam_size, Tk)) return rc;
    if ((size_t)S * cap * ld * 4 > D2T_ATTN_MAP_BUDGET) ld = Tk;
  }
  // ---- nothing is refused below this line ----
  const int chain = async ? (int)(c->decode_seq++ % (unsigned)c->n_chains) : 0;
  d2t_ctx::Chain& ch = c->chains[chain];
  hipStream_t s = ch.stream;
  int rc;
  AttnBeamWs ws{};
  ws.rec.N = N; ws.rec.beam = beam_size; ws.rec.cap = cap; ws.rec.V = V; ws.rec.S = S; ws.rec.end_token = 1;  // attn_converter.py:8
  if ((rc = ensure(c, &ch.abeam_ws, &ch.abeam_ws_cap, attn_beam_ws_carve(Carver(), Hh, ld, true, &ws)))) return rc;
  attn_beam_ws_carve(Carver(ch.abeam_ws), Hh, ld, true, &ws);
  if ((rc = ensure(c, &ch.abeam_mem, &ch.abeam_mem_cap, (mem_rows * Hh + 16) * 4))) return rc;
  if ((rc = ensure(c, &ch.dws, &ch.dws_cap, (mem_rows * Hh + 16) * 4))) return rc;
  float* d_hist = nullptr;
  int* d_path = nullptr;
  if (alpha_out) {  // history [S][cap][ld] | chosen paths [N][S] | their lengths [N]
    if ((rc = ensure(c, &ch.abeam_hist, &ch.abeam_hist_cap, ((size_t)S * cap * ld + (size_t)N * (S + 1) + 16) * 4))) return rc;
    d_hist = ch.abeam_hist;
    d_path = reinterpret_cast<int*>(d_hist + (size_t)S * cap * ld);
  }
  if (!async && (rc = ensure_host_beam(c, ws.res_bytes))) return rc;
  // the per-sample tables: the next slot of the pinned ring, rewritten only once its last upload has run
  const int slot = (int)(c->abeam_tab_seq++ % (unsigned)d2t_ctx::ABEAM_TABS);
  if (!c->abeam_tab_host[slot]) {
    if (hipHostMalloc(reinterpret_cast<void**>(&c->abeam_tab_host[slot]), (size_t)2 * ATTN_BEAM_MAX_N * 4, hipHostMallocDefault) != hipSuccess) {
      c->abeam_tab_host[slot] = nullptr;
      return fail(c, D2T_ENOMEM, "hipHostMalloc failed");
    }
    HIPCHK(c, hipEventCreateWithFlags(&c->abeam_tab_ev[slot], hipEventDisableTiming));
  } else {
    HIPCHK(c, hipEventSynchronize(c->abeam_tab_ev[slot]));
  }
  int* h_tab = c->abeam_tab_host[slot];
  d2t_ragged_beam_tables(N, Ts, h_tab, h_tab + N);
  HIPCHK(c, hipEventRecord(c->ev_in, user));  // the chain's stream starts behind the caller's work (the memory)
  HIPCHK(c, hipStreamWaitEvent(s, c->ev_in, 0));
  HIPCHK(c, hipMemcpyAsync(ws.tab, h_tab, 2 * (size_t)N * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(c->abeam_tab_ev[slot], s));
  HIPCHK(c, hipMemcpyAsync(ch.abeam_mem, memory, mem_rows * Hh * 4, hipMemcpyDeviceToDevice, s));
  float* kp = ch.dws;
  HIPCHK(c, linear_any(nullptr, s, ch.abeam_mem, c->attn.key, nullptr, kp, (int)mem_rows, ACT_NONE));
  const AttnBeamDev& b = ws.rec;
  AttnDecP p = attn_beam_step_params(c, ch.abeam_mem, T, kp, ws, true, ld);
  p.B = cap;
  p.guard = b.ctrl;
  auto enqueue_loop = [&](hipStream_t st) -> hipError_t {
    hipError_t e;
#define LTRY(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)
    LTRY(launch_attn_beam_dev_init(b, 0, st));  // [GO] = 0
    for (int step = 0; step < S; ++step) {  // the steps differ in p.first and in their slice of the history
      p.first = step == 0;
      p.sv_alpha = d_hist ? d_hist + (size_t)step * cap * ld : nullptr;
      LTRY(launch_attn_decode(p, st));
      LTRY(launch_beam_topk_batch(ws.logits, b.scores, b.seg, N, V, beam_size, ws.topv, ws.topi, st, b.ctrl, b.ctrl + 2));
      LTRY(launch_attn_beam_dev_advance(b, st));
      if (step + 1 < S)
        LTRY(launch_attn_beam_dev_gather(b.ctrl, b.idx_h, b.idx_m, ws.st[2], ws.st[3], ws.st[5], ws.st[0], ws.st[1], ws.st[4], cap, Hh, ld, st));
    }
    LTRY(launch_attn_beam_dev_finish(b, ws.r_seq, ws.r_len, ws.r_score, d_path, d_path ? d_path + (size_t)N * S : nullptr, st));
#undef LTRY
    return hipSuccess;
  };
  if (D2T_PROBE_ENV_STR("D2T_NO_GRAPH") == nullptr) {
    d2t_ctx::GraphKey k;
    memset(&k, 0, sizeof k);
    k.loop = d2t_ctx::LOOP_ATTN_BEAM_DEV;
    k.B = cap; k.T = ld; k.steps = S; k.N = N; k.beam = beam_size; k.dev_exit = d_hist ? 1 : 0;
    k.tok = ch.abeam_mem; k.logits = ch.abeam_ws; k.ckv = d_hist; k.dws = ch.dws;
    hipGraphExec_t exec = nullptr;
    if ((rc = tfm::cached_graph(c, s, k, "Attn beam", enqueue_loop, &exec))) return rc;
    HIPCHK(c, hipGraphLaunch(exec, s));
  } else {
    HIPCHK(c, enqueue_loop(s));
  }
  ++c->attn_beam_dev_runs;
  if (alpha_out) HIPCHK(c, launch_attn_alpha_gather_ld(d_hist, d_path, d_path + (size_t)N * S, alpha_out, N, S, cap, ld, Tk, s));
  if (async) {
    HIPCHK(c, hipMemcpyAsync(seq_out, ws.r_seq, (size_t)N * S * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(len_out, ws.r_len, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(score_out, ws.r_score, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipEventRecord(c->ev_done[chain], s));
    c->ev_done_valid[chain] = true;
    return issue_ticket(c, s, 1, b.ctrl + 3);  // one entry: the steps the search executed
  }
  HIPCHK(c, hipMemcpyAsync(c->h_beam, ws.res, ws.res_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  // the host's view of the result block: the same offsets from the pinned copy's base
  const int64_t* h_seq = reinterpret_cast<const int64_t*>(c->h_beam + (reinterpret_cast<char*>(ws.r_seq) - ws.res));
  const int* h_len = reinterpret_cast<const int*>(c->h_beam + (reinterpret_cast<char*>(ws.r_len) - ws.res));
  const float* h_score = reinterpret_cast<const float*>(c->h_beam + (reinterpret_cast<char*>(ws.r_score) - ws.res));
  for (int i = 0; i < N; ++i) {  // as the host loop leaves them: the tokens of the sample's length, nothing behind
    const int n = std::min(std::max(h_len[i], 0), S);
    std::copy_n(h_seq + (size_t)i * S, n, seq_out + (size_t)i * S);
    len_out[i] = n;
    score_out[i] = h_score[i];
  }
  return D2T_OK;
}
}  // namespace

extern "C" {

int d2t_decode_attn_greedy(d2t_ctx* c, const float* memory, int32_t B, int32_t T, int32_t is_test, int64_t* tokens,
                           float* probs, int32_t* steps_out, d2t_stream stream) {
  return d2t_decode_attn_greedy_alpha(c, memory, B, T, is_test, tokens, probs, nullptr, steps_out, stream);
}

int d2t_decode_attn_greedy_alpha(d2t_ctx* c, const float* memory, int32_t B, int32_t T, int32_t is_test, int64_t* tokens,
                                 float* probs, float* alpha, int32_t* steps_out, d2t_stream stream) {
  DevGuard dg_(c);
  if (!steps_out) return fail(c, D2T_EINVAL, "bad argument");
  if (int rc = attn_greedy_check(c, memory, B, T, tokens, probs)) return rc;
  return attn_greedy_impl(c, memory, B, T, is_test, tokens, probs, alpha, steps_out, (hipStream_t)stream, false);
}

int d2t_decode_attn_greedy_submit(d2t_ctx* c, const float* memory, int32_t B, int32_t T, int32_t is_test, int64_t* tokens,
                                  float* probs, float* alpha, d2t_stream stream, int64_t* ticket_out) {
  DevGuard dg_(c);
  if (int rc = attn_greedy_check(c, memory, B, T, tokens, probs)) return rc;
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, probs, "probs")) return rc;
  const int rc = attn_greedy_impl(c, memory, B, T, is_test, tokens, probs, alpha, nullptr, (hipStream_t)stream, true);
  if (rc == D2T_OK && ticket_out) *ticket_out = c->last_ticket;
  return rc;
}

// 1: d2t_decode_attn_greedy_submit_ragged serves this context (any finalized LSTM-attention head); 0: it refuses with D2T_ESTATE
int32_t d2t_decode_attn_supports_ragged_greedy(const d2t_ctx* c) {
  return c && c->finalized && c->cfg.decoder == D2T_DEC_ATTN && c->cfg.vocab <= D2T_ATTN_MAX_CLASSES ? 1 : 0;
}

int d2t_decode_attn_greedy_submit_ragged(d2t_ctx* c, const float* memory, int32_t n_batches, const int32_t* batch_rows,
                                         const int32_t* batch_T, int32_t is_test, int64_t* tokens, float* probs, d2t_stream stream,
                                         int64_t* ticket_out) {
  DevGuard dg_(c);
  // everything is checked before anything is enqueued; the context stays usable after a refusal
  if (!c || !memory || !batch_rows || !batch_T || !tokens || !probs) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  const d2t_config& g = c->cfg;
  if (g.decoder != D2T_DEC_ATTN) return fail(c, D2T_ESTATE, "context was not created with the Attn decoder");
  if (g.vocab > D2T_ATTN_MAX_CLASSES) return fail(c, D2T_EINVAL, "Attn decoder supports num_class <= %d, got %d", D2T_ATTN_MAX_CLASSES, g.vocab);
  if (n_batches < 1 || n_batches > GRP_MAXB) return fail(c, D2T_EINVAL, "a decode group holds 1 to %d batches, got %d", GRP_MAXB, n_batches);
  const int key_off = g.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0;
  long long B = 0, mem_rows = 0;
  int Tmax = 0;
  for (int k = 0; k < n_batches; ++k) {
    if (batch_rows[k] < 1) return fail(c, D2T_EINVAL, "batch %d of the group has %d rows", k, batch_rows[k]);
    if (batch_T[k] - key_off < 1 || batch_T[k] - key_off > memory_cap(c))
      return fail(c, D2T_EINVAL, "batch %d has memory length %d, supported are %d to %d", k, batch_T[k], 1 + key_off, memory_cap(c) + key_off);
    B += batch_rows[k];
    if (B > ATTN_GRP_MAXROWS) return fail(c, D2T_EINVAL, "a decode group of the Attn heads holds at most %d rows", ATTN_GRP_MAXROWS);
    mem_rows += (long long)batch_rows[k] * batch_T[k];
    Tmax = std::max(Tmax, (int)batch_T[k]);
  }
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, tokens, "tokens")) return rc;
  if (int rc = check_dev_ptr(c, probs, "probs")) return rc;
  const int rc = attn_greedy_group_impl(c, memory, n_batches, batch_rows, batch_T, (int)B, (size_t)mem_rows, Tmax, is_test, tokens, probs,
                                        (hipStream_t)stream);
  if (rc == D2T_OK && ticket_out) *ticket_out = c->last_ticket;
  return rc;
}

int d2t_decode_attn_beam(d2t_ctx* c, const float* memory, int32_t T, int32_t beam_size, int64_t* seq_out, int32_t* len_out,
                         float* score_out, d2t_stream stream) {
  DevGuard dg_(c);
  // Attention.forward_beam (prediction_head/seq2seq.py:83-222) / AttentionV2.forward_beam (seq2seq_v2.py:12-174) for
  // one sample: the batched search with N = 1.
  return d2t_decode_attn_beam_batch(c, memory, 1, T, beam_size, seq_out, len_out, score_out, stream);
}

int d2t_decode_attn_beam_batch(d2t_ctx* c, const float* memory, int32_t N, int32_t T, int32_t beam_size, int64_t* seq_out,
                               int32_t* len_out, float* score_out, d2t_stream stream) {
  return d2t_decode_attn_beam_batch_alpha(c, memory, N, T, beam_size, seq_out, len_out, score_out, nullptr, stream);
}

int d2t_decode_attn_beam_batch_alpha(d2t_ctx* c, const float* memory, int32_t N, int32_t T, int32_t beam_size, int64_t* seq_out,
                                     int32_t* len_out, float* score_out, float* alpha_out, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !memory || !seq_out || !len_out || !score_out || N < 1 || T < 1) return fail(c, D2T_EINVAL, "bad argument");
  if (int rc = attn_beam_check(c, beam_size)) return rc;
  const int Tk = T - (c->cfg.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0);
  if (Tk < 1 || Tk > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d unsupported", T);
  if (c->attn_beam_device)
    return attn_beam_dev_impl(c, memory, N, T, nullptr, beam_size, seq_out, len_out, score_out, alpha_out, (hipStream_t)stream, false);
  return attn_beam_impl(c, memory, N, T, nullptr, beam_size, seq_out, len_out, score_out, alpha_out, (hipStream_t)stream);
}

// 1: d2t_decode_attn_beam_batch_ragged serves this context (an LSTM-attention head whose beam search the engine has: the
// coverage and Bahdanau cells); 0: it refuses with D2T_ESTATE
int32_t d2t_decode_attn_supports_ragged_beam(const d2t_ctx* c) {
  return c && c->finalized && c->cfg.decoder == D2T_DEC_ATTN && (c->cfg.attn_coverage || c->cfg.attn_cell == D2T_ATTN_CELL_BAHDANAU) ? 1 : 0;
}

int d2t_decode_attn_beam_batch_ragged(d2t_ctx* c, const float* memory, int32_t N, const int32_t* T, int32_t beam_size,
                                      int64_t* seq_out, int32_t* len_out, float* score_out, float* alpha_out, d2t_stream stream) {
  DevGuard dg_(c);
  // d2t_decode_attn_beam_batch[_alpha] for N samples whose memories have DIFFERENT lengths, packed in `memory`: one step
  // loop, so the batch_max_length + 1 round trips are paid once for all sizes.  Everything is checked before anything is
  // enqueued; the context stays usable after a refusal.
  if (int rc = attn_beam_ragged_check(c, memory, N, T, beam_size, seq_out, len_out, score_out)) return rc;
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, alpha_out, "alpha")) return rc;
  if (c->attn_beam_device)
    return attn_beam_dev_impl(c, memory, N, 0, T, beam_size, seq_out, len_out, score_out, alpha_out, (hipStream_t)stream, false);
  return attn_beam_impl(c, memory, N, 0, T, beam_size, seq_out, len_out, score_out, alpha_out, (hipStream_t)stream);
}

// 1: this context has the device-side LSTM-attention beam search (wherever it has the search at all: the coverage and
// Bahdanau cells); 0: d2t_set_attn_beam_device(1) and d2t_decode_attn_beam_batch_submit refuse with D2T_ESTATE
int32_t d2t_decode_attn_supports_device_beam(const d2t_ctx* c) { return d2t_decode_attn_supports_ragged_beam(c); }

int d2t_set_attn_beam_device(d2t_ctx* c, int32_t on) {
  if (!c) return D2T_EINVAL;
  if (on) {
    if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
    if (int rc = attn_beam_check(c, 1)) return rc;
  }
  c->attn_beam_device = on ? 1 : 0;
  return D2T_OK;
}

int64_t d2t_decode_attn_beam_device_runs(const d2t_ctx* c) { return c ? (int64_t)c->attn_beam_dev_runs : 0; }

int d2t_decode_attn_beam_batch_submit(d2t_ctx* c, const float* memory, int32_t N, const int32_t* T, int32_t beam_size,
                                      int64_t* seq_dev, int32_t* len_dev, float* score_dev, float* alpha_dev, d2t_stream stream,
                                      int64_t* ticket_out) {
  DevGuard dg_(c);
  // the refusals of d2t_decode_attn_beam_batch_ragged, and outputs that the search's stream can write
  if (int rc = attn_beam_ragged_check(c, memory, N, T, beam_size, seq_dev, len_dev, score_dev)) return rc;
  const struct { const void* p; const char* what; } outs[] = {{seq_dev, "seq_dev"}, {len_dev, "len_dev"}, {score_dev, "score_dev"},
                                                              {alpha_dev, "alpha_dev"}};
  for (const auto& o : outs) {
    if (!o.p) continue;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, o.p) != hipSuccess || a.type != hipMemoryTypeDevice) {
      (void)hipGetLastError();
      return fail(c, D2T_EINVAL, "%s must be a device buffer (a submitted search writes its results on the engine's stream)", o.what);
    }
    if (int rc = check_dev_ptr(c, o.p, o.what)) return rc;
  }
  const int rc = attn_beam_dev_impl(c, memory, N, 0, T, beam_size, seq_dev, len_dev, score_dev, alpha_dev, (hipStream_t)stream, true);
  if (rc == D2T_OK && ticket_out) *ticket_out = c->last_ticket;
  return rc;
}

}  // extern "C"
