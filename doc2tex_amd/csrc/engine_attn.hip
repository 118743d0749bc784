// libd2t engine, LSTM-attention heads: the greedy decode (synchronous and pipelined) and the beam search of the C-ABI -- its
// host loop and the device-side loop beside it.  Host code only: the kernels are recurrent.hip's and attn_beam.hip's.
#include "engine_tfm.h"  // (engine_impl.h, carve.h; the captured-loop cache)

extern "C" {

namespace {
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
// The step pack of the beam search (one host -> device copy per step), its size padded to 16 bytes:
// tok i64 [cap] | scores [cap] | map [cap] | idx_h [cap] | idx_m [cap] | seg [N][3].  One layout for the device buffer and
// its pinned host mirror.
struct AttnBeamPack { char* base; size_t bytes; int64_t* tok; float* scores; int *map, *idx_h, *idx_m, *seg; };
static AttnBeamPack attn_beam_pack(Carver& cv, int N, int cap) {
  AttnBeamPack p;
  cv.align(8);
  const size_t at0 = cv.total();
  p.base = cv.here();
  p.tok = cv.take<int64_t>(cap);
  p.scores = cv.take<float>(cap);
  p.map = cv.take<int>(cap); p.idx_h = cv.take<int>(cap); p.idx_m = cv.take<int>(cap);
  p.seg = cv.take<int>(3 * (size_t)N);
  p.bytes = (cv.total() - at0 + 15) & ~(size_t)15;
  cv.at = at0 + p.bytes;
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

// Attention / AttentionV2.forward_beam for N samples in one step loop: rows = live hypotheses of all samples, each
// attending over its own sample's keys (row map).  The attention cell + LSTMCell + generator of every live hypothesis run
// as ONE launch per step (the greedy kernel in step mode, one block per hypothesis), log_softmax + top-k per sample
// segment on the device, the reference's bookkeeping per sample on the host -- including its quirks: step 0 ranks row 0
// only; the LSTM state follows prev_word_inds[incomplete] but the coverage memory only `incomplete`; if the last executed
// step completed nothing the first live sequence is returned; otherwise the best score/len sequence with the MAXIMUM raw
// score.
// Uniform (Ts == nullptr): memory [N][T][H].  Ragged (Ts = host [N], T unused): memory is packed, sample i's Ts[i] rows
// behind sample i-1's; ONE key projection over all packed rows (linear_any computes a row from that row alone, so each
// sample's projection is its uniform call's bit for bit), the per-sample tables [row0 | T] uploaded once in front of the
// loop, and the coverage memory, the alignment history and alpha_out [N][S][st_ld] on the row stride st_ld = the largest Tk.
// The bookkeeping below does not know which of the two it serves.  The caller has checked the lengths.
int attn_beam_impl(d2t_ctx* c, const float* memory, int N, int T, const int32_t* Ts, int beam_size, int64_t* seq_out,
                   int32_t* len_out, float* score_out, float* alpha_out, hipStream_t s) {
  const d2t_config& g = c->cfg;
  const int Hh = g.attn_hidden, S = g.batch_max_length + 1, V = g.vocab, cap = N * beam_size;
  const int key_off = g.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0;
  size_t mem_rows = (size_t)N * T;
  if (Ts) {
    mem_rows = 0; T = 0;
    for (int i = 0; i < N; ++i) { mem_rows += (size_t)Ts[i]; T = std::max(T, (int)Ts[i]); }
  }
  const int Tk = T - key_off;  // ragged: the largest, = st_ld
  int rc;
  // alignment maps (viz_attn): every step's launch writes its rows' alignments into its own slice of a history
  // [S][cap][Tk], kept apart from the workspace below; the chosen paths [N][S] and lengths [N] follow it
  float* d_hist = nullptr;
  int* d_path = nullptr;
  if (alpha_out) {
    const size_t hist_bytes = (size_t)S * cap * Tk * 4;
    if (hist_bytes > D2T_ATTN_MAP_BUDGET)
      return fail(c, D2T_EINVAL, "beam alignment history of %zu bytes (%d steps x %d samples x beam %d x %d keys x 4) exceeds the "
                  "%llu-byte budget: decode fewer samples per call", hist_bytes, S, N, beam_size, Tk, (unsigned long long)D2T_ATTN_MAP_BUDGET);
    if ((rc = ensure(c, &c->beam_hist, &c->beam_hist_cap, hist_bytes + ((size_t)N * (S + 1) + 16) * 4))) return rc;
    d_hist = c->beam_hist;
    d_path = reinterpret_cast<int*>(d_hist + (size_t)S * cap * Tk);
  }
  // the key projection lives in chain 0's workspace, like the synchronous greedy call's: behind that chain's last
  // asynchronous greedy decode (d2t_decode_attn_greedy_submit), which may still read it
  d2t_ctx::Chain& ch = c->chains[0];
  if (c->ev_done_valid[0]) HIPCHK(c, hipStreamWaitEvent(s, c->ev_done[0], 0));
  if ((rc = ensure(c, &ch.dws, &ch.dws_cap, (mem_rows * Hh + 16) * 4))) return rc;
  float* kp = ch.dws;
  // workspace: logits [cap][V] | topv [cap] | topi [cap] (one device -> host copy per step) | h_in c_in h_out c_out [cap][H]
  //            | mem_in mem_out [cap][Tk] | end_step [cap] | dummy tokens i64 [cap] | step pack (one host -> device copy per
  //            step): tok i64 [cap] | scores [cap] | map [cap] | idx_h [cap] | idx_m [cap] | seg [N][3]
  //            | ragged: the per-sample tables row0 [N] | T [N]
  float *d_logits, *d_topv, *st[6];  // st: h_in c_in h_out c_out mem_in mem_out
  int *d_topi, *d_end, *d_tab;
  int64_t* d_dummy;
  AttnBeamPack dp, hpk;  // the step pack on the device and in the pinned mirror
  auto ws_carve = [&](Carver cv) {
    d_logits = cv.take<float>((size_t)cap * V);
    d_topv = cv.take<float>(cap);
    d_topi = cv.take<int>(cap);
    for (int i = 0; i < 6; ++i) st[i] = cv.take<float>((size_t)cap * (i < 4 ? Hh : Tk));
    d_end = cv.take<int>(cap);
    d_dummy = cv.take<int64_t>(cap, 16);
    dp = attn_beam_pack(cv, N, cap);
    d_tab = cv.take<int>(Ts ? 2 * (size_t)N : 0);
    return cv.total() + 64;
  };
  if ((rc = ensure(c, &c->beam_ws, &c->beam_ws_cap, ws_carve(Carver())))) return rc;
  ws_carve(Carver(c->beam_ws));
  // pinned host mirror: the step pack | topv [cap] | topi [cap] | ragged: the tables
  float* h_topv;
  int *h_topi, *h_tab;
  auto mirror_carve = [&](Carver cv) {
    hpk = attn_beam_pack(cv, N, cap);
    h_topv = cv.take<float>(cap);
    h_topi = cv.take<int>(cap);
    h_tab = cv.take<int>(Ts ? 2 * (size_t)N : 0);
    return cv.total();
  };
  if ((rc = ensure_host_beam(c, mirror_carve(Carver())))) return rc;
  mirror_carve(Carver(c->h_beam));
  char *const d_pack = dp.base, *const hp = hpk.base;
  const size_t pack_bytes = dp.bytes;
  int64_t *const d_tok = dp.tok, *const h_tok = hpk.tok;
  float *const d_scores = dp.scores, *const h_scores = hpk.scores;
  int *const d_map = dp.map, *const d_idxh = dp.idx_h, *const d_idxm = dp.idx_m, *const d_seg = dp.seg;
  int *const h_map = hpk.map, *const h_idxh = hpk.idx_h, *const h_idxm = hpk.idx_m, *const h_seg = hpk.seg;
  HIPCHK(c, linear_any(nullptr, s, memory, c->attn.key, nullptr, kp, (int)mem_rows, ACT_NONE));
  AttnDecP p = attn_dec_params(c, memory, T, kp);
  p.probs = d_logits; p.tokens = d_dummy; p.end_step = d_end;
  p.S = 1; p.coverage = 1;
  p.step_mode = 1;
  p.st_h_in = st[0]; p.st_c_in = st[1]; p.st_mem_in = st[4];
  p.st_h_out = st[2]; p.st_c_out = st[3]; p.st_mem_out = st[5];
  p.tok_in = d_tok; p.row_sample = d_map;
  if (Ts) {  // (the previous search has synchronised: the mirror is idle)
    d2t_ragged_beam_tables(N, Ts, h_tab, h_tab + N);
    HIPCHK(c, hipMemcpyAsync(d_tab, h_tab, 2 * (size_t)N * 4, hipMemcpyHostToDevice, s));
    p.smp_row0 = d_tab; p.smp_T = d_tab + N; p.st_ld = Tk;
  }

  struct Smp {
    std::vector<std::vector<int64_t>> seqs, complete;
    std::vector<std::vector<int>> paths, cpaths;  // maps only: per hypothesis, the launch row of its parent at every step
    std::vector<float> live, cscores;
    int k;
    bool last_completed = false, finished = false;
  };
  std::vector<Smp> sm((size_t)N);
  for (auto& x : sm) {
    x.seqs.assign((size_t)beam_size, std::vector<int64_t>{0});  // each starts with [GO] = 0
    x.live.assign((size_t)beam_size, 0.f);
    x.k = beam_size;
    if (alpha_out) x.paths.assign((size_t)beam_size, std::vector<int>{});
  }
  // the rows of a step in sample order: segments, scores and row map into the pack; returns the row count
  auto stage = [&](int step) {
    int rows = 0;
    for (int i = 0; i < N; ++i) {
      Smp& x = sm[i];
      const int M = x.finished ? 0 : (int)x.seqs.size();
      // step 0: all rows of a sample are identical and the reference ranks its row 0 only (seq2seq.py:145-146)
      h_seg[3 * i] = rows; h_seg[3 * i + 1] = M ? (step == 0 ? 1 : M) : 0; h_seg[3 * i + 2] = x.finished ? 0 : x.k;
      for (int j = 0; j < M; ++j) { h_scores[rows + j] = x.live[j]; h_map[rows + j] = i; }
      rows += M;
    }
    return rows;
  };
  int rows = stage(0);
  HIPCHK(c, hipMemcpyAsync(d_pack, hp, pack_bytes, hipMemcpyHostToDevice, s));
  for (int step = 0; step < S; ++step) {
    p.B = rows; p.first = step == 0;
    if (d_hist) p.sv_alpha = d_hist + (size_t)step * cap * Tk;
    HIPCHK(c, launch_attn_decode(p, s));
    HIPCHK(c, launch_beam_topk_batch(d_logits, d_scores, d_seg, N, V, beam_size, d_topv, d_topi, s));
    HIPCHK(c, hipMemcpyAsync(h_topv, d_topv, 2 * (size_t)cap * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    int nrows = 0;
    for (int i = 0; i < N; ++i) {
      Smp& x = sm[i];
      if (x.finished) continue;
      const int off = h_seg[3 * i];
      std::vector<std::vector<int64_t>> nseqs;
      std::vector<std::vector<int>> npaths;
      std::vector<float> nscores;
      x.last_completed = false;
      for (int r = 0; r < x.k; ++r) {
        const int idx = h_topi[(size_t)i * beam_size + r], prev = idx / V, word = idx % V;
        std::vector<int64_t> sq = x.seqs[prev];
        sq.push_back(word);
        std::vector<int> pa;
        if (alpha_out) {  // the step's alignment row of this hypothesis = its parent's row: seqs_alpha[prev_word_inds]
          pa = x.paths[prev];
          pa.push_back(off + prev);
        }
        if (word == 1) {  // [s] (attn_converter.py:8)
          x.complete.push_back(std::move(sq));
          if (alpha_out) x.cpaths.push_back(std::move(pa));
          x.cscores.push_back(h_topv[(size_t)i * beam_size + r]);
          x.last_completed = true;
        } else {
          h_idxh[nrows] = off + prev;  // LSTM state: hidden[prev_word_inds[incomplete]]
          h_idxm[nrows] = off + r;     // coverage memory: (alpha_cum + alpha)[incomplete]
          h_tok[nrows] = word;
          ++nrows;
          nseqs.push_back(std::move(sq));
          if (alpha_out) npaths.push_back(std::move(pa));
          nscores.push_back(h_topv[(size_t)i * beam_size + r]);
        }
      }
      x.seqs.swap(nseqs);
      x.paths.swap(npaths);
      x.live.swap(nscores);
      x.k = (int)x.seqs.size();
      if (x.k == 0) x.finished = true;
    }
    if (!nrows || step + 1 == S) break;
    rows = stage(step + 1);  // == nrows: the survivors, in the order of their gather indices
    HIPCHK(c, hipMemcpyAsync(d_pack, hp, pack_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_gather_rows(st[2], st[0], d_idxh, rows, Hh, s));
    HIPCHK(c, launch_gather_rows(st[3], st[1], d_idxh, rows, Hh, s));
    HIPCHK(c, launch_gather_rows(st[5], st[4], d_idxm, rows, Tk, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  std::vector<int> h_path;  // maps: [N][S] chosen paths | [N] lengths, uploaded in one copy
  if (alpha_out) h_path.assign((size_t)N * (S + 1), 0);
  for (int i = 0; i < N; ++i) {
    Smp& x = sm[i];
    std::vector<int64_t> out;
    const std::vector<int>* path = nullptr;
    float score;
    if (!x.last_completed) {  // seq2seq.py:209-216
      out.assign(x.seqs[0].begin() + 1, x.seqs[0].end());
      score = x.live[0];
      if (alpha_out) path = &x.paths[0];
    } else {
      size_t best = 0;
      for (size_t j = 1; j < x.complete.size(); ++j)
        if ((double)x.cscores[j] / (double)x.complete[j].size() > (double)x.cscores[best] / (double)x.complete[best].size()) best = j;
      out.assign(x.complete[best].begin() + 1, x.complete[best].end());
      score = *std::max_element(x.cscores.begin(), x.cscores.end());
      if (alpha_out) path = &x.cpaths[best];
    }
    const int n = (int)std::min<size_t>(out.size(), (size_t)S);
    for (int j = 0; j < n; ++j) seq_out[(size_t)i * S + j] = out[j];
    len_out[i] = n;
    score_out[i] = score;
    if (alpha_out) {  // one path entry per emitted token; entries index rows of that step's launch (< cap)
      const int m = (int)std::min<size_t>(path->size(), (size_t)n);
      for (int j = 0; j < m; ++j) h_path[(size_t)i * S + j] = (*path)[j];
      h_path[(size_t)N * S + i] = m;
    }
  }
  if (alpha_out) {  // seqs_alpha[best][1:] of every sample: one upload, one gather over all samples
    HIPCHK(c, hipMemcpyAsync(d_path, h_path.data(), h_path.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_attn_alpha_gather(d_hist, d_path, d_path + (size_t)N * S, alpha_out, N, S, cap, Tk, s));
    HIPCHK(c, hipStreamSynchronize(s));  // h_path is pageable and local
  }
  return D2T_OK;
}

// ---- the device-side loop ----
// Its workspace (per decode chain): logits [cap][V] | topv [cap] | topi [cap] | h_in c_in h_out c_out [cap][H] | mem_in mem_out
// [cap][ld] | end_step [cap] | dummy tokens i64 [cap] | the per-sample tables row0 [N] | T [N] | the record (kernels.h
// AttnBeamDev) | the result block seq i64 [N][S] | len [N] | score [N] | ctrl [4] (one device -> host copy at the end of a
// synchronous search), each from a 16-byte boundary.  A function of N, beam, V, S and ld alone: no memory length moves it.
struct AttnBeamDevWs {
  float *logits, *topv, *st[6];
  int *topi, *end, *tab;
  int64_t* dummy;
  AttnBeamDev rec;
  char* res; size_t res_bytes;
  int64_t* r_seq; int* r_len; float* r_score;
};
size_t attn_beam_dev_carve(Carver cv, int Hh, int ld, AttnBeamDevWs* w) {
  AttnBeamDev& r = w->rec;
  const size_t cap = (size_t)r.cap, N = (size_t)r.N, nb = N * r.beam;
  w->logits = cv.take<float>(cap * r.V, 16);
  w->topv = cv.take<float>(cap, 16);
  w->topi = cv.take<int>(cap, 16);
  for (int i = 0; i < 6; ++i) w->st[i] = cv.take<float>(cap * (i < 4 ? Hh : ld), 16);
  w->end = cv.take<int>(cap, 16);
  w->dummy = cv.take<int64_t>(cap, 16);
  w->tab = cv.take<int>(2 * N, 16);
  r.tok = cv.take<int64_t>(cap, 16);
  r.scores = cv.take<float>(cap, 16);
  r.map = cv.take<int>(cap, 16); r.idx_h = cv.take<int>(cap, 16); r.idx_m = cv.take<int>(cap, 16);
  r.seg = cv.take<int>(3 * N, 16);
  r.comp_n = cv.take<int>(N, 16); r.fin = cv.take<int>(N, 16); r.last_completed = cv.take<int>(N, 16);
  r.comp_t = cv.take<int>(nb, 16); r.comp_par = cv.take<int>(nb, 16); r.comp_score = cv.take<float>(nb, 16);
  r.hist_par = cv.take<int>((size_t)r.S * cap, 16); r.hist_tok = cv.take<int>((size_t)r.S * cap, 16);
  cv.align(16);
  w->res = cv.here();
  w->r_seq = cv.take<int64_t>(N * r.S, 16);
  w->r_len = cv.take<int>(N);
  w->r_score = cv.take<float>(N);
  r.ctrl = cv.take<int>(4);
  w->res_bytes = (size_t)(cv.here() - w->res);
  r.topv = w->topv; r.topi = w->topi;
  return cv.total() + 64;
}
constexpr int ATTN_BEAM_LD_QUANTUM = 256;  // the row stride of state and history: the largest Tk rounded up to this

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
  const int key_off = g.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0;
  if (N > ATTN_BEAM_MAX_N)
    return fail(c, D2T_EINVAL, "the device-side beam search takes 1 to %d samples per call, got %d", ATTN_BEAM_MAX_N, N);
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  if (int rc = check_dev_ptr(c, alpha_out, "alpha")) return rc;
  std::vector<int32_t> uniform;
  if (!Ts) { uniform.assign((size_t)N, T); Ts = uniform.data(); }
  size_t mem_rows = 0;
  T = 0;
  for (int i = 0; i < N; ++i) { mem_rows += (size_t)Ts[i]; T = std::max(T, (int)Ts[i]); }
  const int Tk = T - key_off;  // the largest
  int ld = (Tk + ATTN_BEAM_LD_QUANTUM - 1) / ATTN_BEAM_LD_QUANTUM * ATTN_BEAM_LD_QUANTUM;
  if (alpha_out) {
    const size_t hist_bytes = (size_t)S * cap * Tk * 4;
    if (hist_bytes > D2T_ATTN_MAP_BUDGET)
      return fail(c, D2T_EINVAL, "beam alignment history of %zu bytes (%d steps x %d samples x beam %d x %d keys x 4) exceeds the "
                  "%llu-byte budget: decode fewer samples per call", hist_bytes, S, N, beam_size, Tk, (unsigned long long)D2T_ATTN_MAP_BUDGET);
    if ((size_t)S * cap * ld * 4 > D2T_ATTN_MAP_BUDGET) ld = Tk;
  }
  // ---- nothing is refused below this line ----
  const int chain = async ? (int)(c->decode_seq++ % (unsigned)c->n_chains) : 0;
  d2t_ctx::Chain& ch = c->chains[chain];
  hipStream_t s = ch.stream;
  int rc;
  AttnBeamDevWs ws{};
  ws.rec.N = N; ws.rec.beam = beam_size; ws.rec.cap = cap; ws.rec.V = V; ws.rec.S = S; ws.rec.end_token = 1;  // attn_converter.py:8
  if ((rc = ensure(c, &ch.abeam_ws, &ch.abeam_ws_cap, attn_beam_dev_carve(Carver(), Hh, ld, &ws)))) return rc;
  attn_beam_dev_carve(Carver(ch.abeam_ws), Hh, ld, &ws);
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
  AttnDecP p = attn_dec_params(c, ch.abeam_mem, T, kp);
  p.probs = ws.logits; p.tokens = ws.dummy; p.end_step = ws.end;
  p.B = cap; p.S = 1; p.coverage = 1;
  p.step_mode = 1;
  p.st_h_in = ws.st[0]; p.st_c_in = ws.st[1]; p.st_mem_in = ws.st[4];
  p.st_h_out = ws.st[2]; p.st_c_out = ws.st[3]; p.st_mem_out = ws.st[5];
  p.tok_in = b.tok; p.row_sample = b.map;
  p.smp_row0 = ws.tab; p.smp_T = ws.tab + N; p.st_ld = ld;
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
    for (int j = 0; j < n; ++j) seq_out[(size_t)i * S + j] = h_seq[(size_t)i * S + j];
    len_out[i] = n;
    score_out[i] = h_score[i];
  }
  return D2T_OK;
}
}  // namespace

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
  if (!c || !memory || !T || !seq_out || !len_out || !score_out) return fail(c, D2T_EINVAL, "bad argument");
  if (int rc = attn_beam_check(c, beam_size)) return rc;
  if (N < 1 || N > ATTN_BEAM_MAX_N)
    return fail(c, D2T_EINVAL, "ragged beam search takes 1 to %d samples per call, got %d", ATTN_BEAM_MAX_N, N);
  const int key_off = c->cfg.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0;
  for (int i = 0; i < N; ++i)
    if (T[i] - key_off < 1 || T[i] - key_off > memory_cap(c))
      return fail(c, D2T_EINVAL, "sample %d has memory length %d, supported are %d to %d", i, T[i], 1 + key_off, memory_cap(c) + key_off);
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
  if (!c || !memory || !T || !seq_dev || !len_dev || !score_dev) return fail(c, D2T_EINVAL, "bad argument");
  if (int rc = attn_beam_check(c, beam_size)) return rc;
  if (N < 1 || N > ATTN_BEAM_MAX_N)
    return fail(c, D2T_EINVAL, "ragged beam search takes 1 to %d samples per call, got %d", ATTN_BEAM_MAX_N, N);
  const int key_off = c->cfg.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0;
  for (int i = 0; i < N; ++i)
    if (T[i] - key_off < 1 || T[i] - key_off > memory_cap(c))
      return fail(c, D2T_EINVAL, "sample %d has memory length %d, supported are %d to %d", i, T[i], 1 + key_off, memory_cap(c) + key_off);
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
