// Beam-search bookkeeping of the LSTM-attention heads (Attention.forward_beam, prediction_head/seq2seq.py:83-222;
// AttentionV2.forward_beam, seq2seq_v2.py:12-174): the record both step loops of engine_attn.hip keep, its layouts, and the
// reference's rules on it as host functions.  The kernels of attn_beam.hip state the same rules over the same record for the
// device-side loop; tests/attn_beam_refs.py holds both to one array-for-array description.  What differs from the TFM head's
// record (beam_host.h) is the reference: step 0 ranks row 0 of a sample's `beam` identical rows, every completion lowers the
// sample's k (so completions never exceed beam), the LSTM state of a survivor follows its parent row (idx_h) but its coverage
// memory follows its candidate rank (idx_m), and the final pick depends on whether the sample's last step completed anything.
// No HIP and no context -- plain pointers, int and float -- so that tools/probe/attn_beam_host_check.cpp exercises it under a
// sanitizer without a GPU.
#pragma once
#include <cmath>

#include "carve.h"

struct AttnBeamDev {
  int* ctrl;            // [0] step, [1] live rows, [2] stop-at step (0 = none), [3] steps run
  // live hypothesis rows of the coming step, compact and in sample order
  int64_t* tok;         // [cap] input token of a row
  float* scores;        // [cap]
  int* map;             // [cap] sample of a row
  int* idx_h;           // [cap] row of the step just run whose LSTM state the new row resumes (its parent)
  int* idx_m;           // [cap] row of the step just run whose coverage memory it resumes (first row of the sample + rank)
  int* seg;             // [N][3] first row, rows ranked, candidates wanted (k)
  // bookkeeping
  int* comp_n;          // [N] completed hypotheses
  int* fin;             // [N] sample finished (k == 0)
  int* last_completed;  // [N] the last step that processed the sample completed a hypothesis
  int* comp_t;          // [N][beam] step at which a hypothesis completed
  int* comp_par;        // [N][beam] its parent row (that step's row order)
  float* comp_score;    // [N][beam]
  int* hist_par;        // [S][cap] parent row of the hypothesis a step created at row r (the next step's row order)
  int* hist_tok;        // [S][cap] its token
  const float* topv; const int* topi;   // [N][beam] candidates of the step (launch_beam_topk_batch): the kernels read them here
  int N, beam, cap, V, S, end_token;
};

// ---- layouts (r.N, r.beam, r.cap, r.S set beforehand), every array from a 16-byte boundary ----
// The live rows: tok i64 [cap] | scores | map | idx_h | idx_m [cap] | seg [N][3].  What the host loop uploads in one copy per
// step -- the same function over the device buffer and over the pinned mirror, so the two views cannot differ.
inline void attn_beam_rows_carve(Carver& cv, AttnBeamDev& r) {
  r.tok = cv.take<int64_t>(r.cap, 16);
  r.scores = cv.take<float>(r.cap, 16);
  r.map = cv.take<int>(r.cap, 16);
  r.idx_h = cv.take<int>(r.cap, 16);
  r.idx_m = cv.take<int>(r.cap, 16);
  r.seg = cv.take<int>(3 * (size_t)r.N, 16);
  cv.align(16);
}
// The bookkeeping: ctrl [4] | comp_n, fin, last_completed [N] | comp_t, comp_par, comp_score [N][beam] | hist_par, hist_tok [S][cap]
inline void attn_beam_book_carve(Carver& cv, AttnBeamDev& r) {
  const size_t N = (size_t)r.N, nb = N * r.beam, hist = (size_t)r.S * r.cap;
  r.ctrl = cv.take<int>(4, 16);
  r.comp_n = cv.take<int>(N, 16);
  r.fin = cv.take<int>(N, 16);
  r.last_completed = cv.take<int>(N, 16);
  r.comp_t = cv.take<int>(nb, 16);
  r.comp_par = cv.take<int>(nb, 16);
  r.comp_score = cv.take<float>(nb, 16);
  r.hist_par = cv.take<int>(hist, 16);
  r.hist_tok = cv.take<int>(hist, 16);
  cv.align(16);
}

// Step 0 (what attn_beam_dev_init_kernel writes): `beam` identical rows per sample from the token [GO] with score 0, of which
// the reference ranks row 0 only (seq2seq.py:145-146): seg = {i * beam, 1, beam}.
inline void attn_beam_host_init(AttnBeamDev& r, int64_t go_token) {
  for (int i = 0; i < r.N; ++i) {
    r.seg[3 * i] = i * r.beam; r.seg[3 * i + 1] = 1; r.seg[3 * i + 2] = r.beam;
    r.comp_n[i] = 0; r.fin[i] = 0; r.last_completed[i] = 0;
  }
  for (int row = 0; row < r.N * r.beam; ++row) {
    r.tok[row] = go_token; r.scores[row] = 0.f; r.map[row] = row / r.beam; r.idx_h[row] = row; r.idx_m[row] = row;
  }
  r.ctrl[0] = 0; r.ctrl[1] = r.N * r.beam; r.ctrl[2] = 0; r.ctrl[3] = 0;
}

// One step of the reference's bookkeeping for every sample after the per-sample top-k (topv / topi [N][beam], flat index = row
// in the sample * V + word), array for array what attn_beam_dev_advance_kernel writes.  A candidate ending in [s] joins the
// sample's completed set (step, parent row, score) and nothing else; a survivor becomes a row of the next step -- compact, in
// sample order -- with idx_h = parent row (the LSTM state follows prev_word_inds[incomplete]), idx_m = first row + rank (the
// coverage memory follows `incomplete` alone: the reference's quirk), its token, score and sample, and its (parent, token)
// record in the history.  A sample whose k reaches 0 is finished and keeps its seg = {., 0, 0} and its last_completed, which
// is rewritten only for the samples the step processed.  No survivor anywhere sets the stop step, behind which a call does
// nothing.  Returns the live rows.
inline int attn_beam_host_advance(AttnBeamDev& r, const float* topv, const int* topi) {
  const int t = r.ctrl[0];
  if (r.ctrl[2] && t >= r.ctrl[2]) return 0;  // every sample finished at an earlier step
  int run = 0;
  for (int i = 0; i < r.N; ++i) {
    const int off = r.seg[3 * i], k = r.seg[3 * i + 2], first = run;
    if (r.fin[i] || k <= 0) continue;
    int cn = r.comp_n[i];
    for (int q = 0; q < k; ++q) {
      const size_t at = (size_t)i * r.beam + q;
      const int idx = topi[at], prev = idx / r.V, word = idx - prev * r.V;
      if (word == r.end_token) {
        if (cn < r.beam) {  // (always: every completion lowers k)
          const size_t c = (size_t)i * r.beam + cn;
          r.comp_t[c] = t; r.comp_par[c] = off + prev; r.comp_score[c] = topv[at];
          ++cn;
        }
      } else {
        const int row = run++;
        r.idx_h[row] = off + prev;
        r.idx_m[row] = off + q;
        r.tok[row] = word; r.scores[row] = topv[at]; r.map[row] = i;
        r.hist_par[(size_t)t * r.cap + row] = off + prev;
        r.hist_tok[(size_t)t * r.cap + row] = word;
      }
    }
    const int newM = run - first;
    r.last_completed[i] = newM < k;
    r.comp_n[i] = cn;
    r.seg[3 * i] = first; r.seg[3 * i + 1] = newM; r.seg[3 * i + 2] = newM;
    if (newM == 0) r.fin[i] = 1;
  }
  r.ctrl[0] = t + 1; r.ctrl[1] = run; r.ctrl[3] = t + 1;
  if (run == 0) r.ctrl[2] = t + 1;  // nothing left to extend
  return run;
}

// The final pick of every sample (seq2seq.py:209-222), what attn_beam_dev_finish_kernel writes: seq [N][S] (zeros behind the
// length), len [N], score [N], and with path / plen (both or neither) the launch row of every step path [N][S] (written up to
// the length) and plen [N].  The last step that processed the sample completed nothing: its first live hypothesis and that
// hypothesis's score.  Otherwise the completed hypothesis with the largest score / length -- in double, the first maximum, a
// hypothesis completed at step t counting t + 2 tokens with [GO] -- with the MAXIMUM raw completed score.  The tokens and
// rows come from walking the history back.
inline void attn_beam_host_finish(const AttnBeamDev& r, int64_t* seq, int* len, float* score, int* path, int* plen) {
  for (int i = 0; i < r.N; ++i) {
    int64_t* out = seq + (size_t)i * r.S;
    int* pa = path ? path + (size_t)i * r.S : nullptr;
    int t = -1, row = 0, n = 0;
    float sc = 0.f;
    if (!r.last_completed[i]) {
      if (r.seg[3 * i + 1] > 0 && r.ctrl[3] > 0) { t = r.ctrl[3] - 1; row = r.seg[3 * i]; sc = r.scores[row]; n = t + 1; }
    } else if (r.comp_n[i] >= 1) {  // (always, after a step that completed something)
      const float* cs = r.comp_score + (size_t)i * r.beam;
      const int* ct = r.comp_t + (size_t)i * r.beam;
      int best = 0;
      sc = cs[0];
      for (int j = 1; j < r.comp_n[i]; ++j) {
        if ((double)cs[j] / (double)(ct[j] + 2) > (double)cs[best] / (double)(ct[best] + 2)) best = j;
        sc = fmaxf(sc, cs[j]);
      }
      t = ct[best];
      n = t + 1;
      row = r.comp_par[(size_t)i * r.beam + best];
      out[t] = r.end_token;
      if (pa) pa[t] = row;
      --t;
    }
    for (; t >= 0; --t) {
      out[t] = r.hist_tok[(size_t)t * r.cap + row];
      row = r.hist_par[(size_t)t * r.cap + row];
      if (pa) pa[t] = row;
    }
    for (int j = n; j < r.S; ++j) out[j] = 0;
    len[i] = n;
    score[i] = sc;
    if (plen) plen[i] = n;
  }
}
