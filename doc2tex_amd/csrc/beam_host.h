// Beam-search bookkeeping of the TFM head on the host (tools/beam.py:38-140): the record both step loops keep, Beam.advance
// on host arrays, and the final selection.  The record is the one the device-side loop fills (kernels.h BeamDev, same member
// names): the live rows of the coming step, the completed set of every sample, and a (parent row, token) history record per
// step that is walked back once at the end.  No HIP and no context -- plain pointers, int and float -- so that
// tools/probe/beam_host_check.cpp exercises it under a sanitizer without a GPU.
#pragma once
#include "carve.h"

struct BeamRec {
  // live hypothesis rows of the coming step, compact and in sample order
  int64_t* tok;       // [cap] last token of a row
  float* scores;      // [cap]
  int* map;           // [cap] sample of a row
  int* prev;          // [cap] parent row (previous step's row order)
  int* seg;           // [N][3] first row, live rows, candidates wanted (beam - completed)
  // bookkeeping
  int* ctrl;          // [0] step, [1] live rows, [2] stop-at step (0 = none), [3] steps run
  int* comp_n;        // [N] completed hypotheses
  int* fin;           // [N] sample finished (beam completed hypotheses: Beam.done)
  int* comp_t;        // [N][beam] step at which a hypothesis completed
  int* comp_par;      // [N][beam] its parent row (that step's row order)
  float* comp_score;  // [N][beam]
  int* hist_par;      // [S][cap] parent row of the hypothesis a step created at row r (the next step's row order)
  int* hist_tok;      // [S][cap] its token
  int N, beam, cap, V, S, end_token;
};

// ---- layouts (r.N, r.beam, r.cap, r.S set beforehand) ----
// ctrl [8] | comp_n, fin [N] | comp_t, comp_par, comp_score [N][beam] | hist_par, hist_tok [S][cap], each from a 16-byte boundary
inline void beam_book_carve(Carver& cv, BeamRec& r) {
  r.ctrl = cv.take<int>(8, 16);
  r.comp_n = cv.take<int>(r.N, 16);
  r.fin = cv.take<int>(r.N, 16);
  r.comp_t = cv.take<int>(r.cap, 16);
  r.comp_par = cv.take<int>(r.cap, 16);
  r.comp_score = cv.take<float>(r.cap, 16);
  r.hist_par = cv.take<int>((size_t)r.S * r.cap, 16);
  r.hist_tok = cv.take<int>((size_t)r.S * r.cap, 16);
  cv.align(16);
}
// what the final selection reads: scores [cap] | seg [N][3] | the bookkeeping.  The device-side loop carves this block out of
// its workspace and, from the base of the pinned copy, the host's view of it.
inline void beam_result_carve(Carver& cv, BeamRec& r) {
  r.scores = cv.take<float>(r.cap, 16);
  r.seg = cv.take<int>(3 * (size_t)r.N, 16);
  beam_book_carve(cv, r);
}
// the host-side loop's step pack (one host -> device copy per step), padded to 16 bytes:
// tok [cap] i64 | scores [cap] | map [cap] | prev [cap] | seg [N][3] | step [4]; returns the step word
inline int* beam_pack_carve(Carver& cv, BeamRec& r) {
  r.tok = cv.take<int64_t>(r.cap, 16);
  r.scores = cv.take<float>(r.cap);
  r.map = cv.take<int>(r.cap);
  r.prev = cv.take<int>(r.cap);
  r.seg = cv.take<int>(3 * (size_t)r.N);
  int* step = cv.take<int>(4);
  cv.align(16);
  return step;
}

// Every sample starts with one hypothesis [GO] of score 0 (what beam_dev_init_kernel writes).
inline void beam_host_init(BeamRec& r, int64_t go_token) {
  for (int i = 0; i < r.N; ++i) {
    r.seg[3 * i] = i; r.seg[3 * i + 1] = 1; r.seg[3 * i + 2] = r.beam;
    r.tok[i] = go_token; r.scores[i] = 0.f; r.map[i] = i; r.prev[i] = i;
    r.comp_n[i] = 0; r.fin[i] = 0;
  }
  r.ctrl[0] = 0; r.ctrl[1] = r.N; r.ctrl[2] = 0; r.ctrl[3] = 0;
}

// Beam.advance (tools/beam.py:68-105) for every sample after the step's per-sample top-k (topv / topi [N][beam], flat index
// = row in the sample * V + word), as beam_dev_advance_kernel does it: a candidate ending in [s] joins the sample's completed
// set (step, parent row, score), the others become the next step's rows -- compact, in sample order, their parents in prev
// and in the history; a sample with `beam` completed hypotheses is finished and its rows drop out.  Returns the live rows.
inline int beam_host_advance(BeamRec& r, const float* topv, const int* topi) {
  constexpr int KMAX = 16;  // beam <= 16
  const int t = r.ctrl[0];
  if (r.ctrl[2] && t >= r.ctrl[2]) return 0;  // every sample finished at an earlier step
  int run = 0;
  for (int i = 0; i < r.N; ++i) {
    int newM = 0, n_par[KMAX], n_word[KMAX];
    float n_val[KMAX];
    if (!r.fin[i] && r.seg[3 * i + 1] > 0) {
      const int off = r.seg[3 * i], live = r.seg[3 * i + 2];
      int cn = r.comp_n[i];
      for (int k = 0; k < live; ++k) {
        const size_t at = (size_t)i * r.beam + k;
        const int idx = topi[at], prev = idx / r.V, word = idx - prev * r.V;
        if (word == r.end_token) {
          r.comp_t[(size_t)i * r.beam + cn] = t; r.comp_par[(size_t)i * r.beam + cn] = off + prev; r.comp_score[(size_t)i * r.beam + cn] = topv[at];
          ++cn;
        } else {
          n_par[newM] = off + prev; n_word[newM] = word; n_val[newM] = topv[at];
          ++newM;
        }
      }
      r.comp_n[i] = cn;
      if (cn == r.beam) { r.fin[i] = 1; newM = 0; }
    }
    for (int j = 0; j < newM; ++j) {
      const int row = run + j;
      r.tok[row] = n_word[j]; r.scores[row] = n_val[j]; r.map[row] = i; r.prev[row] = n_par[j];
      r.hist_par[(size_t)t * r.cap + row] = n_par[j];
      r.hist_tok[(size_t)t * r.cap + row] = n_word[j];
    }
    r.seg[3 * i] = run; r.seg[3 * i + 1] = newM; r.seg[3 * i + 2] = r.fin[i] ? 0 : r.beam - r.comp_n[i];
    run += newM;
  }
  r.ctrl[0] = t + 1; r.ctrl[1] = run; r.ctrl[3] = t + 1;
  if (run == 0) r.ctrl[2] = t + 1;  // nothing left to extend
  return run;
}

// Sample i's result (Beam.get_best / set_hypothesis, tools/beam.py:107-140) into out[0 .. *len_out): the completed hypothesis
// with the best score over length (compared in double; the first wins ties), a hypothesis completed at step t having t + 1
// tokens; if nothing completed, the first live hypothesis padded to S = max_seq_len + 1 (no live row either: all PAD, score
// 0).  Its tokens are read back through the (parent, token) history.
inline void beam_select(const BeamRec& r, int i, int64_t pad_token, int64_t* out, int* len_out, float* score_out) {
  const int nc = r.comp_n[i];
  const int* ct = r.comp_t + (size_t)i * r.beam;
  const float* cs = r.comp_score + (size_t)i * r.beam;
  int row, last_step, n;  // the hypothesis ends with the history record (last_step, row); n tokens are returned
  float score;
  if (nc > 0) {
    int best = 0;
    for (int j = 1; j < nc; ++j)
      if ((double)cs[j] / (double)(ct[j] + 1) > (double)cs[best] / (double)(ct[best] + 1)) best = j;
    const int t = ct[best];
    n = t + 1 < r.S ? t + 1 : r.S;
    for (int j = 0; j < n; ++j) out[j] = pad_token;
    if (t < n) out[t] = r.end_token;
    row = r.comp_par[(size_t)i * r.beam + best];
    last_step = t - 1;
    score = cs[best];
  } else {
    n = r.S;
    for (int j = 0; j < n; ++j) out[j] = pad_token;
    if (r.seg[3 * i + 1] > 0) { row = r.seg[3 * i]; last_step = r.ctrl[3] - 1; score = r.scores[row]; }
    else { row = -1; last_step = -1; score = 0.f; }
  }
  for (int p = last_step; p >= 0 && row >= 0; --p) {
    if (p < n) out[p] = r.hist_tok[(size_t)p * r.cap + row];
    row = r.hist_par[(size_t)p * r.cap + row];
  }
  *len_out = n;
  *score_out = score;
}
