// The LSTM-attention beam search's host bookkeeping (csrc/attn_beam_host.h: attn_beam_host_init, attn_beam_host_advance,
// attn_beam_host_finish) driven with scripted per-step top-k results and compared with sequences, lengths, scores and launch-row
// paths worked out by hand below.  Every array of the record is its own exact-size allocation, so AddressSanitizer sees any
// index past an end.  No GPU, no HIP.
//   cd tools/probe && g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I../../doc2tex_amd/csrc attn_beam_host_check.cpp -o attn_beam_host_check
//   ./attn_beam_host_check        (prints one line per case; exit status 1 on any mismatch)
#include "attn_beam_host.h"

#include <cstdio>
#include <vector>

namespace {
constexpr int GO = 0, END = 1;  // attn_converter.py:8
constexpr int V = 6;
int failures = 0;

struct Rec {
  std::vector<int64_t> tok;
  std::vector<float> scores, comp_score;
  std::vector<int> map, idx_h, idx_m, seg, ctrl, comp_n, fin, last_completed, comp_t, comp_par, hist_par, hist_tok;
  AttnBeamDev r{};
  Rec(int N, int beam, int S) {
    const int cap = N * beam;
    tok.assign(cap, -7); scores.assign(cap, -7.f); map.assign(cap, -7); idx_h.assign(cap, -7); idx_m.assign(cap, -7);
    seg.assign(3 * N, -7); ctrl.assign(4, -7); comp_n.assign(N, -7); fin.assign(N, -7); last_completed.assign(N, -7);
    comp_t.assign(cap, -7); comp_par.assign(cap, -7); comp_score.assign(cap, -7.f);
    hist_par.assign((size_t)S * cap, -7); hist_tok.assign((size_t)S * cap, -7);
    r.tok = tok.data(); r.scores = scores.data(); r.map = map.data(); r.idx_h = idx_h.data(); r.idx_m = idx_m.data();
    r.seg = seg.data(); r.ctrl = ctrl.data(); r.comp_n = comp_n.data(); r.fin = fin.data(); r.last_completed = last_completed.data();
    r.comp_t = comp_t.data(); r.comp_par = comp_par.data(); r.comp_score = comp_score.data();
    r.hist_par = hist_par.data(); r.hist_tok = hist_tok.data();
    r.N = N; r.beam = beam; r.cap = cap; r.V = V; r.S = S; r.end_token = END;
    attn_beam_host_init(r, GO);
  }
};

// one step's top-k of every sample: [N][beam] (row in the sample * V + word, value); unused entries are poison
struct Step { std::vector<int> topi; std::vector<float> topv; };
constexpr int X = 1 << 30;  // an index that must never be read (prev = X / V lies far outside every array)

void expect(bool ok, const char* name, const char* what) {
  if (!ok) { ++failures; printf("  %s: MISMATCH in %s\n", name, what); }
}
template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {  // the first b.size() entries
  for (size_t i = 0; i < b.size(); ++i) if (a[i] != b[i]) return false;
  return true;
}
// runs the script as the host loop does (it ends when no row is live or at step S - 1); returns the steps run
int run(Rec& R, const std::vector<Step>& script) {
  int steps = 0;
  for (const Step& st : script) {
    const int rows = attn_beam_host_advance(R.r, st.topv.data(), st.topi.data());
    ++steps;
    if (!rows || R.r.ctrl[0] == R.r.S) break;
  }
  return steps;
}
struct Result {
  std::vector<int64_t> seq;
  std::vector<int> len, path, plen;
  std::vector<float> score;
  explicit Result(const Rec& R) : seq((size_t)R.r.N * R.r.S, -9), len(R.r.N, -9), path((size_t)R.r.N * R.r.S, -9), plen(R.r.N, -9),
                                  score(R.r.N, -9.f) {
    attn_beam_host_finish(R.r, seq.data(), len.data(), score.data(), path.data(), plen.data());
  }
};
// sample i of a result: its tokens (zeros behind them), its score, its launch rows (nothing written behind them)
void check_result(const char* name, const Rec& R, const Result& o, int i, const std::vector<int64_t>& seq, float score,
                  const std::vector<int>& path) {
  const int S = R.r.S, n = (int)seq.size();
  expect(o.len[i] == n && o.plen[i] == n, name, "length");
  for (int j = 0; j < S; ++j) {
    expect(o.seq[(size_t)i * S + j] == (j < n ? seq[j] : 0), name, "sequence (zeros behind the length)");
    expect(o.path[(size_t)i * S + j] == (j < n ? path[j] : -9), name, "path (untouched behind the length)");
  }
  expect(o.score[i] == score, name, "score");
}
}  // namespace

int main() {
  {  // 1. one sample, beam 1: [s] at step 0 -> the sequence is [s] alone, its row of the step-0 launch is row 0
    const char* name = "1 end at step 0, beam 1";
    Rec R(1, 1, 4);
    expect(same(R.seg, {0, 1, 1}) && same(R.ctrl, {0, 1, 0, 0}) && R.tok[0] == GO && R.scores[0] == 0.f, name, "state after init");
    const int steps = run(R, {{{0 * V + END}, {-0.5f}}, {{X}, {0.f}}});
    expect(steps == 1 && same(R.ctrl, {1, 0, 1, 1}) && R.fin[0] == 1 && R.last_completed[0] == 1, name, "state after the step");
    expect(R.comp_n[0] == 1 && R.comp_t[0] == 0 && R.comp_par[0] == 0 && same(R.seg, {0, 0, 0}), name, "completed set");
    check_result(name, R, Result(R), 0, {END}, -0.5f, {0});
    printf("%s\n", name);
  }
  {  // 2. nothing completes in S = 3 steps: the first live row, its score, S tokens.  3. On the way: idx_m = first row + rank,
     //    which is not idx_h = parent row.
    const char* name = "2 nothing completes; 3 idx_m follows the rank";
    Rec R(1, 2, 3);
    // init: rows 0, 1 identical, row 0 ranked: seg = {0, 1, 2}
    expect(same(R.seg, {0, 1, 2}) && same(R.map, {0, 0}) && same(R.idx_h, {0, 1}) && same(R.ctrl, {0, 2, 0, 0}), name, "state after init");
    // step 0: both candidates extend row 0: row 0 = [3], row 1 = [4]                     idx_h = {0, 0}, idx_m = {0, 1}
    run(R, {{{0 * V + 3, 0 * V + 4}, {-0.1f, -0.2f}}});
    expect(same(R.idx_h, {0, 0}) && same(R.idx_m, {0, 1}) && same(R.seg, {0, 2, 2}), name, "step 0: both from row 0, memories by rank");
    // step 1: rank 0 = old row 1 + 5 = [4 5], rank 1 = old row 0 + 3 = [3 3]              idx_h = {1, 0}, idx_m = {0, 1}
    run(R, {{{1 * V + 5, 0 * V + 3}, {-0.3f, -0.4f}}});
    expect(same(R.idx_h, {1, 0}) && same(R.idx_m, {0, 1}) && same(R.tok, {5, 3}), name, "step 1: state by parent, memory by rank");
    // step 2: rank 0 = old row 0 + 4 = [4 5 4], rank 1 = old row 1 + 4 = [3 3 4]
    run(R, {{{0 * V + 4, 1 * V + 4}, {-0.6f, -0.7f}}});
    expect(same(R.ctrl, {3, 2, 0, 3}) && R.comp_n[0] == 0 && R.last_completed[0] == 0 && R.fin[0] == 0, name, "state after the loop");
    // [4 5 4] sat in row 0 of step 0's launch ([GO]), row 1 of step 1's ([4]), row 0 of step 2's ([4 5])
    check_result(name, R, Result(R), 0, {4, 5, 4}, -0.6f, {0, 1, 0});
    printf("%s\n", name);
  }
  // 4. two samples, beam 2: sample 0 finishes at step 1 and its rows drop out, sample 1's rows move from 1.. to 0..
  //    6. With S = 4 sample 1's last step completes nothing although it completed a hypothesis at step 2: its first live
  //    hypothesis is returned, not the completed one; with S = 3 the loop ends behind step 2 and the completed one is.
  for (int S = 4; S >= 3; --S) {
    const char* name = S == 4 ? "4 one sample drops out; 6 the last step completed nothing" : "4b the same, ended one step earlier";
    Rec R(2, 2, S);
    expect(same(R.seg, {0, 1, 2, 2, 1, 2}) && same(R.map, {0, 0, 1, 1}), name, "state after init");
    // step 0: s0 (first row 0): [s] completes (-0.2), rank 1 = [3];  s1 (first row 2): [4], [5]
    //         -> rows: 0 = s0 [3] (idx_h 0, idx_m 0 + 1), 1 = s1 [4] (2, 2), 2 = s1 [5] (2, 3)
    run(R, {{{0 * V + END, 0 * V + 3, 0 * V + 4, 0 * V + 5}, {-0.2f, -0.4f, -0.1f, -0.3f}}});
    expect(same(R.idx_h, {0, 2, 2}) && same(R.idx_m, {1, 2, 3}) && same(R.map, {0, 1, 1}) && same(R.seg, {0, 1, 1, 1, 2, 2}) &&
           same(R.last_completed, {1, 0}) && same(R.ctrl, {1, 3, 0, 1}), name, "step 0");
    // step 1: s0 wants 1: [3 s] completes (-0.9): k = 0, finished;  s1 (first row 1): rank 0 = its row 1 + 3 = [5 3], rank 1 =
    //         its row 0 + 4 = [4 4]  -> rows: 0 = s1 [5 3] (idx_h 2, idx_m 1), 1 = s1 [4 4] (idx_h 1, idx_m 2)
    run(R, {{{0 * V + END, X, 1 * V + 3, 0 * V + 4}, {-0.9f, 0.f, -0.5f, -0.6f}}});
    expect(same(R.fin, {1, 0}) && same(R.comp_n, {2, 0}) && same(R.ctrl, {2, 2, 0, 2}), name, "sample 0 finished, two rows live");
    expect(same(R.seg, {0, 0, 0, 0, 2, 2}), name, "segments after sample 0 dropped out");
    expect(same(R.idx_h, {2, 1}) && same(R.idx_m, {1, 2}) && same(R.map, {1, 1}) && same(R.tok, {3, 4}), name, "the shifted rows");
    // step 2: s0 skipped (its entries are never read, its last_completed stays);  s1 (first row 0): its row 0 + [s] completes
    //         [5 3 s] (-0.7), rank 1 = its row 1 + 5 = [4 4 5]  -> row 0 (idx_h 1, idx_m 0 + 1)
    // step 3: s1 wants 1: [4 4 5 3] (-1.5), nothing completes
    const int steps = run(R, {{{X, X, 0 * V + END, 1 * V + 5}, {0.f, 0.f, -0.7f, -0.8f}},
                              {{X, X, 0 * V + 3, X}, {0.f, 0.f, -1.5f, 0.f}}});
    expect(steps == S - 2 && R.r.ctrl[3] == S && R.comp_n[1] == 1 && R.comp_t[2] == 2 && R.comp_par[2] == 0, name, "state after the loop");
    expect(same(R.last_completed, {1, S == 4 ? 0 : 1}) && same(R.seg, {0, 0, 0, 0, 1, 1}), name, "last_completed");
    const Result o(R);
    check_result(name, R, o, 0, {END}, -0.2f, {0});  // -0.2 / 2 beats -0.9 / 3; the larger raw score is -0.2
    // s1 sat in row 2 of step 0's launch; [4] in row 1; [4 4] in row 1; [4 4 5] in row 0 -- [5] in row 2, [5 3] in row 0
    if (S == 4) check_result(name, R, o, 1, {4, 4, 5, 3}, -1.5f, {2, 1, 1, 0});
    else check_result(name, R, o, 1, {5, 3, END}, -0.7f, {2, 2, 0});
    printf("%s\n", name);
  }
  {  // 5. two completed hypotheses of different lengths with equal score / (t + 2) (-1.5 / 3 == -2.0 / 4, exact in double): the
     //    first wins; with -1.9 / 4 the later one is strictly better and wins -- and the score returned is still the MAXIMUM
     //    raw score, -1.5.  7. A step behind the stop changes nothing.
    for (int variant = 0; variant < 2; ++variant) {
      const char* name = variant ? "5b the later one strictly better" : "5a tie: the first wins; 7 a step behind the stop";
      Rec R(1, 2, 4);
      // step 0: [3], [4]; step 1: row 0 + [s] completes [3 s] (-1.5), rank 1 = row 1 + 5 = [4 5] (idx_h 1, idx_m 0 + 1);
      // step 2: wants 1: [4 5 s] completes, k = 0: finished, nothing live, the stop step is set
      const int steps = run(R, {{{0 * V + 3, 0 * V + 4}, {-0.25f, -0.5f}},
                                {{0 * V + END, 1 * V + 5}, {-1.5f, -1.2f}},
                                {{0 * V + END, X}, {variant ? -1.9f : -2.0f, 0.f}},
                                {{X, X}, {0.f, 0.f}}});
      expect(steps == 3 && R.comp_n[0] == 2 && R.fin[0] == 1 && same(R.ctrl, {3, 0, 3, 3}), name, "completed set");
      expect(same(R.comp_t, {1, 2}) && same(R.comp_par, {0, 0}) && R.last_completed[0] == 1, name, "completions");
      if (!variant) {
        const Rec before = R;
        const Step poison{{X, X}, {0.f, 0.f}};
        expect(attn_beam_host_advance(R.r, poison.topv.data(), poison.topi.data()) == 0, name, "live rows behind the stop");
        expect(R.ctrl == before.ctrl && R.seg == before.seg && R.tok == before.tok && R.scores == before.scores && R.map == before.map &&
               R.idx_h == before.idx_h && R.idx_m == before.idx_m && R.comp_n == before.comp_n && R.fin == before.fin &&
               R.last_completed == before.last_completed && R.comp_t == before.comp_t && R.comp_par == before.comp_par &&
               R.comp_score == before.comp_score && R.hist_par == before.hist_par && R.hist_tok == before.hist_tok,
               name, "a step behind the stop is a no-op");
      }
      if (variant) check_result(name, R, Result(R), 0, {4, 5, END}, -1.5f, {0, 1, 0});
      else check_result(name, R, Result(R), 0, {3, END}, -1.5f, {0, 0});
      printf("%s\n", name);
    }
  }
  {  // 8. no step run (not reachable through the loop; the pick still defines it): length 0, score 0, zeros
    const char* name = "8 no step run";
    Rec R(2, 3, 3);
    const Result o(R);
    check_result(name, R, o, 0, {}, 0.f, {});
    check_result(name, R, o, 1, {}, 0.f, {});
    printf("%s\n", name);
  }
  printf(failures ? "FAILED: %d mismatches\n" : "all cases agree\n", failures);
  return failures ? 1 : 0;
}
