// The TFM beam search's host bookkeeping (csrc/beam_host.h: beam_host_init, beam_host_advance, beam_select) driven with
// scripted per-step top-k results and compared with sequences, lengths and scores worked out by hand below.  Every array of
// the record is its own exact-size allocation, so AddressSanitizer sees any index past an end.  No GPU, no HIP.
//   cd tools/probe && g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I../../doc2tex_amd/csrc beam_host_check.cpp -o beam_host_check
//   ./beam_host_check        (prints one line per case; exit status 1 on any mismatch)
#include "beam_host.h"

#include <cstdio>
#include <vector>

namespace {
constexpr int PAD = 0, GO = 1, END = 2;  // converter/tfm_converter.py:8
int failures = 0;

struct Rec {
  std::vector<int64_t> tok;
  std::vector<float> scores, comp_score;
  std::vector<int> map, prev, seg, ctrl, comp_n, fin, comp_t, comp_par, hist_par, hist_tok;
  BeamRec r{};
  Rec(int N, int beam, int V, int S) {
    const int cap = N * beam;
    tok.assign(cap, -7); scores.assign(cap, -7.f); map.assign(cap, -7); prev.assign(cap, -7); seg.assign(3 * N, -7);
    ctrl.assign(8, -7); comp_n.assign(N, -7); fin.assign(N, -7);
    comp_t.assign(cap, -7); comp_par.assign(cap, -7); comp_score.assign(cap, -7.f);
    hist_par.assign((size_t)S * cap, -7); hist_tok.assign((size_t)S * cap, -7);
    r.tok = tok.data(); r.scores = scores.data(); r.map = map.data(); r.prev = prev.data(); r.seg = seg.data();
    r.ctrl = ctrl.data(); r.comp_n = comp_n.data(); r.fin = fin.data();
    r.comp_t = comp_t.data(); r.comp_par = comp_par.data(); r.comp_score = comp_score.data();
    r.hist_par = hist_par.data(); r.hist_tok = hist_tok.data();
    r.N = N; r.beam = beam; r.cap = cap; r.V = V; r.S = S; r.end_token = END;
    beam_host_init(r, GO);
  }
};

// one step's top-k of every sample: [N][beam] (row in the sample * V + word, value); unused entries are poison
struct Step { std::vector<int> topi; std::vector<float> topv; };
constexpr int X = 1 << 30;  // an index that must never be read (prev = X / V lies far outside every array)

void expect(bool ok, const char* name, const char* what) {
  if (!ok) { ++failures; printf("  %s: MISMATCH in %s\n", name, what); }
}
template <typename T>
bool same(const T* a, const std::vector<T>& b) {
  for (size_t i = 0; i < b.size(); ++i) if (a[i] != b[i]) return false;
  return true;
}
// runs the script (as the host loop does: stop when no row is live), returns the steps run
int run(Rec& R, const std::vector<Step>& script) {
  int steps = 0;
  for (const Step& st : script) {
    if (!R.r.ctrl[1]) break;
    beam_host_advance(R.r, st.topv.data(), st.topi.data());
    ++steps;
  }
  return steps;
}
void check_result(const char* name, const Rec& R, int i, const std::vector<int64_t>& seq, float score) {
  std::vector<int64_t> out(R.r.S, -9);
  int len = -1;
  float sc = -9.f;
  beam_select(R.r, i, PAD, out.data(), &len, &sc);
  expect(len == (int)seq.size(), name, "length");
  expect(len == (int)seq.size() && same(out.data(), seq), name, "sequence");
  expect(sc == score, name, "score");
  for (int j = len < 0 ? 0 : len; j < R.r.S; ++j) expect(out[j] == -9, name, "tokens behind the returned length were written");
}
}  // namespace

int main() {
  {  // 1. one sample, beam 1: [s] at step 0 -> the sequence is [s] alone
    const char* name = "1 end at step 0";
    Rec R(1, 1, 5, 4);
    const int steps = run(R, {{{0 * 5 + END}, {-0.5f}}, {{X}, {0.f}}});
    expect(steps == 1 && R.r.ctrl[1] == 0 && R.r.ctrl[2] == 1 && R.fin[0] == 1, name, "state after the step");
    check_result(name, R, 0, {END}, -0.5f);
    printf("%s\n", name);
  }
  {  // 2. nothing completes in S = 3 steps: the first live row, S tokens, its score
    const char* name = "2 nothing completes";
    const int V = 6;
    Rec R(1, 2, V, 3);
    // step 0: row 0 = [3], row 1 = [4]; step 1: row 0 = old row 1 + 5 = [4 5], row 1 = old row 0 + 3 = [3 3];
    // step 2: row 0 = old row 0 + 4 = [4 5 4], row 1 = old row 1 + 4 = [3 3 4]
    const int steps = run(R, {{{0 * V + 3, 0 * V + 4}, {-0.1f, -0.2f}},
                              {{1 * V + 5, 0 * V + 3}, {-0.3f, -0.4f}},
                              {{0 * V + 4, 1 * V + 4}, {-0.6f, -0.7f}}});
    expect(steps == 3 && R.r.ctrl[3] == 3 && R.r.ctrl[1] == 2 && R.comp_n[0] == 0, name, "state after the loop");
    check_result(name, R, 0, {4, 5, 4}, -0.6f);
    printf("%s\n", name);
  }
  {  // 3. a hypothesis completes at the last step S - 1 = 2: S tokens, the last one [s]
    const char* name = "3 completes at the last step";
    const int V = 6;
    Rec R(1, 2, V, 3);
    // step 0: [3], [4]; step 1: row 0 = [3 5], row 1 = [4 3]; step 2: old row 1 + [s] completes = [4 3 s], old row 0 + 4 stays live
    run(R, {{{0 * V + 3, 0 * V + 4}, {-0.1f, -0.2f}},
            {{0 * V + 5, 1 * V + 3}, {-0.3f, -0.5f}},
            {{1 * V + END, 0 * V + 4}, {-0.9f, -1.0f}}});
    expect(R.comp_n[0] == 1 && R.comp_t[0] == 2 && R.comp_par[0] == 1 && R.r.ctrl[1] == 1, name, "completed set");
    check_result(name, R, 0, {4, 3, END}, -0.9f);
    printf("%s\n", name);
  }
  {  // 4. two samples, beam 2: sample 0 fills its completed set at step 1 and drops out; sample 1's rows move from 1.. to 0..
    const char* name = "4 one sample drops out";
    const int V = 6;
    Rec R(2, 2, V, 4);
    // step 0: s0: [s] completes (-0.2), [3] live;  s1: [4], [5] live            -> rows: 0 = s0 [3], 1 = s1 [4], 2 = s1 [5]
    // step 1: s0 wants 1: [3 s] completes (-0.9): finished;  s1 (first row 1): its row 1 + 3 = [5 3], its row 0 + 4 = [4 4]
    //                                                                           -> rows: 0 = s1 [5 3] (parent 2), 1 = s1 [4 4] (parent 1)
    run(R, {{{0 * V + END, 0 * V + 3, 0 * V + 4, 0 * V + 5}, {-0.2f, -0.4f, -0.1f, -0.3f}},
            {{0 * V + END, X, 1 * V + 3, 0 * V + 4}, {-0.9f, 0.f, -0.5f, -0.6f}}});
    expect(R.fin[0] == 1 && R.comp_n[0] == 2 && R.r.ctrl[1] == 2, name, "sample 0 finished, two rows live");
    expect(same(R.seg.data(), std::vector<int>{0, 0, 0, 0, 2, 2}), name, "segments after sample 0 dropped out");
    expect(same(R.prev.data(), std::vector<int>{2, 1}) && same(R.map.data(), std::vector<int>{1, 1}), name, "gather indices / row map");
    expect(same(R.tok.data(), std::vector<int64_t>{3, 4}), name, "tokens of the shifted rows");
    // step 2: s0 skipped (its entries are never read); s1: row 0 + [s] completes [5 3 s] (-0.7), row 1 + 5 = [4 4 5] live
    // step 3: s1 wants 1: [4 4 5 3] live
    run(R, {{{X, X, 0 * V + END, 1 * V + 5}, {0.f, 0.f, -0.7f, -0.8f}},
            {{X, X, 0 * V + 3, X}, {0.f, 0.f, -1.5f, 0.f}}});
    expect(R.r.ctrl[3] == 4 && R.comp_n[1] == 1, name, "state after the loop");
    check_result(name, R, 0, {END}, -0.2f);        // -0.2 / 1 beats -0.9 / 2
    check_result(name, R, 1, {5, 3, END}, -0.7f);  // its only completed hypothesis beats nothing: live rows are not candidates
    printf("%s\n", name);
  }
  {  // 5. two completed hypotheses with equal score over length (-1.0 / 2 == -1.5 / 3, exact in double): the first wins;
     //    with -1.4 / 3 the later one is strictly better and wins
    const int V = 6;
    for (int variant = 0; variant < 2; ++variant) {
      const char* name = variant ? "5b the later one strictly better" : "5a tie: the first wins";
      Rec R(1, 2, V, 4);
      // step 0: [3], [4]; step 1: row 0 + [s] completes [3 s] (-1.0), row 1 + 5 = [4 5]; step 2: wants 1: [4 5 s] completes
      run(R, {{{0 * V + 3, 0 * V + 4}, {-0.25f, -0.5f}},
              {{0 * V + END, 1 * V + 5}, {-1.0f, -1.2f}},
              {{0 * V + END, X}, {variant ? -1.4f : -1.5f, 0.f}}});
      expect(R.comp_n[0] == 2 && R.fin[0] == 1 && R.r.ctrl[1] == 0, name, "completed set");
      if (variant) check_result(name, R, 0, {4, 5, END}, -1.4f);
      else check_result(name, R, 0, {3, END}, -1.0f);
      printf("%s\n", name);
    }
  }
  {  // 6. beam 3 with one hypothesis completed: at step 1 both wanted candidates are [s].  No row is live after that step, the
     //    loop ends there, and the best of the three completed is returned
    const char* name = "6 every candidate ends";
    const int V = 6;
    Rec R(1, 3, V, 4);
    // step 0: [s] completes (-0.6), [3], [4] live; step 1 (wants 2): [3 s] (-1.0) and [4 s] (-1.6) complete
    const int steps = run(R, {{{0 * V + END, 0 * V + 3, 0 * V + 4}, {-0.6f, -0.7f, -0.8f}},
                              {{0 * V + END, 1 * V + END, X}, {-1.0f, -1.6f, 0.f}},
                              {{X, X, X}, {0.f, 0.f, 0.f}}});
    expect(steps == 2 && R.r.ctrl[1] == 0 && R.r.ctrl[2] == 2 && R.comp_n[0] == 3, name, "state after the loop");
    expect(same(R.seg.data(), std::vector<int>{0, 0, 0}), name, "segment of the sample");
    const Step poison{{X, X, X}, {0.f, 0.f, 0.f}};
    expect(beam_host_advance(R.r, poison.topv.data(), poison.topi.data()) == 0 && R.r.ctrl[0] == 2, name, "a step behind the stop is a no-op");
    check_result(name, R, 0, {3, END}, -1.0f);  // -0.6 / 1, -1.0 / 2, -1.6 / 2
    printf("%s\n", name);
  }
  {  // 7. nothing completed and no live row (not reachable through advance; the selection still defines it): all PAD, score 0
    const char* name = "7 nothing at all";
    Rec R(1, 2, 6, 3);
    R.seg[1] = 0;
    check_result(name, R, 0, {PAD, PAD, PAD}, 0.f);
    printf("%s\n", name);
  }
  printf(failures ? "FAILED: %d mismatches\n" : "all cases agree\n", failures);
  return failures ? 1 : 0;
}
