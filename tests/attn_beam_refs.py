"""Pure-Python statements of the LSTM-attention beam search's bookkeeping (Attention / AttentionV2.forward_beam), for the
tests of both step loops:

* `Rec` + `rec_init` / `rec_advance` / `rec_finish`: the rules on the record both loops keep (csrc/attn_beam_host.h
  AttnBeamDev) -- what the host loop's attn_beam_host_init / _advance / _finish and the device-side loop's
  attn_beam_dev_init / _advance / _finish_kernel must write, array for array.  A Rec starts filled with canaries, and these
  functions write exactly the entries the C++ writes, so comparing whole arrays also shows that nothing else was touched.
* `brute_force`: the same search restated the way the reference keeps it -- whole token sequences and whole row paths in
  lists, no record, no history.  It mirrors no C++ text: it is the only whole-sequence statement left, and the record-based
  rules are checked against it on the CPU.

Both read their candidates from a `Stream`: seeded, and a function of (step, sample, k, rows ranked) alone, so two
implementations that disagree about a sample's state draw different candidates and cannot agree by accident.  numpy only."""
import numpy as np

END = 1  # [s] (attn_converter.py:8); [GO] = 0
ICAN, FCAN = -77, np.float32(-7.25)  # canaries of the integer and the float arrays

INT_FIELDS = ("ctrl", "tok", "map", "idx_h", "idx_m", "seg", "comp_n", "fin", "last_completed", "comp_t", "comp_par", "hist_par",
              "hist_tok")
FLOAT_FIELDS = ("scores", "comp_score")
FIELDS = INT_FIELDS + FLOAT_FIELDS


class Stream:
    """Candidates of (step, sample): k of them over `rows` ranked rows of a V-word vocabulary.  [s] with probability p_end
    (always from step end_from on); half of the values are -(step + 2) * q with q in {0.25, 0.5}, so that completed hypotheses
    of different lengths have EQUAL score / length, the others seeded normals."""

    def __init__(self, V, seed, p_end=0.2, end_from=None):
        self.V, self.seed, self.p_end, self.end_from = V, seed, p_end, end_from

    def __call__(self, step, i, k, rows):
        g = np.random.default_rng([self.seed, step, i])
        prev = g.integers(0, rows, k)
        word = g.integers(2, self.V, k)
        ends = g.random(k) < self.p_end
        if self.end_from is not None and step >= self.end_from:
            ends[:] = True
        word[ends] = END
        word[(~ends) & (g.random(k) < 0.1)] = 0  # [GO] is a word like any other
        crafted = -(step + 2) * g.choice(np.array([0.25, 0.5]), k)
        val = np.where(g.random(k) < 0.5, crafted, g.standard_normal(k) - 2.0).astype(np.float32)
        return val, (prev * self.V + word).astype(np.int32)


class Rec:
    def __init__(self, N, beam, S, V, cap=None):
        self.N, self.beam, self.S, self.V = N, beam, S, V
        self.cap = cap = N * beam if cap is None else cap
        I = lambda *shape: np.full(shape, ICAN, np.int32)
        F = lambda *shape: np.full(shape, FCAN, np.float32)
        self.ctrl = I(4)
        self.tok = np.full((cap,), ICAN, np.int64)
        self.scores = F(cap)
        self.map, self.idx_h, self.idx_m = I(cap), I(cap), I(cap)
        self.seg = I(N, 3)
        self.comp_n, self.fin, self.last_completed = I(N), I(N), I(N)
        self.comp_t, self.comp_par, self.comp_score = I(N, beam), I(N, beam), F(N, beam)
        self.hist_par, self.hist_tok = I(S, cap), I(S, cap)


def rec_init(r, go=0):
    """step 0: `beam` rows per sample from [GO] with score 0, of which row 0 is ranked (seq2seq.py:145-146)"""
    n = r.N * r.beam
    for i in range(r.N):
        r.seg[i] = (i * r.beam, 1, r.beam)
    r.comp_n[:], r.fin[:], r.last_completed[:] = 0, 0, 0
    r.tok[:n], r.scores[:n] = go, 0.0
    r.map[:n] = np.arange(n) // r.beam
    r.idx_h[:n] = r.idx_m[:n] = np.arange(n)
    r.ctrl[:] = (0, n, 0, 0)


def candidates(r, stream):
    """topv / topi [N][beam] of the record's current step, canaries wherever the step kernels write nothing"""
    topv = np.full((r.N, r.beam), FCAN, np.float32)
    topi = np.full((r.N, r.beam), ICAN, np.int32)
    t = int(r.ctrl[0])
    for i in range(r.N):
        if not r.fin[i]:
            k = int(r.seg[i, 2])
            topv[i, :k], topi[i, :k] = stream(t, i, k, int(r.seg[i, 1]))
    return topv, topi


def rec_advance(r, topv, topi):
    t = int(r.ctrl[0])
    if r.ctrl[2] and t >= r.ctrl[2]:
        return
    new = {}
    for i in range(r.N):  # (everything is read before anything is written: the kernel's first pass)
        if r.fin[i]:
            continue
        off, k = int(r.seg[i, 0]), int(r.seg[i, 2])
        new[i] = (off, k, [(q, int(topi[i, q]) // r.V, int(topi[i, q]) % r.V, topv[i, q]) for q in range(k)])
    row = 0
    for i in range(r.N):
        if i not in new:
            continue
        off, k, cand = new[i]
        first, cn = row, int(r.comp_n[i])
        for q, prev, word, val in cand:
            if word == END:
                r.comp_t[i, cn], r.comp_par[i, cn], r.comp_score[i, cn] = t, off + prev, val
                cn += 1
            else:
                r.idx_h[row], r.idx_m[row] = off + prev, off + q
                r.tok[row], r.scores[row], r.map[row] = word, val, i
                r.hist_par[t, row], r.hist_tok[t, row] = off + prev, word
                row += 1
        m = row - first
        r.last_completed[i] = int(m < k)
        r.comp_n[i] = cn
        r.seg[i] = (first, m, m)
        if m == 0:
            r.fin[i] = 1
    r.ctrl[0], r.ctrl[1], r.ctrl[3] = t + 1, row, t + 1
    if row == 0:
        r.ctrl[2] = t + 1


def rec_finish(r, with_path=True):
    """seq [N][S] (zeros beyond the length), len, score, path [N][S] (canaries beyond the length), plen"""
    seq = np.full((r.N, r.S), ICAN, np.int64)
    ln, score = np.full(r.N, ICAN, np.int32), np.full(r.N, FCAN, np.float32)
    path, plen = np.full((r.N, r.S), ICAN, np.int32), np.full(r.N, ICAN, np.int32)
    for i in range(r.N):
        if not r.last_completed[i]:
            t = int(r.ctrl[3]) - 1
            row = int(r.seg[i, 0])
            sc, n = r.scores[row], t + 1
        else:
            cs, ct = r.comp_score[i], r.comp_t[i]
            best = 0
            for j in range(1, int(r.comp_n[i])):
                if float(cs[j]) / float(ct[j] + 2) > float(cs[best]) / float(ct[best] + 2):
                    best = j
            sc = np.max(cs[:int(r.comp_n[i])])
            t = int(ct[best])
            n = t + 1
            row = int(r.comp_par[i, best])
            seq[i, t], path[i, t] = END, row
            t -= 1
        while t >= 0:
            seq[i, t] = r.hist_tok[t, row]
            row = int(r.hist_par[t, row])
            path[i, t] = row
            t -= 1
        seq[i, n:] = 0
        ln[i], score[i], plen[i] = n, sc, n
    return (seq, ln, score, path, plen) if with_path else (seq, ln, score)


def run_record(N, beam, S, V, stream):
    """the whole search on a record: (record, steps run, finish outputs)"""
    r = Rec(N, beam, S, V)
    rec_init(r)
    for _ in range(S):
        rec_advance(r, *candidates(r, stream))
    return r, int(r.ctrl[3]), rec_finish(r)


def brute_force(N, beam, S, V, stream):
    """The reference's bookkeeping (forward_beam), whole sequences and whole launch-row paths in lists.  Returns per sample
    (tokens without [GO], score, path), the steps executed, and the set of things that happened on the way."""
    sm = [dict(seqs=[[0] for _ in range(beam)], paths=[[] for _ in range(beam)], live=[np.float32(0)] * beam, complete=[],
               cpaths=[], cscores=[], k=beam, last=False, fin=False) for _ in range(N)]
    events, steps = set(), 0
    for step in range(S):
        offs, rows = [], 0
        for x in sm:
            offs.append(rows)
            rows += 0 if x["fin"] else len(x["seqs"])
        steps = step + 1
        live_before = sum(not x["fin"] for x in sm)
        nrows = finished_now = 0
        for i, x in enumerate(sm):
            if x["fin"]:
                continue
            off = offs[i]
            val, idx = stream(step, i, x["k"], 1 if step == 0 else len(x["seqs"]))
            nseqs, npaths, nscores = [], [], []
            x["last"] = False
            for q in range(x["k"]):
                prev, word = int(idx[q]) // V, int(idx[q]) % V
                sq, pa = x["seqs"][prev] + [word], x["paths"][prev] + [off + prev]
                if word == END:
                    x["complete"].append(sq)
                    x["cpaths"].append(pa)
                    x["cscores"].append(val[q])
                    x["last"] = True
                else:
                    nrows += 1
                    nseqs.append(sq)
                    npaths.append(pa)
                    nscores.append(val[q])
            x["seqs"], x["paths"], x["live"], x["k"] = nseqs, npaths, nscores, len(nseqs)
            if x["k"] == 0:
                x["fin"] = True
                finished_now += 1
        if 0 < finished_now < live_before:
            events.add("a sample finishes while others continue")
        if finished_now == live_before and live_before == N:
            events.add("all samples finish at one step")
        if not nrows:
            break
    if steps == S and any(not x["fin"] for x in sm):
        events.add("the limit is reached with survivors")
    out = []
    for x in sm:
        if not x["last"]:
            events.add("nothing completed at the last step")
            out.append((x["seqs"][0][1:], x["live"][0], x["paths"][0]))
            continue
        ratio = [float(s) / float(len(c)) for s, c in zip(x["cscores"], x["complete"])]
        best = 0
        for j in range(1, len(ratio)):
            if ratio[j] > ratio[best]:
                best = j
        if ratio.count(ratio[best]) > 1 and len({len(c) for c, v in zip(x["complete"], ratio) if v == ratio[best]}) > 1:
            events.add("two completed hypotheses of different lengths tie at the best score / len")
        out.append((x["complete"][best][1:], max(x["cscores"]), x["cpaths"][best]))
    return out, steps, events
