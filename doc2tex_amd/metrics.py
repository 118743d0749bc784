"""The four validation metrics of the reference's training loop with their quadratic work on the device.

Mirrors doc2tex/modules/metrics/ed.py (`get_single_ED`, `get_word_NED`), doc2tex/modules/metrics/bleu.py (`bleu_score`)
and what engine/inferencing.py:127-138,221-230 does with them:

  * Levenshtein distances come from `d2t_metric_edit_distance` (one block per pair, csrc/metrics.hip) -- the reference
    imports `python-Levenshtein` and runs one DP per sample on the host;
  * BLEU's clipped n-gram counts come from `d2t_metric_bleu_counts` on the token tensors the model returned -- the
    reference builds a `Counter` of every 1- to 4-gram per sample;
  * everything after the integers is the reference's own host arithmetic in its own order, so equal integers give
    bit-equal floats.  For BLEU that holds while the corpus totals stay below 2**24: the reference accumulates its counts
    in float32 tensors, which are exact up to there and round beyond; this module sums integers and rounds once.

`ValidationMetrics` keeps the per-sample integers of a whole validation run on the device and downloads them once.
There is no host fallback: without the library or a HIP device every call raises.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

ED_MAX_LEN = _lib.METRIC_ED_MAX_LEN
BLEU_MAX_COLS = _lib.METRIC_BLEU_MAX_COLS
_NO_END = -1  # end_token of rows this module packs itself (its ids are >= 0)


def _symbols(seqs, table):
    """Each sequence as an int32 array: code points of a str, ids from `table` (one dictionary per call) otherwise."""
    out = []
    for s in seqs:
        if isinstance(s, str):
            out.append(np.frombuffer(s.encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.int32))
        else:
            out.append(np.fromiter((table.setdefault(x, len(table)) for x in s), dtype=np.int32))
    return out


def _launch_edit_distance(a, b, device=None):
    """a, b: equally long lists of int32 arrays -> int32 device tensor [N].  One pinned staging buffer, one H2D copy."""
    lib = _lib.require_device()
    n = len(a)
    if len(b) != n:
        raise ValueError(f"edit_distance: {n} strings against {len(b)}")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=device)
    la = np.fromiter((len(x) for x in a), dtype=np.int64, count=n)
    lb = np.fromiter((len(x) for x in b), dtype=np.int64, count=n)
    max_len = int(max(la.max(initial=0), lb.max(initial=0)))
    if max_len > ED_MAX_LEN:
        raise ValueError(f"edit_distance: a string of {max_len} symbols exceeds the kernel's cap of {ED_MAX_LEN}")
    ta, tb = int(la.sum()), int(lb.sum())
    # staging layout: a_off [n + 1] int64 | b_off [n + 1] int64 | a symbols int32 | b symbols int32
    off_bytes = 2 * (n + 1) * 8
    stage = torch.empty(off_bytes + 4 * (ta + tb), dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    offs = host[:off_bytes].view(np.int64)
    offs[0] = 0
    np.cumsum(la, out=offs[1:n + 1])
    offs[n + 1] = 0
    np.cumsum(lb, out=offs[n + 2:])
    syms = host[off_bytes:].view(np.int32)
    if ta:
        np.concatenate(a, out=syms[:ta])
    if tb:
        np.concatenate(b, out=syms[ta:])
    dev = stage.to(device, non_blocking=True)
    dist = torch.empty(n, dtype=torch.int32, device=device)
    need = C.c_int64(0)
    _lib.check(lib.d2t_metric_edit_distance_workspace(n, max_len, C.byref(need)), None, "metric_edit_distance_workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=device) if need.value else None
    base = dev.data_ptr()
    with torch.cuda.device(device):
        _lib.check(lib.d2t_metric_edit_distance(
            C.c_void_p(base + off_bytes) if ta else None, C.c_void_p(base), ta,
            C.c_void_p(base + off_bytes + 4 * ta) if tb else None, C.c_void_p(base + (n + 1) * 8), tb,
            _lib.ptr(dist), n, max_len, _lib.ptr(ws), need.value, _lib.stream_of(dist)), None, "metric_edit_distance")
    return dist


def edit_distance(a, b):
    """Levenshtein distances of N pairs -> int32 device tensor [N] (not read back).  `a`, `b`: lists of str (symbols are code
    points, as `len` and indexing see them) or lists of sequences of hashables (mapped to ints through one dictionary per
    call; a list of words is one such sequence).  A string beyond ED_MAX_LEN symbols raises ValueError."""
    _lib.require_device()
    table = {}
    return _launch_edit_distance(_symbols(a, table), _symbols(b, table))


def _single_ed(gt, pred, dist):
    # ed.py:6-12 given the distance
    if len(gt) == 0 or len(pred) == 0:
        return 0
    if len(gt) > len(pred):
        return 1 - dist / len(gt)
    return 1 - dist / len(pred)


def get_single_ED(gt, pred):
    """ICDAR2019 normalised edit distance of one pair (ed.py:4-12); an empty `gt` or `pred` scores 0."""
    _lib.require_device()
    if len(gt) == 0 or len(pred) == 0:
        return 0
    return _single_ed(gt, pred, int(edit_distance([pred], [gt]).item()))


def _word_ned(word_dists, preds, gts, n_gts):
    # ed.py:16-39 given the word-level distances of the zipped pairs; n_gts = len(list_gts)
    word_NED = 0
    for d, gt, pred in zip(word_dists, gts, preds):
        cur_max_len = max(len(gt.split()), len(pred.split()))
        if len(gt) == 0 or len(pred) == 0:
            word_NED += 0
        else:
            word_NED += 1 - d / cur_max_len  # ZeroDivisionError for non-empty strings without a word, as the reference
    return word_NED / float(n_gts)


def get_word_NED(list_preds, list_gts):
    """Mean over the pairs of 1 - word distance / max(word counts) (ed.py:15-39); `str.split()` gives the words, a pair with
    an empty string scores 0, a single str counts as a list of one."""
    _lib.require_device()
    if isinstance(list_preds, str):
        list_preds = [list_preds]
    if isinstance(list_gts, str):
        list_gts = [list_gts]
    pairs = list(zip(list_gts, list_preds))
    gts, preds = [g for g, _ in pairs], [p for _, p in pairs]
    dists = edit_distance([g.split() for g in gts], [p.split() for p in preds]).tolist() if pairs else []
    return _word_ned(dists, preds, gts, len(list_gts))


def _launch_bleu_counts(cand, ref, end_token, max_n):
    """cand [N, C], ref [N, R] int64 device tensors -> int64 device tensor [N, 2 + max_n]."""
    lib = _lib.require_device()
    if not 1 <= max_n <= 4:
        raise ValueError(f"bleu: max_n must be 1..4, got {max_n}")
    if cand.dim() != 2 or ref.dim() != 2 or cand.shape[0] != ref.shape[0]:
        raise ValueError(f"bleu: candidate rows {tuple(cand.shape)} and reference rows {tuple(ref.shape)} do not pair up")
    if not cand.is_cuda or ref.device != cand.device:
        raise RuntimeError("bleu: token tensors must be ROCm tensors of one device (the engine has no CPU path)")
    for name, t in (("candidate", cand), ("reference", ref)):
        if not 1 <= t.shape[1] <= BLEU_MAX_COLS:
            raise ValueError(f"bleu: {name} rows of {t.shape[1]} tokens; the kernel takes 1..{BLEU_MAX_COLS}")
    cand = cand.to(torch.int64).contiguous()
    ref = ref.to(torch.int64).contiguous()
    n = cand.shape[0]
    out = torch.empty((n, 2 + max_n), dtype=torch.int64, device=cand.device)
    with torch.cuda.device(cand.device):
        _lib.check(lib.d2t_metric_bleu_counts(_lib.ptr(cand), cand.shape[1], _lib.ptr(ref), ref.shape[1], n, int(end_token),
                                              max_n, _lib.ptr(out), _lib.stream_of(out)), None, "metric_bleu_counts")
    return out


def bleu_counts(cand, ref, end_token, max_n=4):
    """Per sample `cand_len, ref_len, clipped_1 .. clipped_max_n` of token rows cut at their first `end_token`."""
    return _launch_bleu_counts(cand, ref, end_token, max_n)


def _bleu_from_counts(counts, max_n, weights):
    """bleu.py:81-120 from the per-sample integers [N][2 + max_n] (host): returns (score, clipped, total)."""
    clipped = [0] * max_n
    total = [0] * max_n
    candidate_len = 0.0
    refs_len = 0.0
    for row in counts:
        candidate_len += row[0]
        refs_len += float(row[1])
        for i in range(max_n):
            clipped[i] += row[2 + i]
            total[i] += max(row[0] - i, 0)
    clipped_counts = torch.tensor(clipped, dtype=torch.float32)
    total_counts = torch.tensor(total, dtype=torch.float32)
    weights = torch.tensor(weights)
    if min(clipped_counts) == 0:
        return 0.0, clipped, total
    pn = clipped_counts / total_counts
    log_pn = weights * torch.log(pn)
    score = torch.exp(sum(log_pn))
    bp = math.exp(min(1 - refs_len / candidate_len, 0))
    return bp * score.item(), clipped, total


def _pack_token_rows(corpus, table):
    width = max([len(s) for s in corpus] + [1])
    rows = np.full((len(corpus), width), _NO_END, dtype=np.int64)
    for i, s in enumerate(corpus):
        rows[i, :len(s)] = [table.setdefault(t, len(table)) for t in s]
    return rows


def bleu_corpus_counts(candidate_corpus, references_corpus, max_n=4):
    """The integers behind `bleu_score`: per-sample counts [N][2 + max_n] as a host list (one download)."""
    _lib.require_device()
    candidate_corpus = [list(c) for c in candidate_corpus]
    references_corpus = [[list(r) for r in refs] for refs in references_corpus]
    assert len(candidate_corpus) == len(references_corpus), "The length of candidate and reference corpus should be the same"
    for refs in references_corpus:
        if len(refs) != 1:
            raise ValueError(f"bleu_score: {len(refs)} references for one candidate; the kernel path serves exactly one "
                             "reference per candidate (what validation_step passes)")
    if not candidate_corpus:
        return []
    table = {}
    cand = _pack_token_rows(candidate_corpus, table)
    ref = _pack_token_rows([refs[0] for refs in references_corpus], table)
    # one pinned staging buffer, one copy
    stage = torch.empty(cand.size + ref.size, dtype=torch.int64, pin_memory=True)
    stage[:cand.size] = torch.from_numpy(cand).view(-1)
    stage[cand.size:] = torch.from_numpy(ref).view(-1)
    dev = stage.to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
    out = _launch_bleu_counts(dev[:cand.size].view(cand.shape), dev[cand.size:].view(ref.shape), _NO_END, max_n)
    return out.cpu().tolist()


def bleu_score(candidate_corpus, references_corpus, max_n=4, weights=[0.25] * 4):
    """Drop-in for modules/metrics/bleu.py `bleu_score` on corpora with ONE reference per candidate (more raise ValueError).
    Tokens are mapped to ids on the host, the clipped counts come from the kernel, and the closing expression is the
    reference's float32 torch CPU expression fed from the integer sums: the value equals the reference's bit for bit while
    the corpus counts stay below 2**24 (the reference's own float32 accumulators are exact only up to there)."""
    assert max_n == len(weights), 'Length of the "weights" list has be equal to max_n'
    counts = bleu_corpus_counts(candidate_corpus, references_corpus, max_n)
    return _bleu_from_counts(counts, max_n, weights)[0]


class ValidationMetrics:
    """Accumulates one validation run (engine/inferencing.py:127-138,221-230).

    update() launches the kernels on the current stream and appends their per-sample integers to device buffers without
    reading them; compute() downloads them once and finishes on the host in the reference's order.  `end_token` is the id
    of "[s]" (converter.dict["[s]"]); BLEU is computed only for token_level "word"."""

    def __init__(self, end_token, token_level="word", max_n=4, weights=(0.25, 0.25, 0.25, 0.25)):
        _lib.require_device()
        self.end_token, self.token_level, self.max_n, self.weights = int(end_token), token_level, int(max_n), list(weights)
        assert self.max_n == len(self.weights), 'Length of the "weights" list has be equal to max_n'
        self.reset()

    def reset(self):
        self._dists = []   # device int32 [2 * B] per update: character distances, then word distances
        self._bleu = []    # device int64 [B, 2 + max_n] per update
        self._preds, self._gts = [], []

    def update(self, pred_index, target_index, pred_strs, gt_strs):
        """pred_index / target_index: device token tensors [B, *] (BLEU, cut at `end_token`); pred_strs / gt_strs: the B
        post-processed host strings (exact match, character NED, word NED)."""
        _lib.require_device()
        pred_strs, gt_strs = list(pred_strs), list(gt_strs)
        B = len(pred_strs)
        if len(gt_strs) != B or pred_index.shape[0] != B or target_index.shape[0] != B:
            raise ValueError("ValidationMetrics.update: tensors and string lists disagree on the batch size")
        table = {}
        a = _symbols(pred_strs, table) + _symbols([s.split() for s in pred_strs], table)
        b = _symbols(gt_strs, table) + _symbols([s.split() for s in gt_strs], table)
        self._dists.append(_launch_edit_distance(a, b, pred_index.device))
        if self.token_level == "word":
            self._bleu.append(_launch_bleu_counts(pred_index, target_index.to(pred_index.device), self.end_token, self.max_n))
        self._preds += pred_strs
        self._gts += gt_strs

    def compute(self):
        """-> dict(accuracy, norm_ED, word_ED, bleu, records); `records` holds one dict per sample (pred, gt, correct,
        char_dist, word_dist, and with BLEU cand_len, ref_len, clipped).  No sample at all divides by zero as the
        reference does."""
        n = len(self._preds)
        word = self.token_level == "word"
        if n:  # one download: every buffer flattened into one int64 vector
            parts = [d.to(torch.int64) for d in self._dists] + ([t.reshape(-1) for t in self._bleu] if word else [])
            flat = torch.cat(parts).cpu().tolist()
        else:
            flat = []
        char_d, word_d, pos = [], [], 0
        for d in self._dists:
            B = d.numel() // 2
            char_d += flat[pos:pos + B]
            word_d += flat[pos + B:pos + 2 * B]
            pos += 2 * B
        w = 2 + self.max_n
        counts = [flat[pos + i * w:pos + (i + 1) * w] for i in range(n)] if word else None
        n_correct = 0
        norm_ED = 0
        word_ED = 0
        records = []
        for i, (pred, gt) in enumerate(zip(self._preds, self._gts)):
            if min(char_d[i], word_d[i]) < 0:
                raise RuntimeError(f"ValidationMetrics: the edit-distance kernel refused sample {i}")
            correct = char_d[i] == 0
            if correct:
                n_correct += 1
            norm_ED += _single_ed(gt, pred, char_d[i])
            word_ED += _word_ned([word_d[i]], [pred], [gt], 1)
            rec = {"pred": pred, "gt": gt, "correct": correct, "char_dist": char_d[i], "word_dist": word_d[i]}
            if word:
                rec.update(cand_len=counts[i][0], ref_len=counts[i][1], clipped=counts[i][2:])
            records.append(rec)
        accuracy = n_correct / float(n)
        norm_ED = norm_ED / float(n)
        word_ED = word_ED / float(n)
        bleu = _bleu_from_counts(counts, self.max_n, self.weights)[0] if word else None
        return {"accuracy": accuracy, "norm_ED": norm_ED, "word_ED": word_ED, "bleu": bleu, "records": records}
