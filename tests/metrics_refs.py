"""Host references for the validation metrics (tests/test_metrics_*.py, tests/test_validate_gpu.py), written from the
definitions: Levenshtein distance, the two normalised edit distances of modules/metrics/ed.py, and BLEU with one reference
per candidate (modules/metrics/bleu.py).  tests/test_metrics_refs_cpu.py checks them against a plain triple-loop DP and
against the reference's recorded BLEU values."""
import collections
import math

import numpy as np
import torch


def symbols(seq, table=None):
    """int64 array of a sequence: code points of a str, otherwise ids of its items through `table`."""
    if isinstance(seq, str):
        return np.array([ord(c) for c in seq], dtype=np.int64)
    table = {} if table is None else table
    return np.array([table.setdefault(x, len(table)) for x in seq], dtype=np.int64)


def levenshtein(a, b):
    """Insert / delete / substitute, each 1.  Row-wise DP over the longer string, each row vectorised: with
    t[j] = min(D[i-1][j] + 1, D[i-1][j-1] + [a_i != b_j]) the in-row chain D[i][j] = min(t[j], D[i][j-1] + 1) unrolls to
    D[i][j] = j + min_{k <= j}(t[k] - k), a running minimum (a 16384 x 16384 pair takes about a second)."""
    table = {}
    a, b = symbols(a, table), symbols(b, table)
    if len(a) < len(b):
        a, b = b, a
    n = len(b)
    idx = np.arange(n + 1, dtype=np.int64)
    row = idx.copy()
    t = np.empty(n + 1, dtype=np.int64)
    for i in range(1, len(a) + 1):
        t[0] = i
        np.minimum(row[1:] + 1, row[:-1] + (b != a[i - 1]), out=t[1:])
        row = np.minimum.accumulate(t - idx) + idx
    return int(row[n])


def levenshtein_loops(a, b):
    """The definition, cell by cell (small inputs only)."""
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        for j in range(len(b) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
                continue
            best = D[i - 1][j - 1] + (0 if a[i - 1] == b[j - 1] else 1)
            for cand in (D[i - 1][j] + 1, D[i][j - 1] + 1):
                best = min(best, cand)
            D[i][j] = best
    return D[len(a)][len(b)]


def single_ed(gt, pred):
    """1 - distance / longer length; 0 when either string is empty."""
    if len(gt) == 0 or len(pred) == 0:
        return 0
    return 1 - levenshtein(pred, gt) / max(len(gt), len(pred))


def word_ned(list_preds, list_gts):
    """Mean over the pairs of 1 - word-level distance / larger word count (0 for a pair with an empty string)."""
    if isinstance(list_preds, str):
        list_preds = [list_preds]
    if isinstance(list_gts, str):
        list_gts = [list_gts]
    acc = 0
    for gt, pred in zip(list_gts, list_preds):
        wg, wp = gt.split(), pred.split()
        if len(gt) == 0 or len(pred) == 0:
            acc += 0
        else:
            acc += 1 - levenshtein(wg, wp) / max(len(wg), len(wp))
    return acc / float(len(list_gts))


def ngram_counts(tokens, max_n):
    tokens = list(tokens)
    return collections.Counter(tuple(tokens[i:i + n]) for n in range(1, max_n + 1) for i in range(len(tokens) - n + 1))


def bleu_sample_counts(cand, ref, max_n=4):
    """[cand_len, ref_len, clipped_1 .. clipped_max_n] of one pair."""
    both = ngram_counts(cand, max_n) & ngram_counts(ref, max_n)
    clipped = [0] * max_n
    for gram, c in both.items():
        clipped[len(gram) - 1] += c
    return [len(cand), len(ref)] + clipped


def bleu(candidates, references, max_n=4, weights=(0.25, 0.25, 0.25, 0.25)):
    """Corpus BLEU with one reference per candidate -> (score, clipped counts, total counts).  The closing expression is
    evaluated in float32 torch on the CPU like the reference's."""
    clipped, total = [0] * max_n, [0] * max_n
    cand_len, ref_len = 0.0, 0.0
    for c, r in zip(candidates, references):
        row = bleu_sample_counts(c, r, max_n)
        cand_len += row[0]
        ref_len += float(row[1])
        for i in range(max_n):
            clipped[i] += row[2 + i]
            total[i] += max(row[0] - i, 0)
    cl, to = torch.tensor(clipped, dtype=torch.float32), torch.tensor(total, dtype=torch.float32)
    if min(cl) == 0:
        return 0.0, clipped, total
    log_pn = torch.tensor(list(weights)) * torch.log(cl / to)
    score = torch.exp(sum(log_pn))
    bp = math.exp(min(1 - ref_len / cand_len, 0))
    return bp * score.item(), clipped, total
