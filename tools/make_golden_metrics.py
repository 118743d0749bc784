#!/usr/bin/env python3
"""Generate tests/golden/metrics_bleu.json and tests/golden/metrics_encode.json from the reference.

Authoring-container only (it imports the reference, like tools/make_golden_prep.py); only the recorded data is committed.

  metrics_bleu.json    seeded single-reference corpora of token-id lists with the value of the reference's
                       `bleu_score` (modules/metrics/bleu.py; tokens are handed to it as the decimal strings of the ids)
                       and the corpus `clipped_counts` / `total_counts`, formed with the reference's own
                       `_compute_ngram_counter` exactly as bleu.py:96-109 forms them.
  metrics_encode.json  labels with the `encode` outputs of TFMLabelConverter and AttnLabelConverter.

modules/metrics/ed.py cannot be imported here (python-Levenshtein is not installed), so edit distance has no recording:
the tests pin it against its definition.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_metrics.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

import numpy as np

from doc2tex.modules.converter.attn_converter import AttnLabelConverter
from doc2tex.modules.converter.tfm_converter import TFMLabelConverter
from doc2tex.modules.metrics import bleu as RB

GOLD = os.path.join(ROOT, "tests", "golden")
MAX_N = 4


def mutate(rng, seq, vocab, p):
    """A reference that shares long runs with `seq`: each token replaced, dropped or doubled with probability p / 3 each."""
    out = []
    for t in seq:
        u = rng.random()
        if u < p / 3:
            out.append(int(rng.integers(0, vocab)))
        elif u < 2 * p / 3:
            continue
        elif u < p:
            out += [t, t]
        else:
            out.append(t)
    return out


def corpora():
    rng = np.random.default_rng(20240607)
    cases = {}
    cand = [[int(t) for t in rng.integers(0, 12, size=int(rng.integers(5, 31)))] for _ in range(6)]
    cases["random_overlap"] = (cand, [mutate(rng, c, 12, 0.2) for c in cand])
    cases["identical"] = (cand[:3], [list(c) for c in cand[:3]])
    # unigrams and bigrams in common, no 4-gram: the score is exactly 0.0
    cases["zero_score"] = ([[1, 2, 3, 9, 1, 2], [4, 5, 6]], [[1, 2, 7, 3, 9, 8, 1, 2], [4, 5, 0, 6]])
    # a candidate shorter than 4 tokens (no 4-gram of its own) beside one that carries the corpus
    cases["short_candidate"] = ([[3, 4, 5], [1, 2, 3, 4, 5, 6, 7]], [[3, 4, 5], [1, 2, 3, 4, 5, 6, 8]])
    # repeated tokens: x x x y against x y is clipped to 1 + 1 unigrams; the second pair repeats a bigram
    cases["clipping"] = ([[7, 7, 7, 8], [1, 2, 1, 2, 1, 2, 3, 4, 5, 6]], [[7, 8], [1, 2, 3, 4, 5, 6, 1, 2]])
    # candidates shorter than their references: brevity penalty < 1
    long_ref = [[int(t) for t in rng.integers(0, 9, size=n)] for n in (24, 17)]
    cases["brevity"] = ([r[:n] for r, n in zip(long_ref, (15, 9))], long_ref)
    # an empty candidate and an empty reference among ordinary pairs
    cases["empty_rows"] = ([[], [1, 2, 3, 4, 5], [2, 3, 4, 5, 6, 7]], [[1, 2], [1, 2, 3, 4, 5], []])
    # one long pair over a small alphabet: many equal n-grams on both sides
    one = [int(t) for t in rng.integers(0, 4, size=120)]
    cases["long_small_alphabet"] = ([one], [mutate(rng, one, 4, 0.15)])
    return cases


def reference_counts(cand, refs):
    clipped, total = [0] * MAX_N, [0] * MAX_N
    for c, r in zip(cand, refs):
        both = RB._compute_ngram_counter(c, MAX_N) & RB._compute_ngram_counter(r, MAX_N)  # bleu.py:96-102, one reference
        for ngram, count in both.items():
            clipped[len(ngram) - 1] += count
        for i in range(MAX_N):
            total[i] += max(len(c) - i, 0)
    return clipped, total


def make_bleu():
    out = []
    for name, (cand, refs) in corpora().items():
        sc, sr = [[str(t) for t in c] for c in cand], [[str(t) for t in r] for r in refs]
        score = RB.bleu_score(sc, [[r] for r in sr])
        clipped, total = reference_counts(sc, sr)
        assert (score == 0.0) == (min(clipped) == 0)
        out.append({"name": name, "candidates": cand, "references": refs, "bleu": float(score), "clipped_counts": clipped,
                    "total_counts": total})
    by = {e["name"]: e for e in out}
    assert by["zero_score"]["bleu"] == 0.0 and by["zero_score"]["clipped_counts"][0] > 0
    assert by["identical"]["bleu"] == 1.0
    assert 0.0 < by["brevity"]["bleu"] < 1.0 and by["brevity"]["clipped_counts"] == by["brevity"]["total_counts"]
    assert by["clipping"]["clipped_counts"][0] < by["clipping"]["total_counts"][0]
    assert all(0.0 < by[n]["bleu"] < 1.0 for n in ("random_overlap", "short_candidate", "clipping", "long_small_alphabet"))
    with open(os.path.join(GOLD, "metrics_bleu.json"), "w") as f:
        json.dump({"max_n": MAX_N, "cases": out}, f, indent=1)
    print("metrics_bleu.json:", {e["name"]: e["bleu"] for e in out})


def make_encode():
    vocab = list("abcdefxyz0123456789+-=(){}^_ ") + ["\\frac", "\\mathrm", "\\alpha", "\\sqrt"]
    labels = [
        "x^{2}+y=z",                                       # characters
        ["\\frac", "{", "a", "}", "{", "b", "}"],           # word-level tokens
        "",                                                # empty label: [GO] [s]
        "a?b#c",                                           # unknown characters
        ["\\mathrm", "{", "\\unknown", "}", "[UNK]"],      # an unknown command, and the special token by name
        "0123456789abcdef",                                # 16 > batch_max_length + 1: cut to batch_max_length
        ["x"] * 13,                                        # 13 > 12: cut
        "0123456789a",                                     # 11 = batch_max_length: fits whole
        "[s]",                                             # characters of a special token's name are ordinary symbols
    ]
    bml = 11
    out = {"character": vocab, "batch_max_length": bml, "labels": labels}
    for head, cls in (("TFM", TFMLabelConverter), ("Attn", AttnLabelConverter)):
        rows, length = cls(vocab, "cpu").encode(labels, batch_max_length=bml)
        out[head] = {"text": rows.tolist(), "length": length.tolist(), "text_dtype": str(rows.dtype), "length_dtype": str(length.dtype)}
    with open(os.path.join(GOLD, "metrics_encode.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("metrics_encode.json:", len(labels), "labels")


if __name__ == "__main__":
    make_bleu()
    make_encode()
