"""CPU: the host references of tests/metrics_refs.py against independent values (the reference's recorded BLEU numbers in
tests/golden/metrics_bleu.json, a cell-by-cell DP), `LabelDecoder.encode` against the reference converters' recorded
outputs (tests/golden/metrics_encode.json), and the no-GPU behaviour of doc2tex_amd.metrics / doc2tex_amd.validate."""
import json
import os
import random

import pytest
import torch

import metrics_refs as MR
from conftest import GOLD
from doc2tex_amd import _lib
from doc2tex_amd.postprocess import LabelDecoder


def bleu_golden():
    with open(os.path.join(GOLD, "metrics_bleu.json")) as f:
        return json.load(f)


def encode_golden():
    with open(os.path.join(GOLD, "metrics_encode.json")) as f:
        return json.load(f)


BLEU_CASES = bleu_golden()["cases"]


def test_bleu_fixture_covers_the_edge_cases():
    by = {c["name"]: c for c in BLEU_CASES}
    assert any(c["bleu"] == 0.0 and c["clipped_counts"][0] > 0 for c in BLEU_CASES)  # a zero from one empty order
    assert any(len(x) < 4 for c in BLEU_CASES for x in c["candidates"])
    assert by["clipping"]["candidates"][0] == [7, 7, 7, 8] and by["clipping"]["references"][0] == [7, 8]
    b = by["brevity"]  # every n-gram matches, so the score is the brevity penalty alone
    assert b["clipped_counts"] == b["total_counts"] and 0.0 < b["bleu"] < 1.0


@pytest.mark.parametrize("case", BLEU_CASES, ids=[c["name"] for c in BLEU_CASES])
def test_helper_bleu_equals_the_recorded_reference(case):
    score, clipped, total = MR.bleu(case["candidates"], case["references"], bleu_golden()["max_n"])
    assert clipped == case["clipped_counts"]
    assert total == case["total_counts"]
    assert score == case["bleu"]


def test_helper_levenshtein_equals_the_definition():
    rng = random.Random(7)
    for _ in range(400):
        alphabet = rng.choice([2, 3, 5])
        a = [rng.randrange(alphabet) for _ in range(rng.randrange(0, 13))]
        b = [rng.randrange(alphabet) for _ in range(rng.randrange(0, 13))]
        assert MR.levenshtein(a, b) == MR.levenshtein_loops(a, b), (a, b)
    assert MR.levenshtein("kitten", "sitting") == 3
    assert MR.levenshtein("", "abc") == 3 and MR.levenshtein("abc", "") == 3 and MR.levenshtein("", "") == 0
    assert MR.levenshtein(["a", "bc"], ["a", "b", "c"]) == 2  # word level: items are compared whole


def test_helper_ned_edge_cases():
    assert MR.single_ed("", "abc") == 0 and MR.single_ed("abc", "") == 0
    assert MR.single_ed("abcd", "abcd") == 1.0
    assert MR.single_ed("abcd", "abxd") == 1 - 1 / 4
    assert MR.word_ned("a b c", "a x c") == 1 - 1 / 3
    assert MR.word_ned(["a b", ""], ["a b", "c"]) == (1.0 + 0) / 2.0
    with pytest.raises(ZeroDivisionError):
        MR.word_ned(" ", "  ")


@pytest.mark.parametrize("head", ["TFM", "Attn"])
def test_label_decoder_encode_equals_the_reference_converters(head):
    g = encode_golden()
    dec = LabelDecoder(g["character"], head)
    rows, length = dec.encode(g["labels"], batch_max_length=g["batch_max_length"])
    assert str(rows.dtype) == g[head]["text_dtype"] and str(length.dtype) == g[head]["length_dtype"]
    assert rows.tolist() == g[head]["text"]
    assert length.tolist() == g[head]["length"]
    assert rows.device.type == "cpu"
    # the fixture holds what the issue asks for: a cut label, an unknown token
    assert any(n > g["batch_max_length"] + 1 for n in g[head]["length"])
    assert any(dec.dict["[UNK]"] in r[1:] for r in g[head]["text"])
    # dict: token -> index, specials first
    assert [dec.dict[t] for t in dec.character] == list(range(len(dec.character)))
    assert dec.dict["[s]"] == (2 if head == "TFM" else 1)
    # default batch_max_length is the converters' 25
    assert dec.encode(["ab"])[0].shape == (1, 27)
    # a label of exactly batch_max_length + 1 tokens does not fit its row, as in the reference
    with pytest.raises(RuntimeError):
        dec.encode(["a" * 4], batch_max_length=3)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour WITHOUT a GPU")
def test_metrics_and_validate_import_without_a_gpu_and_calls_fail_loudly():
    from doc2tex_amd import metrics, validate

    _lib.load()
    calls = [
        lambda: metrics.edit_distance(["abc"], ["abd"]),
        lambda: metrics.get_single_ED("abc", "abd"),
        lambda: metrics.get_single_ED("", "abd"),
        lambda: metrics.get_word_NED("a b", "a c"),
        lambda: metrics.bleu_score([["a", "b"]], [[["a", "b"]]]),
        lambda: metrics.ValidationMetrics(2),
        lambda: validate.validation_step(None, None, None, [], None, {"Prediction": {"name": "TFM"}}, None, "cuda"),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
