"""GPU: d2t_metric_edit_distance and d2t_metric_bleu_counts one at a time, and the functions of doc2tex_amd.metrics above
them.  Everything the kernels return is an integer and is compared with `==` against tests/metrics_refs.py (itself checked
on the CPU by tests/test_metrics_refs_cpu.py); the floats above the integers are compared with `==` too, since the
arithmetic after the kernels is the reference's own.

Shapes: every length at which the edit-distance kernel takes another path -- an empty side, one symbol, diagonals shorter
and longer than a wave (63 / 64 / 65), around 256, longer than the block (1024 threads: 1500), the last length whose
diagonals stay in LDS and the first that goes to the workspace (4095 / 4096), 16384, and one above the cap."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import metrics_refs as MR
from conftest import GOLD
from doc2tex_amd import _lib, metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT32_MAX = 2**31 - 1


def _ed_raw(pairs, max_len=None, dist=None, workspace=True):
    """d2t_metric_edit_distance on lists of int pairs, through ctypes alone -> (return code, dist tensor)."""
    lib = _lib.require_device()
    n = len(pairs)
    a_off = np.zeros(n + 1, np.int64)
    b_off = np.zeros(n + 1, np.int64)
    a_off[1:] = np.cumsum([len(a) for a, _ in pairs])
    b_off[1:] = np.cumsum([len(b) for _, b in pairs])
    a_sym = torch.tensor([x for a, _ in pairs for x in a], dtype=torch.int32, device=DEV)
    b_sym = torch.tensor([x for _, b in pairs for x in b], dtype=torch.int32, device=DEV)
    a_off_d, b_off_d = torch.from_numpy(a_off).to(DEV), torch.from_numpy(b_off).to(DEV)
    if max_len is None:
        max_len = max([len(x) for p in pairs for x in p] + [0])
    if dist is None:
        dist = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    need = C.c_int64(0)
    ws = None
    if workspace and lib.d2t_metric_edit_distance_workspace(n, max_len, C.byref(need)) == _lib.D2T_OK and need.value:
        ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    rc = lib.d2t_metric_edit_distance(_lib.ptr(a_sym) if a_sym.numel() else None, _lib.ptr(a_off_d), a_sym.numel(),
                                      _lib.ptr(b_sym) if b_sym.numel() else None, _lib.ptr(b_off_d), b_sym.numel(),
                                      _lib.ptr(dist), n, max_len, _lib.ptr(ws), need.value if ws is not None else 0,
                                      _lib.stream_of(dist))
    torch.cuda.synchronize()
    return rc, dist


def _expect(pairs):
    return [MR.levenshtein(a, b) for a, b in pairs]


def _rand(rng, n, alphabet=4):
    return [int(x) for x in rng.integers(0, alphabet, size=n)]


def _mutated(rng, a, p=0.1, alphabet=4):
    out = []
    for x in a:
        u = rng.random()
        if u < p / 3:
            out.append(int(rng.integers(0, alphabet)))
        elif u < 2 * p / 3:
            continue
        elif u < p:
            out += [x, int(rng.integers(0, alphabet))]
        else:
            out.append(x)
    return out


def _small_pairs():
    base = [3, 1, 4, 1, 5, 9, 2, 6, 5]
    pairs = [([], []), ([], base[:5]), (base[:5], []), ([7], [7]), ([7], [8]), (base, list(base))]
    for pos in (0, len(base) // 2, len(base) - 1):
        pairs.append((base, base[:pos] + [77] + base[pos + 1:]))  # one substitution
        pairs.append((base, base[:pos] + [77] + base[pos:]))      # one insertion
        pairs.append((base, base[:pos] + base[pos + 1:]))         # one deletion
    pairs.append((base, base + [77]))                             # an insertion behind the last symbol
    pairs.append(([1, 1, 1, 1], [1, 1, 1]))                       # "aaaa" against "aaa"
    pairs.append(([1, 2, 3, 4], [1, 3, 2, 4]))                    # a transposition costs 2
    # any int32, compared as integers: above 0xFFFF, negative, the extremes; values that agree in their low 16 bits differ
    pairs.append(([0x10000, 0x1F600, -1, INT32_MAX], [0x10000, 0x1F600, -1, INT32_MAX]))
    pairs.append(([0x10000, 0x1F600, -1, INT32_MAX], [0, 0xF600, 0xFFFF, -INT32_MAX - 1]))
    pairs.append(([-5, -4, -3, INT32_MAX, 0x20000], [-5, -3, INT32_MAX, INT32_MAX - 1, 0x20000]))
    return pairs


def test_edit_distance_small_cases_in_one_launch_and_alone():
    pairs = _small_pairs()
    want = _expect(pairs)
    assert want[:6] == [0, 5, 5, 0, 1, 0] and want[6:15] == [1] * 9 and want[15:18] == [1, 1, 2] and want[18:20] == [0, 4]
    rc, dist = _ed_raw(pairs)
    assert rc == _lib.D2T_OK and dist.tolist() == want
    for i in (0, 1, 4, 7, 17):  # N = 1
        rc, dist = _ed_raw([pairs[i]])
        assert rc == _lib.D2T_OK and dist.tolist() == [want[i]]


@pytest.mark.parametrize("lengths", [(63, 64, 65), (255, 256, 257)])
def test_edit_distance_lengths_around_the_wave_and_block_sizes(lengths):
    rng = np.random.default_rng(sum(lengths))
    strings = {n: _rand(rng, n) for n in lengths}
    pairs = [(strings[x], strings[y] if x != y else _mutated(rng, strings[x])) for x in lengths for y in lengths]
    rc, dist = _ed_raw(pairs)
    assert rc == _lib.D2T_OK and dist.tolist() == _expect(pairs)


def test_edit_distance_33_mixed_pairs_and_very_different_lengths():
    rng = np.random.default_rng(33)
    lens = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1500, 1, 300, 64, 1024, 1025, 7, 100, 0, 31, 32, 33,
            127, 129, 511, 513, 2]
    assert len(lens) == 33
    pairs = []
    for k, n in enumerate(lens):
        a = _rand(rng, n)
        b = _mutated(rng, a, 0.2) if k % 3 else _rand(rng, lens[-1 - k])
        pairs.append((a, b))
    pairs[17] = (_rand(rng, 1), _rand(rng, 300))
    pairs[18] = (_rand(rng, 300), _rand(rng, 1))
    rc, dist = _ed_raw(pairs)
    assert rc == _lib.D2T_OK and dist.tolist() == _expect(pairs)


def test_edit_distance_last_lds_length_and_first_workspace_length():
    rng = np.random.default_rng(4095)
    lds = _lib.METRIC_ED_LDS_LEN
    a = _rand(rng, lds + 5)
    pairs = [(a[:lds], _mutated(rng, a)), (a[:lds + 1], _mutated(rng, a) + a[:40]), ([5], [6])]
    assert min(len(pairs[1][0]), len(pairs[1][1])) > lds  # the shorter string decides the tier
    lib = _lib.load()
    need = C.c_int64(-1)
    assert lib.d2t_metric_edit_distance_workspace(3, lds, C.byref(need)) == _lib.D2T_OK and need.value == 0
    assert lib.d2t_metric_edit_distance_workspace(3, lds + 1, C.byref(need)) == _lib.D2T_OK and need.value == 3 * 3 * (lds + 2) * 4
    rc, dist = _ed_raw(pairs)
    assert rc == _lib.D2T_OK and dist.tolist() == _expect(pairs)
    # a call that needs the workspace and does not get it launches nothing
    rc, dist = _ed_raw(pairs, workspace=False)
    assert rc == _lib.D2T_EINVAL and dist.tolist() == [-7] * 3


def test_edit_distance_16384_symbols():
    rng = np.random.default_rng(16384)
    a = _rand(rng, 16384)
    b = _mutated(rng, a, 0.3)
    b = (b + _rand(rng, 16384))[:16384]
    pairs = [(a, b)]
    want = _expect(pairs)
    assert want[0] > 1000
    rc, dist = _ed_raw(pairs)
    assert rc == _lib.D2T_OK and dist.tolist() == want


def test_edit_distance_above_the_cap_is_refused_and_nothing_is_written():
    cap = _lib.METRIC_ED_MAX_LEN
    lib = _lib.load()
    need = C.c_int64(-1)
    assert lib.d2t_metric_edit_distance_workspace(1, cap + 1, C.byref(need)) == _lib.D2T_EINVAL
    assert lib.d2t_metric_edit_distance_workspace(1, cap, C.byref(need)) == _lib.D2T_OK
    long = [1] * (cap + 1)
    dist = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    rc, dist = _ed_raw([(long, [1, 2]), ([1, 2], [1, 3])], dist=dist)
    assert rc == _lib.D2T_EINVAL and dist.tolist() == [-7, -7]
    with pytest.raises(ValueError, match="cap"):
        metrics.edit_distance(["a" * (cap + 1)], ["a"])
    # a pair longer than the max_len the caller declared is reported, never cut; the other pairs of the launch are served
    rc, dist = _ed_raw([([1, 2, 3, 4], [1, 2]), ([1, 2], [1, 3])], max_len=3)
    assert rc == _lib.D2T_OK and dist.tolist() == [-1, 1]
    rc, dist = _ed_raw([([1, 2], [1, 3]), ([4, 5, 6], [])])
    assert rc == _lib.D2T_OK and dist.tolist() == [1, 3]


def test_edit_distance_function_strings_and_words():
    a = ["kitten", "", "x^{2}", "\U0001F600a\U0001F601", "naïve", "a b c"]
    b = ["sitting", "abc", "x^{2}", "\U0001F600b\U0001F602", "naive", "a c"]
    out = metrics.edit_distance(a, b)
    assert out.dtype == torch.int32 and out.is_cuda and out.tolist() == [3, 3, 0, 2, 1, 2]
    assert out.tolist() == [MR.levenshtein(x, y) for x, y in zip(a, b)]
    # word level: lists of strings (and any other hashables) are compared item by item
    wa = [["\\frac", "{", "a", "}"], "a b c".split(), [], [("t", 1), 2, None]]
    wb = [["\\frac", "{", "ab", "}"], "a c".split(), ["x"], [("t", 1), 3, None, 2]]
    assert metrics.edit_distance(wa, wb).tolist() == [1, 1, 1, 2]
    assert metrics.edit_distance([], []).tolist() == []


def test_ned_functions_equal_the_helpers_exactly():
    pairs = [("x^{2}+y", "x^{2}-y"), ("", "abc"), ("abc", ""), ("", ""), ("\\frac { a } { b }", "\\frac { a } { c } d"),
             ("abc", "abc"), ("a", "bcdefg")]
    for gt, pred in pairs:
        got, want = metrics.get_single_ED(gt, pred), MR.single_ed(gt, pred)
        assert got == want and type(got) is type(want), (gt, pred)
        got, want = metrics.get_word_NED(pred, gt), MR.word_ned(pred, gt)
        assert got == want and isinstance(got, float), (gt, pred)
    preds, gts = [p for _, p in pairs], [g for g, _ in pairs]
    assert metrics.get_word_NED(preds, gts) == MR.word_ned(preds, gts)
    with pytest.raises(ZeroDivisionError):
        metrics.get_word_NED(" ", "  ")


# ---- BLEU counts ----------------------------------------------------------------------------------------------------
END = 2


def _bleu_raw(cand, ref, max_n=4, end=END):
    """d2t_metric_bleu_counts on two lists of equally long rows, through ctypes alone -> (return code, out tensor)."""
    lib = _lib.require_device()
    c = torch.tensor(cand, dtype=torch.int64, device=DEV)
    r = torch.tensor(ref, dtype=torch.int64, device=DEV)
    out = torch.full((c.shape[0], 2 + max_n), -7, dtype=torch.int64, device=DEV)
    rc = lib.d2t_metric_bleu_counts(_lib.ptr(c), c.shape[1], _lib.ptr(r), r.shape[1], c.shape[0], end, max_n, _lib.ptr(out),
                                    _lib.stream_of(out))
    torch.cuda.synchronize()
    return rc, out


def _cut(row, end=END):
    return row[:row.index(end)] if end in row else row


def _bleu_expect(cand, ref, max_n=4):
    return [MR.bleu_sample_counts(_cut(c), _cut(r), max_n) for c, r in zip(cand, ref)]


def test_bleu_counts_short_rows_end_token_and_clipping():
    X, Y = 10, 11
    cand = [[END, 5, 5, 5, 5, 5],       # end_token at column 0: length 0
            [5, END, 5, 5, 5, 5],       # 1
            [5, 6, END, 5, 6, 7],       # 2
            [5, 6, 7, END, END, 5],     # 3; tokens behind the first end_token do not count
            [5, 6, 7, 8, END, 9],       # 4
            [5, 6, 7, 8, 9, 5],         # no end_token: the whole row
            [X, X, X, Y, END, 0],       # clipping: x x x y against x y
            [5, 6, 7, 8, 9, END],       # a reference shorter than n
            [5, 6, 5, 6, 5, 6]]         # repeated bigrams, the reference has two of them
    ref = [[5, 5, END, 0, 0, 0, 0],
           [5, END, 0, 0, 0, 0, 0],
           [5, 6, 7, END, 0, 0, 0],
           [5, 6, 7, 8, END, 0, 0],
           [5, 6, 7, 8, END, 0, 0],
           [5, 6, 7, 8, 9, 5, 6],
           [X, Y, END, 0, 0, 0, 0],
           [5, 6, END, 0, 0, 0, 0],
           [5, 6, 5, 6, END, 0, 0]]
    want = _bleu_expect(cand, ref)
    assert [w[0] for w in want] == [0, 1, 2, 3, 4, 6, 4, 5, 6]
    assert want[6] == [4, 2, 2, 1, 0, 0] and want[7] == [5, 2, 2, 1, 0, 0] and want[8] == [6, 4, 4, 3, 2, 1]
    rc, out = _bleu_raw(cand, ref)
    assert rc == _lib.D2T_OK and out.tolist() == want
    for max_n in (1, 2, 3):
        rc, out = _bleu_raw(cand, ref, max_n)
        assert rc == _lib.D2T_OK and out.tolist() == [w[:2 + max_n] for w in want]
    rc, out = _bleu_raw(cand[6:7], ref[6:7])  # N = 1
    assert rc == _lib.D2T_OK and out.tolist() == want[6:7]


def _token_rows(n, cols, seed, vocab):
    """n candidate / reference rows `cols` wide over a small vocabulary (ids >= 3), an end_token in most rows."""
    rng = np.random.default_rng(seed)
    cand, ref = [], []
    for i in range(n):
        c = [int(x) for x in rng.integers(3, 3 + vocab, size=cols)]
        r = _mutated(rng, c, 0.2, vocab)
        r = [x + 3 if x < 3 else x for x in r]
        r = (r + [int(x) for x in rng.integers(3, 3 + vocab, size=cols)])[:cols]
        if i % 4 != 1:
            c[int(rng.integers(0, cols))] = END
        if i % 4 != 2:
            r[int(rng.integers(0, cols))] = END
        cand.append(c)
        ref.append(r)
    return cand, ref


@pytest.mark.parametrize("n,cols", [(3, 64), (3, 65), (2, 501), (70, 40), (2, 1024), (1, 2048)])
def test_bleu_counts_widths_and_batches(n, cols):
    cand, ref = _token_rows(n, cols, 100 * n + cols, 6)
    cand[0] = [x if x != END else 3 for x in cand[0]]  # one full-width row on each side
    ref[0] = [x if x != END else 3 for x in ref[0]]
    want = _bleu_expect(cand, ref)
    assert want[0][0] == cols and want[0][1] == cols and want[0][5] > 0
    rc, out = _bleu_raw(cand, ref)
    assert rc == _lib.D2T_OK and out.tolist() == want


def test_bleu_counts_refuses_what_it_does_not_serve():
    cap = _lib.METRIC_BLEU_MAX_COLS
    wide, ok = [[5] * (cap + 1)], [[5, 6, END]]
    for cand, ref, max_n in ((wide, ok, 4), (ok, wide, 4), (ok, ok, 5), (ok, ok, 0)):
        rc, out = _bleu_raw(cand, ref, max_n)
        assert rc == _lib.D2T_EINVAL and bool((out == -7).all())
    with pytest.raises(ValueError, match="2048"):
        metrics.bleu_counts(torch.tensor(wide, device=DEV), torch.tensor(ok, device=DEV), END)
    rc, out = _bleu_raw(ok, ok)  # a valid call after the refusals
    assert rc == _lib.D2T_OK and out.tolist() == [[2, 2, 2, 1, 0, 0]]


with open(os.path.join(GOLD, "metrics_bleu.json")) as _f:
    BLEU_GOLD = json.load(_f)


@pytest.mark.parametrize("case", BLEU_GOLD["cases"], ids=[c["name"] for c in BLEU_GOLD["cases"]])
def test_bleu_score_equals_the_recorded_reference(case):
    cand = [[str(t) for t in c] for c in case["candidates"]]
    refs = [[[str(t) for t in r]] for r in case["references"]]
    counts = metrics.bleu_corpus_counts(cand, refs, BLEU_GOLD["max_n"])
    assert counts == [MR.bleu_sample_counts(c, r[0]) for c, r in zip(cand, refs)]
    score, clipped, total = metrics._bleu_from_counts(counts, BLEU_GOLD["max_n"], [0.25] * 4)
    assert clipped == case["clipped_counts"] and total == case["total_counts"]
    got = metrics.bleu_score(cand, refs)
    assert got == case["bleu"] and got == score and isinstance(got, float)


def test_bleu_score_refuses_more_than_one_reference():
    with pytest.raises(ValueError, match="one reference"):
        metrics.bleu_score([["a", "b"]], [[["a", "b"], ["a"]]])
    with pytest.raises(ValueError, match="one reference"):
        metrics.bleu_score([["a", "b"]], [[]])
    assert metrics.bleu_score([], []) == 0.0
