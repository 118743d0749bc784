"""CPU: the device-side LSTM-attention beam search's interface -- its C-ABI entries in the ctypes table with the header's
argument counts, the record struct, the Engine and Model surface -- and the record-based bookkeeping rules that the GPU tests
hold the kernels to (attn_beam_refs.rec_*), checked here against a brute-force restatement that keeps whole sequences in
lists, as the host loop does."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import attn_beam_refs as AR
from doc2tex_amd import Model, _lib
from doc2tex_amd.build_model import BeamSearchHandle
from doc2tex_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["d2t_decode_attn_supports_device_beam", "d2t_set_attn_beam_device", "d2t_decode_attn_beam_device_runs",
           "d2t_decode_attn_beam_batch_submit", "d2t_op_attn_beam_advance", "d2t_op_attn_beam_finish"]


def _header():
    with open(os.path.join(ROOT, "include", "d2t.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_are_declared_bound_and_exported(name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.S)
    assert m, f"{name} is not declared in include/d2t.h"
    args = [a for a in m.group(1).split(",") if a.strip()]
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == len(args), name
    assert hasattr(_lib.load(), name)


def test_the_record_struct_matches_the_header():
    body = re.search(r"typedef struct d2t_op_attn_beam_rec \{(.*?)\} d2t_op_attn_beam_rec;", _header(), re.S).group(1)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [f[0] for f in _lib.D2TOpAttnBeamRec._fields_]
    assert C.sizeof(_lib.D2TOpAttnBeamRec) == 17 * 8 + 6 * 4
    assert set(AR.FIELDS) | {"topv", "topi"} == set(names[:17])


def test_engine_and_model_surface():
    for f in ("supports_device_attn_beam", "set_attn_beam_device", "decode_attn_beam_batch_async", "attn_beam_device_runs"):
        assert callable(getattr(Engine, f)), f
    assert callable(Model.beam_search_batch_async)
    for f in ("done", "wait", "result", "steps"):
        assert callable(getattr(BeamSearchHandle, f)), f
    h = BeamSearchHandle(None, None, (), [], False)  # what an empty list of inputs gives: nothing in flight
    assert h.done() and h.result() == [] and h.steps() == 0


def test_the_switch_is_off_by_default():
    from doc2tex_amd import synth
    assert Model(synth.make_config("TS0")).attn_beam_device is False


# (N, beam, stream seed, p([s]), the step from which every candidate is [s]): every N x beam of the issue with a stream that
# runs to the limit and one that ends everything at step 4, and three with [s] rare.  S = 12, V = 7.
S, V = 12, 7
CASES = [(N, beam) + st for N in (1, 5, 300) for beam in (1, 3, 16) for st in ((1, 0.2, None), (2, 0.2, 4))] + \
        [(1, 1, 2, 0.05, None), (5, 3, 2, 0.05, None), (300, 16, 2, 0.05, None)]
_EVENTS = set()


@pytest.mark.parametrize("N,beam,seed,p_end,end_from", CASES)
def test_record_rules_equal_the_brute_force_search(N, beam, seed, p_end, end_from):
    stream = AR.Stream(V, seed, p_end, end_from)
    want, steps, events = AR.brute_force(N, beam, S, V, stream)
    _EVENTS.update(events)
    r, rsteps, (seq, ln, score, path, plen) = AR.run_record(N, beam, S, V, stream)
    assert rsteps == steps
    assert (r.ctrl[2] != 0) == (r.ctrl[1] == 0), r.ctrl  # the stop step is set exactly when nothing is left to extend ...
    assert steps == S or r.ctrl[2] == steps, r.ctrl    # ... at the step the brute-force loop breaks at
    for i, (toks, sc, pa) in enumerate(want):
        assert seq[i, :ln[i]].tolist() == toks, (i, seq[i].tolist(), toks)
        assert (seq[i, ln[i]:] == 0).all()
        assert np.float32(sc).view(np.int32) == score[i].view(np.int32), (i, sc, score[i])
        assert plen[i] == ln[i] and path[i, :plen[i]].tolist() == pa, (i, path[i].tolist(), pa)
        assert (path[i, plen[i]:] == AR.ICAN).all()
    assert (r.comp_n <= beam).all() and (r.comp_n >= 0).all()  # completions never exceed beam: each lowers the sample's k


def test_the_streams_hold_every_situation_the_issue_names():
    if len(_EVENTS) == 0:  # (run alone: gather them)
        for N, beam, seed, p_end, end_from in CASES:
            _EVENTS.update(AR.brute_force(N, beam, S, V, AR.Stream(V, seed, p_end, end_from))[2])
    assert _EVENTS >= {"a sample finishes while others continue", "all samples finish at one step",
                       "nothing completed at the last step", "the limit is reached with survivors",
                       "two completed hypotheses of different lengths tie at the best score / len"}, _EVENTS


def test_a_stopped_record_is_left_alone():
    stream = AR.Stream(V, 2, 0.2, 4)
    r, steps, _ = AR.run_record(5, 3, S, V, stream)
    assert steps == 5 and r.ctrl.tolist() == [5, 0, 5, 5]
    before = {f: getattr(r, f).copy() for f in AR.FIELDS}
    AR.rec_advance(r, *AR.candidates(r, stream))
    assert all(np.array_equal(before[f], getattr(r, f)) for f in AR.FIELDS)
