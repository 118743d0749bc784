"""CPU: the device-side LSTM-attention beam search's interface -- its C-ABI entries in the ctypes table with the header's
argument counts, the record struct, the Engine and Model surface -- and the record-based bookkeeping rules that the GPU tests
hold the kernels to (attn_beam_refs.rec_*), checked here against a brute-force restatement that keeps whole sequences in
lists; and the host loop's bookkeeping (csrc/attn_beam_host.h), run through its two device-free operators and held to the
same rules array for array."""
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
           "d2t_decode_attn_beam_batch_submit", "d2t_op_attn_beam_advance", "d2t_op_attn_beam_finish",
           "d2t_op_attn_beam_host_advance", "d2t_op_attn_beam_host_finish"]


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


# =====================================================================================================================
# the host loop's bookkeeping (csrc/attn_beam_host.h) through its operators: no device, every array a numpy array
# =====================================================================================================================
D2T_EINVAL = 1  # include/d2t.h


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


class HostRec:
    """a canary-filled record in host memory, laid out as the reference record `r`"""

    def __init__(self, r):
        self.t = {f: getattr(r, f).copy() for f in AR.FIELDS}
        self.topv = np.full((r.N, r.beam), AR.FCAN, np.float32)
        self.topi = np.full((r.N, r.beam), AR.ICAN, np.int32)
        self.a = a = _lib.D2TOpAttnBeamRec()
        for f in AR.FIELDS:
            setattr(a, f, self.t[f].ctypes.data)
        a.topv, a.topi = self.topv.ctypes.data, self.topi.ctypes.data
        a.N, a.beam, a.cap, a.V, a.S, a.end_token = r.N, r.beam, r.cap, r.V, r.S, AR.END

    def advance(self, init=False, cands=None):
        if cands is not None:
            self.topv[...], self.topi[...] = cands
        return _lib.load().d2t_op_attn_beam_host_advance(C.byref(self.a), int(init), 0)

    def finish(self, with_path=True):
        N, Sx = self.a.N, self.a.S
        out = [np.full((N, Sx), AR.ICAN, np.int64), np.full(N, AR.ICAN, np.int32), np.full(N, AR.FCAN, np.float32),
               np.full((N, Sx), AR.ICAN, np.int32), np.full(N, AR.ICAN, np.int32)]
        ptr = [o.ctypes.data for o in out]
        rc = _lib.load().d2t_op_attn_beam_host_finish(C.byref(self.a), ptr[0], ptr[1], ptr[2], ptr[3] if with_path else None,
                                                      ptr[4] if with_path else None)
        return rc, out

    def differs_from(self, r):
        """names of the arrays that are not the reference's, bit for bit (canaries included)"""
        return [f for f in AR.FIELDS if not np.array_equal(_bits(self.t[f]), _bits(getattr(r, f)))]


@pytest.mark.parametrize("N,beam,seed,p_end,end_from", CASES)
def test_host_operator_chain_equals_the_record_rules(N, beam, seed, p_end, end_from):
    """init, S chained steps of the host loop's bookkeeping (those behind the stop step included: they must leave the record
    alone) and its final pick: every array of the record after every step, and every output of finish, is the reference's --
    integers exactly, floats by their bits, canaries where nothing is to be written (cap > N x beam)."""
    stream = AR.Stream(V, seed, p_end, end_from)
    r = AR.Rec(N, beam, S, V, cap=N * beam + 3)
    h = HostRec(r)
    assert h.advance(init=True) == 0
    AR.rec_init(r)
    assert h.differs_from(r) == [], "after init"
    for step in range(S):
        cands = AR.candidates(r, stream)
        assert h.advance(cands=cands) == 0, f"step {step}"
        AR.rec_advance(r, *cands)
        assert h.differs_from(r) == [], f"after step {step}"
    want = AR.rec_finish(r)
    rc, got = h.finish()
    assert rc == 0
    for name, g, w in zip(("seq", "len", "score", "path", "plen"), got, want):
        assert np.array_equal(_bits(g), _bits(w)), f"finish: {name}"
    rc, got = h.finish(with_path=False)
    assert rc == 0
    assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got[:3], want[:3]))
    assert (got[3] == AR.ICAN).all() and (got[4] == AR.ICAN).all()
    assert h.differs_from(r) == [], "finish writes nothing into the record"


def test_host_operators_leave_a_stopped_record_alone():
    stream = AR.Stream(V, 2, 0.2, 4)
    r = AR.Rec(5, 3, S, V, cap=5 * 3 + 3)
    h = HostRec(r)
    assert h.advance(init=True) == 0
    AR.rec_init(r)
    for _ in range(5):
        cands = AR.candidates(r, stream)
        assert h.advance(cands=cands) == 0
        AR.rec_advance(r, *cands)
    assert h.t["ctrl"].tolist() == [5, 0, 5, 5] and h.differs_from(r) == []
    poison = (np.full((5, 3), AR.FCAN, np.float32), np.full((5, 3), 1 << 30, np.int32))
    assert h.advance(cands=poison) == 0
    assert h.differs_from(r) == []


def test_host_operator_refusals_write_nothing():
    """what test_operator_refusals_write_nothing asks of the device operators"""
    stream = AR.Stream(V, 1)
    r = AR.Rec(5, 3, S, V)
    h = HostRec(r)
    lib = _lib.load()
    for field, value in (("N", 0), ("beam", 0), ("beam", 17), ("cap", 14), ("V", 0), ("S", 0), ("end_token", V), ("seg", None),
                         ("hist_tok", None), ("last_completed", None)):
        keep = getattr(h.a, field)
        setattr(h.a, field, value)
        assert h.advance(init=True) == D2T_EINVAL, (field, value)
        assert h.finish()[0] == D2T_EINVAL, (field, value)
        setattr(h.a, field, keep)
    assert lib.d2t_op_attn_beam_host_advance(None, 1, 0) == D2T_EINVAL
    assert h.differs_from(r) == []
    assert h.advance(init=True) == 0
    AR.rec_init(r)
    topv, topi = AR.candidates(r, stream)
    for bad in (-1, V, 3 * V):  # a candidate of a row the segment does not rank (step 0 ranks one row)
        t2 = topi.copy()
        t2[2, 1] = bad
        assert h.advance(cands=(topv, t2)) == D2T_EINVAL, bad
    h.t["ctrl"][0] = S  # a step beyond the history
    assert h.advance(cands=(topv, topi)) == D2T_EINVAL
    h.t["ctrl"][0] = 0
    assert h.differs_from(r) == []
    h.t["last_completed"][1] = 1  # "completed" with an empty completed set
    rc, out = h.finish()
    assert rc == D2T_EINVAL
    assert all((o == (AR.FCAN if o.dtype == np.float32 else AR.ICAN)).all() for o in out)
    h.t["last_completed"][1] = 0
    assert h.advance(cands=(topv, topi)) == 0
    AR.rec_advance(r, topv, topi)
    assert h.differs_from(r) == []


def test_host_operators_have_no_sample_limit():
    """N = 1025 is beyond the kernels' 1024 samples; the host functions take it (the uniform entries of the host loop do)"""
    stream = AR.Stream(V, 1, 0.2, 2)
    r = AR.Rec(1025, 2, 4, V)
    h = HostRec(r)
    assert h.advance(init=True) == 0
    AR.rec_init(r)
    for _ in range(4):
        cands = AR.candidates(r, stream)
        assert h.advance(cands=cands) == 0
        AR.rec_advance(r, *cands)
    assert h.differs_from(r) == []
    rc, got = h.finish()
    assert rc == 0 and all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, AR.rec_finish(r)))
