"""GPU: the LSTM-attention beam search with its bookkeeping on the device (attn_beam.hip, engine_attn.hip
attn_beam_dev_impl): the operators against the record rules of attn_beam_refs (every integer and every float bit, canaries
included), the search against the host loop of the same build (sequence, length, score bits, alignment-map bits), the models
of test_ragged_attn_beam_gpu through Model.attn_beam_device and Model.beam_search_batch_async, submitted searches in flight
beside a greedy decode, the refusals, and the switch (off: the host loop runs, read from the context's run counter).

Nothing here has a tolerance: the device-side search runs the host loop's kernels per row and restates its integer
bookkeeping, so every comparison is for equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_beam_refs as AR
import test_attn_vocab_gpu as vocab
import test_ragged_attn_beam_gpu as rag
from conftest import engine_model
from doc2tex_amd import Model, _lib, synth
from doc2tex_amd.engine import pack_memories
from test_attn_beam_device_cpu import CASES, S, V
from test_parity_gpu import _case

pytestmark = pytest.mark.gpu
DEV = "cuda"
D2T_EINVAL, D2T_ESTATE = 1, 4  # include/d2t.h
H = 256


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# =====================================================================================================================
# 1. the operators
# =====================================================================================================================
class DevRec:
    """a canary-filled record on the device, laid out as the reference record `r`"""

    def __init__(self, r):
        self.t = {f: torch.from_numpy(getattr(r, f).copy()).to(DEV) for f in AR.FIELDS}
        self.topv = torch.full((r.N, r.beam), float(AR.FCAN), device=DEV)
        self.topi = torch.full((r.N, r.beam), AR.ICAN, dtype=torch.int32, device=DEV)
        self.a = a = _lib.D2TOpAttnBeamRec()
        for f in AR.FIELDS:
            setattr(a, f, self.t[f].data_ptr())
        a.topv, a.topi = self.topv.data_ptr(), self.topi.data_ptr()
        a.N, a.beam, a.cap, a.V, a.S, a.end_token = r.N, r.beam, r.cap, r.V, r.S, AR.END

    def advance(self, init=False, cands=None):
        if cands is not None:
            self.topv.copy_(torch.from_numpy(cands[0]))
            self.topi.copy_(torch.from_numpy(cands[1]))
        rc = _lib.require_device().d2t_op_attn_beam_advance(C.byref(self.a), int(init), 0, _stream())
        torch.cuda.synchronize()
        return rc

    def finish(self, with_path=True):
        N, Sx = self.a.N, self.a.S
        seq = torch.full((N, Sx), AR.ICAN, dtype=torch.int64, device=DEV)
        ln = torch.full((N,), AR.ICAN, dtype=torch.int32, device=DEV)
        score = torch.full((N,), float(AR.FCAN), device=DEV)
        path = torch.full((N, Sx), AR.ICAN, dtype=torch.int32, device=DEV)
        plen = torch.full((N,), AR.ICAN, dtype=torch.int32, device=DEV)
        rc = _lib.require_device().d2t_op_attn_beam_finish(C.byref(self.a), seq.data_ptr(), ln.data_ptr(), score.data_ptr(),
                                                          path.data_ptr() if with_path else None,
                                                          plen.data_ptr() if with_path else None, _stream())
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy() for t in (seq, ln, score, path, plen)]

    def differs_from(self, r):
        """names of the arrays that are not the reference's, bit for bit (canaries included)"""
        return [f for f in AR.FIELDS if not np.array_equal(_bits(self.t[f].cpu().numpy()), _bits(getattr(r, f)))]


@pytest.mark.parametrize("N,beam,seed,p_end,end_from", CASES)
def test_operator_chain_equals_the_record_rules(N, beam, seed, p_end, end_from):
    """init, S chained advance steps (those behind the stop step included: they must leave the record alone) and finish on
    the CPU test's candidate streams: every array of the record after every step, and every output of finish, is the
    reference's -- integers exactly, floats by their bits, canaries where nothing is to be written (cap > N x beam).
    N = 300 puts samples on the second pass of the advance kernel's 256 threads."""
    stream = AR.Stream(V, seed, p_end, end_from)
    r = AR.Rec(N, beam, S, V, cap=N * beam + 5)
    d = DevRec(r)
    assert d.advance(init=True) == 0
    AR.rec_init(r)
    assert d.differs_from(r) == [], "after init"
    for step in range(S):
        cands = AR.candidates(r, stream)
        assert d.advance(cands=cands) == 0, f"step {step}"
        AR.rec_advance(r, *cands)
        assert d.differs_from(r) == [], f"after step {step}"
    want = AR.rec_finish(r)
    rc, got = d.finish()
    assert rc == 0
    for name, g, w in zip(("seq", "len", "score", "path", "plen"), got, want):
        assert np.array_equal(_bits(g), _bits(w)), f"finish: {name}"
    rc, got = d.finish(with_path=False)
    assert rc == 0
    assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got[:3], want[:3]))
    assert (got[3] == AR.ICAN).all() and (got[4] == AR.ICAN).all()
    assert d.differs_from(r) == [], "finish writes nothing into the record"


def test_operator_refusals_write_nothing():
    stream = AR.Stream(V, 1)
    r = AR.Rec(5, 3, S, V)
    d = DevRec(r)
    lib = _lib.require_device()
    for field, value in (("N", 0), ("N", 1025), ("beam", 0), ("beam", 17), ("cap", 14), ("V", 0), ("S", 0), ("end_token", V),
                         ("seg", None), ("hist_tok", None), ("last_completed", None)):
        keep = getattr(d.a, field)
        setattr(d.a, field, value)
        assert d.advance(init=True) == D2T_EINVAL, (field, value)
        assert d.finish()[0] == D2T_EINVAL, (field, value)
        setattr(d.a, field, keep)
    assert lib.d2t_op_attn_beam_advance(None, 1, 0, _stream()) == D2T_EINVAL
    assert d.differs_from(r) == []
    assert d.advance(init=True) == 0
    AR.rec_init(r)
    topv, topi = AR.candidates(r, stream)
    for bad in (-1, V, 3 * V):  # a candidate of a row the segment does not rank (step 0 ranks one row)
        t2 = topi.copy()
        t2[2, 1] = bad
        assert d.advance(cands=(topv, t2)) == D2T_EINVAL, bad
    d.t["ctrl"][0] = S  # a step beyond the history
    assert d.advance(cands=(topv, topi)) == D2T_EINVAL
    d.t["ctrl"][0] = 0
    assert d.differs_from(r) == []
    d.t["last_completed"][1] = 1  # "completed" with an empty completed set
    assert d.finish()[0] == D2T_EINVAL
    d.t["last_completed"][1] = 0
    assert d.advance(cands=(topv, topi)) == 0
    AR.rec_advance(r, topv, topi)
    assert d.differs_from(r) == []


# =====================================================================================================================
# 2. the search, against the host loop of the same build
# =====================================================================================================================
def _host_and_device(eng, fn, what):
    """fn() with the switch off and on: the results, equal; and the run counter says which loop ran"""
    runs = eng.attn_beam_device_runs()
    host = fn()
    assert eng.attn_beam_device_runs() == runs, f"{what}: the switch is off, the device-side loop ran"
    eng.set_attn_beam_device(True)
    try:
        dev = fn()
        assert eng.attn_beam_device_runs() == runs + 1, f"{what}: the switch is on, the device-side loop did not run"
    finally:
        eng.set_attn_beam_device(False)
    rag._same(dev, host, what)
    return host


@pytest.mark.parametrize("beam", [1, 3, 16])
def test_ragged_search_equals_the_host_loop(beam):
    """Tk = 1, Tk below the taps, a 1024-strided loop going round twice; with and without maps; the list reversed"""
    eng = rag._engine().engine()
    assert eng.supports_device_attn_beam()
    mems = rag._synthetic(rag.SEARCH_T, 5)
    for ms, tag in ((mems, ""), (mems[::-1], " reversed")):
        packed, lengths = pack_memories(ms)
        plain = _host_and_device(eng, lambda: eng.decode_attn_beam_batch_ragged(packed, lengths, beam), f"beam {beam}{tag}")
        maps = _host_and_device(eng, lambda: eng.decode_attn_beam_batch_ragged(packed, lengths, beam, return_alpha=True),
                                f"beam {beam}{tag} with maps")
        rag._same([g[:2] for g in maps], plain, "maps change nothing")


def test_one_sample_and_the_uniform_entries():
    eng = rag._engine().engine()
    one = torch.randn(1, 261, H, generator=torch.Generator().manual_seed(262)).to(DEV)
    _host_and_device(eng, lambda: eng.decode_attn_beam_batch_ragged(one.reshape(-1, H), [261], 3, return_alpha=True), "N = 1, T = 261")
    mem = torch.randn(4, 17, H, generator=torch.Generator().manual_seed(21)).to(DEV)
    _host_and_device(eng, lambda: eng.decode_attn_beam_batch(mem, 5), "d2t_decode_attn_beam_batch")
    _host_and_device(eng, lambda: eng.decode_attn_beam_batch(mem, 5, return_alpha=True), "d2t_decode_attn_beam_batch_alpha")
    _host_and_device(eng, lambda: [eng.decode_attn_beam(one, 5)], "d2t_decode_attn_beam")


def _wide_model():
    cfg = vocab._cfg("TS0", 1025, 8, beam_size=3)
    return vocab._model(cfg, vocab._seeded(cfg, end_bias=0.3))


@pytest.mark.parametrize("name", ["TB0", "TO0", "C0", "TS0 with 1025 classes"])
def test_other_cells_keys_and_the_wide_vocabulary(name):
    """Bahdanau with one-hot targets and a zero initial state; one-hot targets; init_mode mean over v1 keys; the wide build"""
    m = _wide_model() if name.startswith("TS0") else engine_model(name, 8, 1234, 0.3, beam_size=3)[1]
    eng = m.engine()
    assert eng.supports_device_attn_beam()
    packed, lengths = pack_memories(rag._synthetic([6, 40, 2], 31))
    _host_and_device(eng, lambda: eng.decode_attn_beam_batch_ragged(packed, lengths, 3, return_alpha=True), name)


# =====================================================================================================================
# 3. the models
# =====================================================================================================================
@pytest.mark.parametrize("name,fixture,eb,crops,kind", rag.MODEL_CASES)
def test_models_through_the_switch_and_the_async_call(cases, name, fixture, eb, crops, kind):
    c = _case(cases, "attn_beam", fixture)
    beam = c["beam_size"]
    m = rag._engine(name, c["max_seq_len"], c["end_bias"] if eb is None else eb, beam)
    imgs = [synth.synth_images(n, Hh, Ww, seed=4100 + i) for i, (n, Hh, Ww) in enumerate(crops)]
    imgs[0][:1] = synth.synth_images(1, c["H"], c["W"], seed=c["iseed"])
    imgs = [x.cuda() for x in imgs]
    eng = m.engine()
    with torch.no_grad():
        want, wmaps = m.beam_search_batch(imgs, beam), m.beam_search_batch(imgs, beam, return_attn=True)
        wone = m.beam_search_batch(imgs[0], beam, return_attn=True)
        runs = eng.attn_beam_device_runs()
        m.attn_beam_device = True
        try:
            got, gmaps = m.beam_search_batch(imgs, beam), m.beam_search_batch(imgs, beam, return_attn=True)
            gone = m.beam_search_batch(imgs[0], beam, return_attn=True)
            assert m.engine().attn_beam_device_runs() == runs + 3
        finally:
            m.attn_beam_device = False
        m.engine()
        h = m.beam_search_batch_async(imgs, beam)
        hm = m.beam_search_batch_async(tuple(imgs), beam, return_attn=True)
        h1 = m.beam_search_batch_async(imgs[0], beam, return_attn=True)
        assert m.beam_search_batch_async([], beam).result() == []
    rag._same(got, want, f"{name} {kind}: switch")
    rag._same(gmaps, wmaps, f"{name} {kind}: switch, maps")
    rag._same(gone, wone, f"{name} {kind}: switch, one tensor")
    rag._same(h.result(), want, f"{name} {kind}: async")
    rag._same(hm.result(), wmaps, f"{name} {kind}: async, maps")
    rag._same(h1.result(), wone, f"{name} {kind}: async, one tensor")
    assert h.done() and hm.done() and 1 <= h.steps() <= c["max_seq_len"] + 1
    if eb is None:  # the reference's own result for the sample in row 0
        for res in (got, h.result()):
            assert res[0][0][0].tolist() == c["seq"], (res[0][0].tolist(), c["seq"])
            assert abs(float(res[0][1]) - c["score"]) <= 1e-3, (float(res[0][1]), c["score"])


def test_model_async_names_what_it_cannot_do(monkeypatch):
    _, mt = engine_model("T2", 12, 1234, 1.8, beam_size=3)
    img = synth.synth_images(1, 48, 64, seed=1).cuda()
    with pytest.raises(NotImplementedError, match="TFM"):
        mt.beam_search_batch_async(img, 3)
    cfg = synth.make_config("TS0", device=DEV, max_seq_len=6, beam_size=3)
    cfg["Prediction"]["params"]["attn_type"] = "loc_aware"
    ml = Model(cfg).to(DEV).eval()
    ml.attn_beam_device = True  # ignored where the head has no such search
    assert not ml.engine().supports_device_attn_beam()
    with pytest.raises(NotImplementedError, match="loc_aware"):
        ml.beam_search_batch_async(img, 3)
    m = rag._engine()
    monkeypatch.setattr(_lib, "ATTN_MAP_BUDGET", 1024)
    ticket = int(m.engine().lib.d2t_decode_last_ticket(m.engine().ctx))
    with pytest.raises(RuntimeError, match="budget"), torch.no_grad():
        m.beam_search_batch_async([img, img], 3, return_attn=True)
    assert int(m.engine().lib.d2t_decode_last_ticket(m.engine().ctx)) == ticket  # nothing was submitted


# =====================================================================================================================
# 4. submitted searches
# =====================================================================================================================
def _results(eng, out, lengths, maps):
    """what decode_attn_beam_batch_ragged returns, from the tensors of decode_attn_beam_batch_async (complete by now)"""
    seq, n, score = (t.cpu() for t in out[:3])
    res = [(seq[i, :int(n[i])].unsqueeze(0), score[i]) for i in range(len(lengths))]
    if maps:
        res = [r + (out[3][i, :int(n[i]), :eng.attn_keys(T)],) for i, (r, T) in enumerate(zip(res, lengths))]
    for i in range(len(lengths)):
        assert bool((seq[i, int(n[i]):] == 0).all()), "tokens beyond a sample's length are zeros"
    return res


def _busy(ms=20):
    """about `ms` milliseconds of work on the current stream: a submitted search is ordered behind it"""
    x = torch.randn(4096, 4096, device=DEV)
    for _ in range(ms):
        x = (x @ x).clamp_(-1, 1)
    return x


def test_two_searches_and_a_greedy_decode_in_flight():
    """two chains: search A (maps), a greedy decode, search B -- all three submitted behind ~20 ms of work on the caller's
    stream, so none has completed when the calls return (done() is false without anything blocking); each equals its
    synchronous call.  decode_steps of a beam-1 search equals the host loop's step count, which for beam 1 is the longest
    returned sequence (a sample leaves the loop exactly when its one hypothesis emits [s]); for wider beams the results do not
    determine it and it is bounded: the longest result <= steps <= S."""
    m = rag._engine()
    m.decode_chains = 2
    try:
        eng = m.engine()
        Sx = eng.cfg.batch_max_length + 1
        A, B1 = rag._synthetic(rag.SEARCH_T, 5), rag._synthetic([40, 7, 300, 9], 6)
        pa, la = pack_memories(A)
        pb, lb = pack_memories(B1)
        gm = torch.randn(6, 300, H, generator=torch.Generator().manual_seed(9)).to(DEV)
        want_a = eng.decode_attn_beam_batch_ragged(pa, la, 3, return_alpha=True)
        want_b = eng.decode_attn_beam_batch_ragged(pb, lb, 1)
        tok_sync, probs_sync = eng.decode_attn_greedy(gm, False)

        def submit_all():
            return (eng.decode_attn_beam_batch_async(pa, la, 3, return_alpha=True), eng.decode_attn_greedy_async(gm, False),
                    eng.decode_attn_beam_batch_async(pb, lb, 1))
        for _ in range(2):  # the chains take turns: after two rounds each has its buffers and graphs for A and for B
            submit_all()
        eng.decode_wait(host_sync=True)
        keep = _busy()
        out_a, (tok, probs, tg), out_b = submit_all()
        first_look = [eng.ticket_done(out_a[-1]), eng.ticket_done(tg), eng.ticket_done(out_b[-1])]
        assert out_a[-1] < tg < out_b[-1]
        eng.wait_ticket(out_b[-1], host_sync=True)
        eng.wait_ticket(tg, host_sync=True)
        eng.wait_ticket(out_a[-1], host_sync=True)
        assert first_look == [False, False, False], first_look
        assert eng.ticket_done(out_a[-1]) and eng.ticket_done(tg) and eng.ticket_done(out_b[-1])
        rag._same(_results(eng, out_a, la, True), want_a, "submitted A")
        rag._same(_results(eng, out_b, lb, False), want_b, "submitted B")
        assert torch.equal(tok, tok_sync) and rag.rops._same(probs.cpu(), probs_sync.cpu())
        steps_a, steps_b = eng.decode_steps(out_a[-1]), eng.decode_steps(out_b[-1])
        assert len(steps_a) == 1 and len(steps_b) == 1
        assert steps_b[0] == max(r[0].shape[1] for r in want_b), (steps_b, [r[0].shape[1] for r in want_b])
        assert max(r[0].shape[1] for r in want_a) <= steps_a[0] <= Sx
        del keep
        # the synchronous searches still work beside the chains, on either loop
        _host_and_device(eng, lambda: eng.decode_attn_beam_batch_ragged(pb, lb, 3), "after the submitted searches")
    finally:
        m.decode_chains = 1
        m.engine()


def test_another_mix_of_lengths_replays_the_graph_and_workspaces_are_reused():
    eng = rag._engine().engine()
    first, second = rag._synthetic([9, 30, 2, 200, 9], 40), rag._synthetic([12, 100, 5, 3, 90], 41)  # Tk <= 256 both
    want = [eng.decode_attn_beam_batch_ragged(*pack_memories(ms), 3, return_alpha=True) for ms in (first, second)]
    p1, l1 = pack_memories(first)
    out = eng.decode_attn_beam_batch_async(p1, l1, 3, return_alpha=True)
    eng.wait_ticket(out[-1], host_sync=True)
    graphs = eng.graph_count()
    assert graphs >= 1
    rag._same(_results(eng, out, l1, True), want[0], "first mix")
    p2, l2 = pack_memories(second)
    out = eng.decode_attn_beam_batch_async(p2, l2, 3, return_alpha=True)
    eng.wait_ticket(out[-1], host_sync=True)
    rag._same(_results(eng, out, l2, True), want[1], "second mix")
    assert eng.graph_count() == graphs, "another mix of lengths with the same N, beam and stride capacity captured a new graph"
    # workspace reuse: large, small, large again
    big, small = rag._synthetic([700, 40, 1030], 7), rag._synthetic([3, 5], 8)
    wb = eng.decode_attn_beam_batch_ragged(*pack_memories(big), 3, return_alpha=True)
    ws = eng.decode_attn_beam_batch_ragged(*pack_memories(small), 3, return_alpha=True)
    for ms, w, what in ((big, wb, "large"), (small, ws, "small after large"), (big, wb, "large again")):
        p, l = pack_memories(ms)
        out = eng.decode_attn_beam_batch_async(p, l, 3, return_alpha=True)
        eng.wait_ticket(out[-1], host_sync=True)
        rag._same(_results(eng, out, l, True), w, what)


# =====================================================================================================================
# 5. refusals
# =====================================================================================================================
def _submit(eng, packed, Ts, beam, N=None, alpha=None, host_seq=False):
    """the raw entry on canary-filled outputs: rc, message, and whether everything is as it was"""
    n = len(Ts) if N is None else N
    Sx = eng.cfg.batch_max_length + 1
    k = max(n, 1)
    seq = torch.full((k, Sx), AR.ICAN, dtype=torch.int64, device="cpu" if host_seq else DEV)
    ln = torch.full((k,), AR.ICAN, dtype=torch.int32, device=DEV)
    score = torch.full((k,), float(AR.FCAN), device=DEV)
    ticket, runs = int(eng.lib.d2t_decode_last_ticket(eng.ctx)), eng.attn_beam_device_runs()
    t = C.c_int64(-5)
    rc = eng.lib.d2t_decode_attn_beam_batch_submit(eng.ctx, _lib.ptr(packed), n, (C.c_int32 * max(len(Ts), 1))(*Ts), beam,
                                                   _lib.ptr(seq), _lib.ptr(ln), _lib.ptr(score), _lib.ptr(alpha),
                                                   _lib.stream_of(packed), C.byref(t))
    msg = eng.lib.d2t_last_error(eng.ctx).decode()
    torch.cuda.synchronize()
    intact = bool((seq == AR.ICAN).all()) and bool((ln == AR.ICAN).all()) and bool((score == float(AR.FCAN)).all()) and \
        t.value == -5 and int(eng.lib.d2t_decode_last_ticket(eng.ctx)) == ticket and eng.attn_beam_device_runs() == runs
    return rc, msg, intact


def test_submit_refusals_enqueue_nothing_and_leave_the_context_usable():
    eng = rag._engine().engine()
    assert eng.cfg.attn_keys == _lib.ATTN_KEYS_NOCLS_INIT_CLS  # Attnv2 behind a ViT: T = Tk + 1
    packed = torch.randn(4200, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    Sx = eng.cfg.batch_max_length + 1
    assert Sx * 70 * 16 * 4096 * 4 > _lib.ATTN_MAP_BUDGET
    alpha = torch.full((16,), float(AR.FCAN), device=DEV)
    for Ts, beam, N, a, host_seq, words in [
        ([], 3, 0, None, False, "1 to 1024 samples"),
        ([2] * 1025, 3, None, None, False, "1 to 1024 samples"),
        ([8, 1], 3, None, None, False, "memory length 1"),  # Tk = 0
        ([8, 4098], 3, None, None, False, "memory length 4098"),  # Tk = 4097
        ([8, 9], 0, None, None, False, "beam_size must be in [1,16]"),
        ([8, 9], 17, None, None, False, "beam_size must be in [1,16]"),
        ([8, 9], 3, None, None, True, "seq_dev must be a device buffer"),
        ([4097] + [2] * 69, 16, None, alpha, False, "budget"),
    ]:
        rc, msg, intact = _submit(eng, packed, Ts, beam, N, a, host_seq)
        assert rc == D2T_EINVAL and words in msg, (Ts[:3], beam, rc, msg)
        assert intact and bool((alpha == float(AR.FCAN)).all()), (Ts[:3], beam)
    # ... and the context still searches, on both loops and submitted
    mems = rag._synthetic([9, 30, 4], 21)
    p, l = pack_memories(mems)
    want = _host_and_device(eng, lambda: eng.decode_attn_beam_batch_ragged(p, l, 3), "after the refusals")
    out = eng.decode_attn_beam_batch_async(p, l, 3)
    eng.wait_ticket(out[-1], host_sync=True)
    rag._same(_results(eng, out, l, False), want, "submitted after the refusals")
    with pytest.raises(ValueError, match="does not hold"):
        eng.decode_attn_beam_batch_async(packed[:10], [4, 5], 3)


def test_contexts_without_the_device_side_search():
    """supports_device_attn_beam() is false exactly where the submit refuses with D2T_ESTATE"""
    packed = torch.zeros(64, H, device=DEV)
    _, mt = engine_model("T2", 12, 1234, 1.8, beam_size=3)
    cfg = synth.make_config("TS0", device=DEV, max_seq_len=6, beam_size=3)
    cfg["Prediction"]["params"]["attn_type"] = "loc_aware"
    ml = Model(cfg).to(DEV).eval()
    for eng, words in ((mt.engine(), "Attn decoder"), (ml.engine(), "loc_aware")):
        assert not eng.supports_device_attn_beam()
        rc, msg, intact = _submit(eng, packed, [8, 9], 3)
        assert rc == D2T_ESTATE and words in msg and intact, (rc, msg)
        with pytest.raises(RuntimeError, match=words):
            eng.set_attn_beam_device(True)
        eng.set_attn_beam_device(False)
    for name in ("TS0", "TB0"):
        eng = (rag._engine() if name == "TS0" else engine_model(name, 8, 1234, 0.3, beam_size=3)[1]).engine()
        assert eng.supports_device_attn_beam()
        rc, msg, intact = _submit(eng, packed, [8, 9], 3)
        assert rc == 0 and not intact, (name, rc, msg)


# =====================================================================================================================
# 6. the switch
# =====================================================================================================================
def test_with_the_switch_off_every_entry_takes_the_host_loop():
    eng = rag._engine().engine()
    mem = torch.randn(2, 12, H, generator=torch.Generator().manual_seed(77)).to(DEV)
    calls = (lambda: eng.decode_attn_beam(mem[:1], 3), lambda: eng.decode_attn_beam_batch(mem, 3),
             lambda: eng.decode_attn_beam_batch(mem, 3, return_alpha=True),
             lambda: eng.decode_attn_beam_batch_ragged(mem.reshape(-1, H), [12, 12], 3))
    runs = eng.attn_beam_device_runs()
    for f in calls:
        f()
    assert eng.attn_beam_device_runs() == runs
    eng.set_attn_beam_device(True)
    try:
        for f in calls:
            f()
        assert eng.attn_beam_device_runs() == runs + len(calls)
    finally:
        eng.set_attn_beam_device(False)
    calls[1]()
    assert eng.attn_beam_device_runs() == runs + len(calls)


def test_the_host_loop_takes_more_samples_than_the_kernels():
    """1025 samples through the uniform entry with the switch off: the host loop's bookkeeping has no sample limit (the
    device-side kernels stop at 1024), and every sample's result is that of the same search split into two calls"""
    eng = rag._engine(L=8).engine()
    mem = torch.randn(1025, 3, H, generator=torch.Generator().manual_seed(1025)).to(DEV)
    assert 9 * 1025 * 2 * eng.attn_keys(3) * 4 <= _lib.ATTN_MAP_BUDGET
    runs = eng.attn_beam_device_runs()
    for maps in (False, True):
        whole = eng.decode_attn_beam_batch(mem, 2, return_alpha=maps)
        parts = eng.decode_attn_beam_batch(mem[:512], 2, return_alpha=maps) + eng.decode_attn_beam_batch(mem[512:], 2, return_alpha=maps)
        rag._same(whole, parts, f"1025 samples, maps {maps}")
    assert eng.attn_beam_device_runs() == runs
