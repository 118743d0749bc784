"""GPU: LSTM-attention (Attn / Attnv2) beam search over samples whose encoder memories have DIFFERENT lengths, in one step
loop (d2t_decode_attn_beam_batch_ragged, Model.beam_search_batch on a list of image tensors), and the ragged build of the
step kernel behind it (d2t_op_attn_decode_ragged).  The invariant at every level: a sample's results are those of the uniform
call on that sample alone, bit for bit -- a block of the ragged build finds its sample's length and first packed row through
the row map, and its arithmetic depends on that length alone.

Operator tests in the style of tests/test_recurrent_ops_gpu.py (whose helpers they use): outputs pre-filled with NaN / -1
behind a guard tail; values by that file's measured rule against recurrent_refs.attn_ref, err <= 8 e32 + 1e-6 max |y64|
(the project's margin), figures printed before they are asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import recurrent_refs as RR
import test_recurrent_ops_gpu as rops
from conftest import engine_model
from doc2tex_amd import Model, _lib, synth
from doc2tex_amd.engine import pack_memories
from test_parity_gpu import _case

pytestmark = pytest.mark.gpu
DEV = "cuda"
D2T_EINVAL, D2T_ESTATE = 1, 4  # include/d2t.h
H = 256
END = 1  # [s] of the LSTM-attention heads (attn_converter.py:8)


def _fbits(v):
    return int(np.float32(float(v)).view(np.int32))


# =====================================================================================================================
# 1. the operator
# =====================================================================================================================
OP_T = (19, 2, 1030, 5)  # key_off 1: Tk = 18, 1 (one key), 1029 (the 1024-strided loops go round twice), 4 (< taps)
OP_ROWS = [2, 0, 3, 1, 2, 2, 0]
OP_LD = 1031  # larger than every Tk, no multiple of 4
OP_TAPS, OP_KEY_OFF = 11, 1


@functools.lru_cache(maxsize=None)
def _op_inputs(V):
    """weights, per-sample memories and key projections (float64 products rounded to fp32: inputs of the kernel), the tokens fed"""
    W = RR.attn_weights(V, OP_TAPS, 91 + V)
    mems = [torch.randn(1, T, H, generator=rops._gen(700 + i)) for i, T in enumerate(OP_T)]
    kps = [(m.double() @ W["wk"].double().t() + W["bk"].double()).float() for m in mems]
    fed = torch.randint(0, V, (len(OP_ROWS), 3), generator=rops._gen(17))
    fed[:, 0] = 0  # [GO]: what a first step starts from
    return W, mems, kps, fed


@functools.lru_cache(maxsize=None)
def _op_reference(V, init_mode):
    """per sample: float64 reference and e32 of the three steps on that sample's rows (computed once, never written)"""
    W, mems, kps, fed = _op_inputs(V)
    out = {}
    for i in range(len(OP_T)):
        mine = [b for b, r in enumerate(OP_ROWS) if r == i]

        def fn(dt, mode):
            r = RR.attn_ref(RR.cast(W, dt), mems[i].to(dt), kps[i].to(dt), 3, rows=[0] * len(mine), teacher=fed[mine], mode=mode,
                            key_off=OP_KEY_OFF, init_mode=init_mode, coverage=True)
            return {f"{k}{s}": r[k][:, s] for k in ("probs", "hafter", "cafter", "mem", "alpha") for s in range(3)}
        out[i] = (mine,) + RR.e32_of(fn)
    return out


def _ragged_step(W, mem, kp, Ts, rows, st_ld, *, first, state=None, tok_in=None, key_off=OP_KEY_OFF, init_mode=2, row0=None,
                 step_mode=True, over=None):
    """one d2t_op_attn_decode_ragged call on the packed mem / kp [sum Ts][256]; returns rc and the outputs (CPU; the Bufs
    themselves after a refusal)"""
    lib = _lib.require_device()
    B, V, taps = len(rows), W["wg_t"].shape[1], W["wloc"].shape[1]
    keep = [rops._d(mem), rops._d(kp)]
    a = _lib.D2TOpAttnDecodeArgs()
    a.mem, a.kp = keep[0].data_ptr(), keep[1].data_ptr()
    for k in rops._W_KEYS:
        if k in W:
            keep.append(rops._d(W[k]))
            setattr(a, k, keep[-1].data_ptr())
    o = dict(probs=rops.Buf(B, 1, V), tokens=rops.Buf(B, 1, dtype=torch.int64), end_step=rops.Buf(B, dtype=torch.int32, fill=-7),
             sv_alpha=rops.Buf(B, 1, max(st_ld, 1)))
    if step_mode:
        o.update(st_h_out=rops.Buf(B, H), st_c_out=rops.Buf(B, H), st_mem_out=rops.Buf(B, max(st_ld, 1)))
        a.step_mode, a.first = 1, int(first)
        keep.append(rops._d(torch.as_tensor(rows, dtype=torch.int32)))
        a.row_sample = keep[-1].data_ptr()
        if not first:
            for k, v in zip(("st_h_in", "st_c_in", "st_mem_in"), state):
                keep.append(rops._d(v))
                setattr(a, k, keep[-1].data_ptr())
            keep.append(rops._d(tok_in.to(torch.int64)))
            a.tok_in = keep[-1].data_ptr()
    for k, b in o.items():
        setattr(a, k, b.ptr)
    a.bscore, a.out_dropscale = float(W["bscore"]), 1.0
    a.B, a.T, a.S, a.V, a.taps, a.key_off, a.init_mode = B, max(Ts), 1, V, taps, key_off, init_mode
    a.coverage, a.end_token, a.samples = 1, 1, len(Ts)
    for k, v in (over or {}).items():
        setattr(a, k, v)
    r0 = list(np.concatenate([[0], np.cumsum(Ts)[:-1]])) if row0 is None else row0
    keep += [rops._d(torch.as_tensor([int(v) for v in r0], dtype=torch.int32)), rops._d(torch.as_tensor(list(Ts), dtype=torch.int32))]
    rc = lib.d2t_op_attn_decode_ragged(C.byref(a), keep[-2].data_ptr(), keep[-1].data_ptr(), st_ld, rops._stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, o
    return rc, {k: b.get() for k, b in o.items()}


@pytest.mark.parametrize("V", (37, 1025))  # the narrow and the wide build
@pytest.mark.parametrize("init_mode", (1, 2))
def test_ragged_step_chain_equals_the_uniform_step_per_sample(init_mode, V):
    """three chained steps (first, then two resumed through st_*) over 7 rows of 4 samples of different lengths: every row
    equals, bit for bit, the uniform d2t_op_attn_decode on its sample's memory alone (T = T_i), meets the measured rule against
    the float64 reference, and has an alignment row of exact zeros beyond its sample's keys"""
    W, mems, kps, fed = _op_inputs(V)
    ref = _op_reference(V, init_mode)
    packed_mem, packed_kp = torch.cat([m[0] for m in mems]), torch.cat([k[0] for k in kps])
    kw = dict(key_off=OP_KEY_OFF, init_mode=init_mode, coverage=True)
    state, ustate = None, {}
    for s in range(3):
        rc, got = _ragged_step(W, packed_mem, packed_kp, OP_T, OP_ROWS, OP_LD, first=s == 0, state=state, tok_in=fed[:, s],
                               init_mode=init_mode)
        assert rc == 0, f"step {s}: rc {rc}"
        for i, T in enumerate(OP_T):
            mine, y64, e32 = ref[i]
            Tk = T - OP_KEY_OFF
            st = dict(first=s == 0, rows=None, B=len(mine), state=ustate.get(i), tok_in=fed[mine, s])
            rc, uni = rops._decode(W, mems[i], kps[i], 1, alpha=True, step=st, **kw)
            assert rc == 0
            ustate[i] = (uni["st_h_out"], uni["st_c_out"], uni["st_mem_out"])
            for name, a, b in (("probs", got["probs"][mine], uni["probs"]), ("tokens", got["tokens"][mine], uni["tokens"]),
                               ("st_h_out", got["st_h_out"][mine], uni["st_h_out"]), ("st_c_out", got["st_c_out"][mine], uni["st_c_out"]),
                               ("st_mem_out", got["st_mem_out"][mine, :Tk], uni["st_mem_out"]),
                               ("sv_alpha", got["sv_alpha"][mine, 0, :Tk], uni["sv_alpha"][:, 0])):
                assert rops._same(a, b), f"step {s}, sample {i} (T {T}): {name} differs from the uniform step"
            assert bool((rops._bits(got["sv_alpha"][mine, 0, Tk:]) == 0).all()), f"step {s}, sample {i}: alignment not zero beyond Tk"
            info = dict(step=s, T=T, V=V, init=init_mode)
            rops._rule("ragged_step_probs", got["probs"][mine, 0], y64[f"probs{s}"], e32[f"probs{s}"], **info)
            rops._rule("ragged_step_h", got["st_h_out"][mine], y64[f"hafter{s}"], e32[f"hafter{s}"], **info)
            rops._rule("ragged_step_c", got["st_c_out"][mine], y64[f"cafter{s}"], e32[f"cafter{s}"], **info)
            rops._rule("ragged_step_mem", got["st_mem_out"][mine, :Tk], y64[f"mem{s}"], e32[f"mem{s}"], **info)
            rops._rule("ragged_step_alpha", got["sv_alpha"][mine, 0, :Tk], y64[f"alpha{s}"], e32[f"alpha{s}"], **info)
        state = (got["st_h_out"], got["st_c_out"], got["st_mem_out"])  # tails beyond Tk as the kernel left them


def test_ragged_step_refusals():
    """tables that would index out of range, a stride below a Tk, the ragged fields outside step mode: D2T_EINVAL, nothing written"""
    V = 37
    W, mems, kps, fed = _op_inputs(V)
    mem, kp = torch.cat([m[0] for m in mems]), torch.cat([k[0] for k in kps])
    total = sum(OP_T)
    ok = dict(Ts=OP_T, rows=OP_ROWS, st_ld=OP_LD)
    r0 = [0, 19, 21, 1051]
    assert r0[-1] + OP_T[-1] == total
    cases = [dict(Ts=(19, 0, 1030, 5)), dict(Ts=(19, 1, 1030, 5)),  # T = 1 behind the dropped token: Tk = 0
             dict(Ts=(19, -2, 1030, 5)), dict(Ts=(19, 2, 4098, 5), st_ld=4096),  # Tk = 4097
             dict(row0=[0, 19, -1, 1051]),
             dict(row0=[0, 19, 21, 1052]), dict(row0=[0, 19, 27, 1051]),  # row0 + T beyond the packed rows
             dict(st_ld=1028), dict(st_ld=1), dict(st_ld=0), dict(st_ld=4097),  # below a Tk (1029); outside [1, 4096]
             dict(over=dict(T=1031)), dict(over=dict(T=19)),  # args->T is not the largest length
             dict(rows=[2, 0, 4, 1, 2, 2, 0]),  # a row of a sample the tables do not hold
             dict(step_mode=False, rows=[0, 1, 2, 3])]  # the ragged fields without step mode
    for c in cases:
        kw = dict(ok)
        kw.update(c)
        Ts, rows, st_ld = kw.pop("Ts"), kw.pop("rows"), kw.pop("st_ld")
        rc, o = _ragged_step(W, mem, kp, Ts, rows, st_ld, first=True, **kw)
        assert rc == D2T_EINVAL, (c, rc)
        assert all(b.untouched() for b in o.values()), c
    lib = _lib.require_device()
    a = _lib.D2TOpAttnDecodeArgs()
    assert lib.d2t_op_attn_decode_ragged(C.byref(a), None, None, 8, rops._stream()) == D2T_EINVAL
    # the explicit tables of the accepted call are the default ones
    rc, got = _ragged_step(W, mem, kp, OP_T, OP_ROWS, OP_LD, first=True, row0=r0)
    assert rc == 0 and not torch.isnan(got["probs"]).any()


# =====================================================================================================================
# 2. the search
# =====================================================================================================================
def _synthetic(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, T, H, generator=g).to(DEV) for T in lengths]


def _per_sample(eng, mems, beam, return_alpha=False):
    """d2t_decode_attn_beam_batch[_alpha] on every sample alone"""
    return [eng.decode_attn_beam_batch(m[j:j + 1].contiguous(), beam, return_alpha)[0] for m in mems for j in range(m.shape[0])]


def _same(got, want, what):
    """(seq [1, len], score[, map [len, Tk]]) tuples: tokens, length, the score's float bits and the map's bits"""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w)
        assert g[0].shape == w[0].shape and torch.equal(g[0], w[0]), f"{what}: sample {i}: {g[0].tolist()} != {w[0].tolist()}"
        assert _fbits(g[1]) == _fbits(w[1]), f"{what}: sample {i}: score {float(g[1])!r} != {float(w[1])!r}"
        if len(g) > 2:
            assert g[2].shape == w[2].shape, f"{what}: sample {i}: map {tuple(g[2].shape)} != {tuple(w[2].shape)}"
            assert rops._same(g[2].cpu(), w[2].cpu()), f"{what}: sample {i}: alignment map differs"


_ENGINES = {}


def _engine(name="TS0", L=14, eb=0.3, beam=5):
    """one model per configuration for this file's searches (the beam width is an argument of every call)"""
    key = (name, L, eb)
    if key not in _ENGINES:
        _ENGINES[key] = engine_model(name, L, 1234, eb, beam_size=beam)[1]
    return _ENGINES[key]


SEARCH_T = [9, 30, 2, 1030, 9]


@pytest.mark.parametrize("beam", [1, 3, 16])
def test_every_sample_equals_its_own_search(beam):
    eng = _engine().engine()
    assert eng.supports_ragged_attn_beam() and not eng.supports_ragged_beam()
    mems = _synthetic(SEARCH_T, 5)
    packed, lengths = pack_memories(mems)
    assert lengths == SEARCH_T
    want = _per_sample(eng, mems, beam)
    _same(eng.decode_attn_beam_batch_ragged(packed, lengths, beam), want, f"beam {beam}")
    wmaps = _per_sample(eng, mems, beam, return_alpha=True)
    gmaps = eng.decode_attn_beam_batch_ragged(packed, lengths, beam, return_alpha=True)
    for T, g in zip(SEARCH_T, gmaps):
        assert g[2].shape == (g[0].shape[1], eng.attn_keys(T))
    _same(gmaps, wmaps, f"beam {beam} with maps")
    _same([g[:2] for g in gmaps], want, f"beam {beam}: maps change nothing")
    # the same list reversed: other offsets, other rows, the same results
    rev = mems[::-1]
    _same(eng.decode_attn_beam_batch_ragged(*pack_memories(rev), beam, return_alpha=True), wmaps[::-1], f"beam {beam} reversed")


def test_the_raw_map_is_zero_beyond_a_samples_keys_and_length():
    eng = _engine().engine()
    mems = _synthetic([9, 30, 2], 6)
    packed, lengths = pack_memories(mems)
    N, S, ld = 3, eng.cfg.batch_max_length + 1, eng.attn_keys(30)
    seq, n, score = (C.c_int64 * (N * S))(), (C.c_int32 * N)(), (C.c_float * N)()
    alpha = torch.full((N, S, ld), float("nan"), device=DEV)
    rc = eng.lib.d2t_decode_attn_beam_batch_ragged(eng.ctx, _lib.ptr(packed), N, (C.c_int32 * N)(*lengths), 3, seq, n, score,
                                                   _lib.ptr(alpha), _lib.stream_of(packed))
    assert rc == 0
    a = alpha.cpu()
    assert not torch.isnan(a).any()
    for i, T in enumerate(lengths):
        assert bool((a[i, :, eng.attn_keys(T):] == 0).all()) and bool((a[i, n[i]:] == 0).all())
        rows = a[i, :n[i], :eng.attn_keys(T)].double().sum(-1)
        assert float((rows - 1).abs().max()) <= 1e-5  # each row a softmax over the sample's own keys


def test_workspace_reuse_and_a_search_behind_a_pipelined_greedy_decode():
    eng = _engine().engine()
    big, small = _synthetic([700, 40, 1030], 7), _synthetic([3, 5], 8)
    wb, ws = _per_sample(eng, big, 3, True), _per_sample(eng, small, 3, True)
    for mems, want, what in ((big, wb, "large"), (small, ws, "small after large"), (big, wb, "large again")):
        _same(eng.decode_attn_beam_batch_ragged(*pack_memories(mems), 3, return_alpha=True), want, what)
    # chain 0's key projection workspace is shared with the pipelined greedy decode: the search waits for it
    gm = torch.randn(6, 900, H, generator=torch.Generator().manual_seed(9)).to(DEV)
    tok_sync, probs_sync = eng.decode_attn_greedy(gm, False)
    tok, probs, ticket = eng.decode_attn_greedy_async(gm, False)
    got = eng.decode_attn_beam_batch_ragged(*pack_memories(small), 3, return_alpha=True)
    eng.wait_ticket(ticket, host_sync=True)
    _same(got, ws, "behind a submitted greedy decode")
    assert torch.equal(tok, tok_sync) and rops._same(probs.cpu(), probs_sync.cpu())
    assert int(eng.lib.d2t_decode_last_ticket(eng.ctx)) == int(ticket)  # the search takes no ticket


@pytest.mark.parametrize("N,T,beam", [(4, 17, 5), (1, 261, 3)])
def test_equal_lengths_give_what_the_uniform_call_gives(N, T, beam):
    eng = _engine().engine()
    mem = torch.randn(N, T, H, generator=torch.Generator().manual_seed(N + T)).to(DEV)
    _same(eng.decode_attn_beam_batch_ragged(mem.reshape(-1, H), [T] * N, beam, return_alpha=True),
          eng.decode_attn_beam_batch(mem, beam, return_alpha=True), "uniform")


# =====================================================================================================================
# 3. the model
# =====================================================================================================================
# (config, fixture, end_bias (None: the fixture's), crops (samples, H, W), what the per-tensor searches must show).  The
# fixture's crop is the first tensor's size and its sample rides in row 0; image seeds 4100 + tensor index.  Chosen on the
# CPU oracle (oracle.restatement's beam search at the fixture's beam width):
#   TS0 at the fixture's 0.3: the 48 x 64 and 48 x 32 crops emit [s] after 1 to 3 tokens, the 32 x 64 crops run to the limit
#       of 15 -- samples drop out of the shared loop while others stay to its end.
#   C0: the seeded VGG + BiLSTM stack barely looks at its input (the oracle's scores over these 3 crop widths, 6 seeds and 12 contrast /
#       brightness settings agree to 2e-4), so one list cannot hold both kinds: every sample runs to the limit of 13 up to
#       end_bias 0.17 (the fixture's 0.15 included) and every sample emits [s] at once from 0.175 on.  Both are run.
MODEL_CASES = [("TS0", "ts0_beam5", None, [(3, 48, 64), (2, 48, 32), (2, 32, 64)], "mixed"),
               ("C0", "c0_beam3", None, [(2, 32, 320), (2, 32, 160), (2, 32, 96)], "limit"),
               ("C0", "c0_beam3", 0.18, [(2, 32, 320), (2, 32, 160), (2, 32, 96)], "end")]


@pytest.mark.parametrize("name,fixture,eb,crops,kind", MODEL_CASES)
def test_model_list_equals_the_per_tensor_calls(cases, name, fixture, eb, crops, kind):
    c = _case(cases, "attn_beam", fixture)
    assert c["config"] == name and (c["H"], c["W"]) == crops[0][1:]
    beam, S = c["beam_size"], c["max_seq_len"] + 1
    m = _engine(name, c["max_seq_len"], c["end_bias"] if eb is None else eb, beam)
    imgs = [synth.synth_images(n, Hh, Ww, seed=4100 + i) for i, (n, Hh, Ww) in enumerate(crops)]
    imgs[0][:1] = synth.synth_images(1, c["H"], c["W"], seed=c["iseed"])
    imgs = [x.cuda() for x in imgs]
    with torch.no_grad():
        want = [r for x in imgs for r in m.beam_search_batch(x, beam)]
        wmaps = [r for x in imgs for r in m.beam_search_batch(x, beam, return_attn=True)]
        lengths = [m.forward_encoder(x)[0].shape[1] for x in imgs]
    assert len(set(lengths)) >= 2, lengths  # (TS0's 48 x 32 and 32 x 64 crops have one memory length, in different tensors)
    ended = [int(s[0, -1]) == END for s, _ in want]
    print("FIG ragged_attn_model", name, kind, [(s.shape[1], e) for (s, _), e in zip(want, ended)])
    assert all(s.shape[1] == S for (s, _), e in zip(want, ended) if not e)  # whoever does not emit [s] runs to the limit
    if kind == "mixed":
        assert any(ended) and not all(ended), ended
    else:
        assert all(ended) if kind == "end" else not any(ended), ended
    with torch.no_grad():
        got = m.beam_search_batch(imgs, beam)
        gmaps = m.beam_search_batch(imgs, beam, return_attn=True)
    _same(got, want, f"{name} list")
    _same(gmaps, wmaps, f"{name} list with maps")
    if eb is None:  # the reference's own result for the sample in row 0
        assert got[0][0][0].tolist() == c["seq"], (got[0][0].tolist(), c["seq"])
        assert abs(float(got[0][1]) - c["score"]) <= 1e-3, (float(got[0][1]), c["score"])
    with torch.no_grad():  # a tuple, a list of one tensor, the empty list; the single-tensor form is still today's call
        _same(m.beam_search_batch(tuple(imgs[1:]), beam), want[crops[0][0]:], "tuple")
        _same(m.beam_search_batch([imgs[2]], beam), want[-crops[2][0]:], "a list of one tensor")
        assert m.beam_search_batch([], beam) == []


def test_model_falls_back_when_the_lists_history_exceeds_the_budget(monkeypatch):
    """return_attn on a list whose history would not fit: the tensors are searched one after the other, with the same maps"""
    m = _engine()
    imgs = [synth.synth_images(2, 48, 64, seed=4300).cuda(), synth.synth_images(1, 32, 64, seed=4301).cuda()]
    with torch.no_grad():
        want = m.beam_search_batch(imgs, 3, return_attn=True)
        monkeypatch.setattr(_lib, "ATTN_MAP_BUDGET", 1024)
        calls = []
        eng = m.engine()
        monkeypatch.setattr(eng, "decode_attn_beam_batch_ragged", lambda *a, **k: calls.append(a) or [])
        got = m.beam_search_batch(imgs, 3, return_attn=True)
    assert not calls
    _same(got, want, "per-tensor path")


# =====================================================================================================================
# 4. refusals
# =====================================================================================================================
def _raw(eng, packed, Ts, beam, N=None, alpha=None):
    n = len(Ts) if N is None else N
    S = eng.cfg.batch_max_length + 1
    k = max(len(Ts), 1)
    seq, ln, score = (C.c_int64 * (max(n, 1) * S))(), (C.c_int32 * max(n, 1))(), (C.c_float * max(n, 1))()
    rc = eng.lib.d2t_decode_attn_beam_batch_ragged(eng.ctx, _lib.ptr(packed), n, (C.c_int32 * k)(*Ts), beam, seq, ln, score,
                                                   _lib.ptr(alpha), _lib.stream_of(packed))
    return rc, eng.lib.d2t_last_error(eng.ctx).decode()


def test_refusals_leave_the_context_usable():
    eng = _engine().engine()
    assert eng.cfg.attn_keys == _lib.ATTN_KEYS_NOCLS_INIT_CLS  # Attnv2 behind a ViT: T = Tk + 1
    packed = torch.randn(4200, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    tok, probs, ticket = eng.decode_attn_greedy_async(packed[:40].reshape(2, 20, H), False)
    eng.wait_ticket(ticket, host_sync=True)
    S = eng.cfg.batch_max_length + 1
    # S * N * beam * max Tk * 4 bytes of history: 15 x 70 x 16 x 4096 x 4 = 275 MB > 256 MiB
    over_budget = torch.empty(16, device=DEV)
    assert S * 70 * 16 * 4096 * 4 > _lib.ATTN_MAP_BUDGET
    for Ts, beam, N, alpha, code, words in [
        ([], 3, 0, None, D2T_EINVAL, "1 to 1024 samples"),
        ([4], 3, -2, None, D2T_EINVAL, "1 to 1024 samples"),
        ([2] * 1025, 3, None, None, D2T_EINVAL, "1 to 1024 samples"),
        ([8, 1], 3, None, None, D2T_EINVAL, "memory length 1"),  # Tk = 0
        ([8, 0], 3, None, None, D2T_EINVAL, "memory length 0"),
        ([8, -3], 3, None, None, D2T_EINVAL, "memory length -3"),
        ([8, 4098], 3, None, None, D2T_EINVAL, "memory length 4098"),  # Tk = 4097
        ([8, 9], 0, None, None, D2T_EINVAL, "beam_size must be in [1,16]"),
        ([8, 9], 17, None, None, D2T_EINVAL, "beam_size must be in [1,16]"),
        ([4097] + [2] * 69, 16, None, over_budget, D2T_EINVAL, "budget"),
    ]:
        rc, msg = _raw(eng, packed, Ts, beam, N, alpha)
        assert rc == code and words in msg, (Ts[:3], beam, rc, msg)
    if torch.cuda.device_count() > 1:  # (a second GPU is the only way to own a pointer of another device)
        rc, msg = _raw(eng, torch.zeros(64, H, device="cuda:1"), [8], 3)
        assert rc == D2T_EINVAL and "device" in msg, (rc, msg)
    assert int(eng.lib.d2t_decode_last_ticket(eng.ctx)) == int(ticket)
    # ... and the context still searches, correctly
    mems = _synthetic([9, 30, 4], 21)
    _same(eng.decode_attn_beam_batch_ragged(*pack_memories(mems), 3), _per_sample(eng, mems, 3), "after the refusals")
    with pytest.raises(ValueError, match="does not hold"):
        eng.decode_attn_beam_batch_ragged(packed[:10], [4, 5], 3)


def test_contexts_that_the_ragged_search_does_not_serve():
    packed = torch.zeros(64, H, device=DEV)
    # a TFM context
    _, mt = engine_model("T2", 12, 1234, 1.8, beam_size=3)
    assert not mt.engine().supports_ragged_attn_beam()
    rc, msg = _raw(mt.engine(), packed, [8, 9], 3)
    assert rc == D2T_ESTATE and "Attn decoder" in msg, (rc, msg)
    # the 'loc_aware' cell: the uniform call's refusal (weights as constructed: nothing is decoded)
    cfg = synth.make_config("TS0", device=DEV, max_seq_len=6, beam_size=3)
    cfg["Prediction"]["params"]["attn_type"] = "loc_aware"
    ml = Model(cfg).to(DEV).eval()
    eng = ml.engine()
    assert not eng.supports_ragged_attn_beam()
    rc, msg = _raw(eng, packed, [8, 9], 3)
    S = eng.cfg.batch_max_length + 1
    seq, ln, score = (C.c_int64 * (2 * S))(), (C.c_int32 * 2)(), (C.c_float * 2)()
    rcu = eng.lib.d2t_decode_attn_beam_batch(eng.ctx, _lib.ptr(packed), 2, 8, 3, seq, ln, score, _lib.stream_of(packed))
    assert rc == D2T_ESTATE and rcu == D2T_ESTATE and "loc_aware" in msg and msg == eng.lib.d2t_last_error(eng.ctx).decode()
    # the Bahdanau cell with one-hot targets and a zero initial state is served
    _, mb = engine_model("TB0", 8, 1234, 0.3, beam_size=3)
    eb = mb.engine()
    assert eb.supports_ragged_attn_beam()
    mems = _synthetic([6, 40, 2], 31)
    _same(eb.decode_attn_beam_batch_ragged(*pack_memories(mems), 3, return_alpha=True), _per_sample(eb, mems, 3, True), "TB0")
