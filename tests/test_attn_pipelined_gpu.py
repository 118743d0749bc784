"""GPU: pipelined serving of the LSTM-attention heads (Attn / Attnv2) and their early exit decided inside the kernel.

The pipelined forward (Model.pipelined, d2t_decode_attn_greedy_submit) must return bit for bit what the synchronous forward
returns -- tokens, probs, alignment maps, zeros after the is_test exit -- for every head variant, with 1, 2 and 3 decode
chains, consumed out of order; the exit rule is pinned on fixtures from the reference whose rows end at DIFFERENT steps
(tests/golden/attn_serve_*.npz, tools/make_golden_attn_serve.py), on more rows than the chip holds blocks, on a batch with
a row that never ends and on output buffers full of garbage."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, engine_model
from doc2tex_amd import _lib, synth

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "attn_serve_cases.json")) as f:
    SERVE = {c["case"]: c for c in json.load(f)["cases"]}
with open(os.path.join(GOLD, "viz_cases.json")) as f:
    VIZ = {c["case"]: c for c in json.load(f)["cases"]}
LOGIT_TOL = 1e-3  # the LSTM-head parity tests' bar
ALPHA_TOL = 1e-4  # tests/test_viz_attn_gpu.py ATOL


def _load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _forward(m, img, L, is_test):
    """One Model.forward in eval mode: (tokens, probs, alpha_stores or None, addition_outputs)."""
    text = torch.zeros(img.shape[0], L + 1, dtype=torch.long, device="cuda")
    pred = m.predicter.Prediction
    if hasattr(pred, "alpha_stores"):
        del pred.alpha_stores
    with torch.no_grad():
        p, l, add = m(img, text, is_train=False, is_test=is_test)
    return p, l, getattr(pred, "alpha_stores", None), add


def _sync_ref(m, imgs, L, is_test):
    m.pipelined = False
    out = []
    for x in imgs:
        p, l, a, add = _forward(m, x, L, is_test)
        assert add == {}
        out.append((p.clone(), l.clone(), None if a is None else a.clone()))
    torch.cuda.synchronize()
    return out


def _ref_steps(tokens, is_test):
    """The reference's step count of a full-size [B, S] token tensor of these heads ([s] = 1)."""
    S = tokens.shape[1]
    if not is_test:
        return S
    ended = (tokens == 1).any(1)
    if not bool(ended.all()):
        return S
    last = int((tokens == 1).float().argmax(1).max())
    return last + 1 if last + 1 < S else S


def _same(got, want):
    return all((g is None and w is None) or torch.equal(g, w) for g, w in zip(got, want))


def _raw(eng, mem, is_test, submit, garbage=True, misalign=False):
    """The C-ABI itself on caller buffers (pre-filled with garbage): (tokens, probs, alpha, steps)."""
    B, T, _ = mem.shape
    S, V, Tk = eng.cfg.batch_max_length + 1, eng.cfg.vocab, eng.attn_keys(T)
    tok = torch.full((B, S), 0x7F7F7F7F7F7F7F7F if garbage else 0, dtype=torch.int64, device="cuda")
    fill = float("nan") if garbage else 0.0
    off = 1 if misalign else 0  # buffers that start 4 bytes past a 16-byte boundary: the finalize kernel's unaligned ends
    pbuf = torch.full((B * S * V + off,), fill, dtype=torch.float32, device="cuda")
    abuf = torch.full((B * S * Tk + off,), fill, dtype=torch.float32, device="cuda")
    probs, alpha = pbuf[off:].view(B, S, V), abuf[off:].view(B, S, Tk)
    assert probs.data_ptr() % 16 == 4 * off
    stream = _lib.stream_of(mem)
    if submit:
        t = C.c_int64(0)
        rc = eng.lib.d2t_decode_attn_greedy_submit(eng.ctx, _lib.ptr(mem), B, T, int(is_test), _lib.ptr(tok), _lib.ptr(probs),
                                                   _lib.ptr(alpha), stream, C.byref(t))
        assert rc == 0, eng.lib.d2t_last_error(eng.ctx)
        assert int(t.value) == int(eng.lib.d2t_decode_last_ticket(eng.ctx))
        eng.wait_ticket(int(t.value), host_sync=True)
        assert eng.ticket_done(int(t.value))
        steps = eng.decode_steps(int(t.value))
        assert len(steps) == 1
        steps = steps[0]
    else:
        n = C.c_int32(0)
        rc = eng.lib.d2t_decode_attn_greedy_alpha(eng.ctx, _lib.ptr(mem), B, T, int(is_test), _lib.ptr(tok), _lib.ptr(probs),
                                                  _lib.ptr(alpha), C.byref(n), stream)
        assert rc == 0, eng.lib.d2t_last_error(eng.ctx)
        torch.cuda.synchronize()
        steps = int(n.value)
    return tok, probs, alpha, steps


def _serve_model(name):
    c = SERVE[name]
    _, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], c["end_bias"])
    return c, m, synth.staggered_images(seed=c["iseed"]).cuda()


# ---- 1. the new fixtures, synchronous call ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["attn_serve_ts0_stagger", "attn_serve_to0_stagger"])
def test_rows_ending_at_different_steps_match_the_reference(name):
    """A block whose row ended early must still run to the LARGEST end step: steps 7 .. 14 of rows 0, 1, 3 of the TS0 case
    are values the reference produces."""
    c, m, img = _serve_model(name)
    z = _load(name)
    with torch.no_grad():
        mem = m.forward_encoder(img)[0].contiguous()
    tok, probs, alpha, steps = _raw(m.engine(), mem, True, submit=False)
    err = float(np.abs(probs.cpu().numpy() - z["probs"]).max())
    aerr = float(np.abs(alpha.cpu().numpy() - z["alpha"]).max())
    print(f"{name}: steps {steps}, max |dprob| = {err:.2e}, max |dalpha| = {aerr:.2e}")
    assert steps == c["steps"] == {"attn_serve_ts0_stagger": 15, "attn_serve_to0_stagger": 7}[name]
    assert np.array_equal(tok.cpu().numpy(), z["tokens"])
    assert err <= LOGIT_TOL and aerr <= ALPHA_TOL
    assert not bool(probs[:, steps:].any()) and not bool(tok[:, steps:].any()) and not bool(alpha[:, steps:].any())
    # and through Model.forward
    p, l, _, add = _forward(m, img, c["max_seq_len"], True)
    assert add == {} and torch.equal(p, tok) and torch.equal(l, probs)


# ---- 2. pipelined = synchronous, bitwise ----------------------------------------------------------------------------------
# config, batch_max_length, end_bias, input seed of the first batch (the *_greedy_early fixtures' where there is one)
STACKS = [("TS0", 30, 0.45, 1120), ("TO0", 14, 0.6, 1310), ("TB0", 12, 0.45, 1320), ("TA0", 12, 0.3, 1330),
          ("C0", 150, 0.0, 1007), ("B0", 40, 0.0, 1081)]


@pytest.mark.parametrize("cname,L,eb,iseed", STACKS)
def test_pipelined_equals_synchronous_bitwise(cname, L, eb, iseed):
    H, W = synth.crop_shape(cname)
    _, m = engine_model(cname, L, 1234, eb)
    m.predicter.Prediction.viz_attn = True  # the alignment maps too
    sizes = [3, 2, 4, 1, 3, 2]  # batch 0 = viz_ts0_greedy_early / c0_greedy_early / b0_greedy_early where they exist
    imgs = [synth.synth_images(b, H, W, seed=iseed + i).cuda() for i, b in enumerate(sizes)]
    if H == 48:
        imgs[2] = synth.staggered_images(seed=iseed).cuda()  # rows that end at different steps
    exits = []
    for is_test in (False, True):
        ref = _sync_ref(m, imgs, L, is_test)
        want_steps = [_ref_steps(r[0], is_test) for r in ref]
        exits += [s for s in want_steps if s < L + 1]
        for chains in (1, 2, 3):
            m.pipelined, m.decode_chains = True, chains
            outs = []
            for x in imgs:  # six forwards in flight before the first wait
                p, l, a, add = _forward(m, x, L, is_test)
                assert sorted(add) == ["decode"] and tuple(p.shape) == (x.shape[0], L + 1) and a.shape[-1] == 1
                outs.append((p, l, a, add["decode"]))
            # a synchronous forward right behind them (it shares chain 0's workspace)
            m.pipelined = False
            p, l, a, add = _forward(m, imgs[2], L, is_test)
            assert add == {} and _same((p, l, a), ref[2]), (cname, is_test, chains, "synchronous call after pipelined ones")
            for i in (4, 1, 5, 0, 3, 2):  # consumed out of order
                p, l, a, h = outs[i]
                h.wait(host_sync=True)
                assert h.done()
                assert _same((p, l, a), ref[i]), (cname, is_test, chains, i)
                assert h.steps() == want_steps[i], (cname, is_test, chains, i, h.steps(), want_steps[i])
                rp, rl = h.result()
                assert rp is p and rl is l  # full size, as the synchronous forward of these heads returns them
            m.synchronize()
    print(f"{cname}: early exits at steps {sorted(set(exits))} of {L + 1}")
    if eb > 0.0:
        assert exits, "no batch of this stack took the early exit"


# ---- 3. output buffers full of garbage ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_test", [True, False])
def test_outputs_do_not_depend_on_what_the_buffers_held(is_test):
    c, m, img = _serve_model("attn_serve_ts0_stagger")
    with torch.no_grad():
        mem = m.forward_encoder(img)[0].contiguous()
    eng = m.engine()
    clean = _raw(eng, mem, is_test, submit=False, garbage=False)
    assert clean[3] == (c["steps"] if is_test else c["max_seq_len"] + 1)
    for submit in (False, True):
        for misalign in (False, True):
            got = _raw(eng, mem, is_test, submit=submit, misalign=misalign)
            assert got[3] == clean[3] and _same(got[:3], clean[:3]), (submit, misalign)
    assert bool(torch.isfinite(clean[1]).all())


# ---- 4. more rows than the chip holds blocks ----------------------------------------------------------------------------------
def test_more_rows_than_resident_blocks():
    """600 one-block rows on 256 CUs: blocks that start late must neither hang the early ones nor change a result."""
    c, m, img = _serve_model("attn_serve_ts0_stagger")
    with torch.no_grad():
        mem = m.forward_encoder(img)[0].contiguous()
    eng = m.engine()
    small = _raw(eng, mem, True, submit=False)
    assert small[3] == 15
    big_mem = mem.repeat(150, 1, 1).contiguous()
    assert big_mem.shape[0] == 600
    runs = [_raw(eng, big_mem, True, submit=False), _raw(eng, big_mem, True, submit=True),
            _raw(eng, big_mem, True, submit=False), _raw(eng, big_mem, True, submit=True)]
    for k, (tok, probs, alpha, steps) in enumerate(runs):
        assert steps == 15, (k, steps)
        assert torch.equal(tok, small[0].repeat(150, 1)), k
        assert torch.equal(probs, small[1].repeat(150, 1, 1)), k
        assert torch.equal(alpha, small[2].repeat(150, 1, 1)), k


# ---- 5. a row that never ends ------------------------------------------------------------------------------------------------
def test_a_row_that_never_ends_keeps_every_step():
    c, m, img = _serve_model("attn_serve_ts0_noend")
    z = _load("attn_serve_ts0_noend")
    S = c["max_seq_len"] + 1
    with torch.no_grad():
        mem = m.forward_encoder(img)[0].contiguous()
    eng = m.engine()
    full = _raw(eng, mem, False, submit=False)
    err = float(np.abs(full[1].cpu().numpy() - z["probs"]).max())
    print(f"attn_serve_ts0_noend: max |dprob| = {err:.2e}")
    assert np.array_equal(full[0].cpu().numpy(), z["tokens"]) and err <= LOGIT_TOL
    ends = [int((full[0][b] == 1).nonzero()[0]) if bool((full[0][b] == 1).any()) else -1 for b in range(4)]
    assert ends == c["end_steps"] == [6, -1, -1, 6]
    for submit in (False, True):
        got = _raw(eng, mem, True, submit=submit)
        assert got[3] == S == full[3]
        assert _same(got[:3], full[:3]), submit  # nothing zeroed
    assert bool((full[1][:, -1] != 0).any())


# ---- 6. viz_attn + pipelined ----------------------------------------------------------------------------------------------------
def test_pipelined_alpha_stores_match_the_reference():
    name = "viz_ts0_greedy_early"
    c, z = VIZ[name], _load(name)
    _, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], c["end_bias"])
    m.predicter.Prediction.viz_attn = True
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]).cuda()
    (rp, rl, ra), = _sync_ref(m, [img], c["max_seq_len"], True)
    m.pipelined, m.decode_chains = True, 2
    p, l, a, add = _forward(m, img, c["max_seq_len"], True)
    assert a is m.predicter.Prediction.alpha_stores and tuple(a.shape) == z["alpha"].shape + (1,)  # set at call time
    add["decode"].wait(host_sync=True)
    assert torch.equal(a, ra) and torch.equal(p, rp) and torch.equal(l, rl)
    assert np.array_equal(p.cpu().numpy(), z["tokens"])
    err = float(np.abs(a[..., 0].cpu().numpy() - z["alpha"]).max())
    print(f"{name} (pipelined): max |d alpha| = {err:.2e}")
    assert err <= ALPHA_TOL
    assert float(a[:, c["exit_step"] + 1:].abs().max()) == 0.0
    assert add["decode"].steps() == c["exit_step"] + 1
    # the maps-off pipelined forward leaves no alpha_stores behind and returns the same tensors
    m.predicter.Prediction.viz_attn = False
    p2, l2, a2, add2 = _forward(m, img, c["max_seq_len"], True)
    add2["decode"].wait(host_sync=True)
    assert a2 is None and torch.equal(p2, rp) and torch.equal(l2, rl)
    m.synchronize()


# ---- 7. handle semantics ---------------------------------------------------------------------------------------------------------
def test_handles_tickets_and_synchronize():
    cname, L = "C0", 150  # 151 steps per loop: the decodes are still running while the next forwards are issued
    H, W = synth.crop_shape(cname)
    _, m = engine_model(cname, L, 1234, 0.0)
    imgs = [synth.synth_images(3, H, W, seed=1400 + i).cuda() for i in range(12)]
    ref = _sync_ref(m, imgs, L, False)
    m.pipelined, m.decode_chains = True, 2
    eng = m.engine()
    t0 = int(eng.lib.d2t_decode_last_ticket(eng.ctx))
    outs = []
    for i, x in enumerate(imgs):
        p, l, _, add = _forward(m, x, L, False)
        h = add["decode"]
        assert h.ticket == t0 + i + 1  # one ticket per forward, the counter of the TFM decodes
        assert h.done() in (True, False)  # a poll: never blocks, never raises
        outs.append((p, l, h))
        if i == 4:  # consume batch 3 while 4 is in flight
            outs[3][2].wait(host_sync=True)
            assert outs[3][2].done() and torch.equal(outs[3][0], ref[3][0]) and torch.equal(outs[3][1], ref[3][1])
    m.synchronize()
    assert int(eng.lib.d2t_decode_last_ticket(eng.ctx)) - t0 == len(imgs)
    assert all(h.done() for _, _, h in outs)
    for (p, l, h), (rp, rl, _) in zip(outs, ref):  # twelve batches later the first ones are still intact
        assert torch.equal(p, rp) and torch.equal(l, rl) and h.steps() == L + 1
    with pytest.raises(RuntimeError):
        eng.wait_ticket(10 ** 9)
    m.pipelined = False
    p, l, _, add = _forward(m, imgs[0], L, False)
    assert add == {} and torch.equal(p, ref[0][0]) and torch.equal(l, ref[0][1])


# ---- 8. wide vocabulary -------------------------------------------------------------------------------------------------------------
def test_wide_vocabulary_pipelined_early_exit():
    from test_attn_vocab_gpu import _cfg, _model, _pad, _seeded
    V0, V1, L = 1000, 3000, 12
    cfg0, cfg1 = _cfg("TS0", V0, L), _cfg("TS0", V1, L)
    m = _model(cfg1, _pad(_seeded(cfg0, end_bias=0.3), V0, V1 - V0))
    m.predicter.Prediction.viz_attn = True
    imgs = [synth.synth_images(3, 48, 64, seed=701).cuda(), synth.staggered_images().cuda(),
            synth.synth_images(2, 48, 64, seed=702).cuda()]
    ref = _sync_ref(m, imgs, L, True)
    assert ref[0][1].shape[-1] == V1
    m.pipelined, m.decode_chains = True, 2
    outs = [_forward(m, x, L, True) for x in imgs]
    m.synchronize()
    exits = []
    for (p, l, a, add), r in zip(outs, ref):
        assert _same((p, l, a), r)
        assert add["decode"].steps() == _ref_steps(r[0], True)
        exits.append(add["decode"].steps())
    print(f"V = {V1}: step counts {exits} of {L + 1}")
    assert min(exits) < L + 1  # the early exit is exercised in the wide build


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_beam_search_ignores_pipelined():
    _, m = engine_model("TS0", 14, 1234, 0.3, beam_size=5)
    img = synth.synth_images(1, 48, 64, seed=1050).cuda()
    text = torch.zeros(1, 15, dtype=torch.long, device="cuda")
    with torch.no_grad():
        s0, v0, a0 = m(img, text, is_train=False, is_test=True)
        m.pipelined, m.decode_chains = True, 2
        eng = m.engine()
        t0 = int(eng.lib.d2t_decode_last_ticket(eng.ctx))
        s1, v1, a1 = m(img, text, is_train=False, is_test=True)
    assert a0 == {} and a1 == {} and torch.equal(s0, s1) and float(v0) == float(v1)
    assert int(eng.lib.d2t_decode_last_ticket(eng.ctx)) == t0  # no asynchronous decode was submitted
    # beam_size is read on every call: a search right behind pipelined greedy forwards of the same model (they share chain
    # 0's key-projection workspace) still returns the same hypothesis, and the greedy results are intact
    m.opt["beam_size"] = 1
    imgs = [synth.synth_images(4, 48, 64, seed=1060 + i).cuda() for i in range(3)]
    ref = _sync_ref(m, imgs, 14, False)
    m.pipelined = True
    outs = [_forward(m, x, 14, False) for x in imgs]
    m.opt["beam_size"] = 5
    with torch.no_grad():
        s2, v2, a2 = m(img, text, is_train=False, is_test=True)
    assert a2 == {} and torch.equal(s0, s2) and float(v0) == float(v2)
    m.synchronize()
    for (p, l, _, add), r in zip(outs, ref):
        assert add["decode"].done() and torch.equal(p, r[0]) and torch.equal(l, r[1])


def test_tfm_context_refuses_the_attn_submit():
    _, m = engine_model("T2", 12)
    eng = m.engine()
    img = synth.synth_images(2, 48, 64, seed=1000).cuda()
    with torch.no_grad():
        mem = m.forward_encoder(img)[0].contiguous()
    B, T, _ = mem.shape
    tok = torch.zeros(B, 13, dtype=torch.int64, device="cuda")
    probs = torch.zeros(B, 13, eng.cfg.vocab, device="cuda")
    t = C.c_int64(-1)
    t0 = int(eng.lib.d2t_decode_last_ticket(eng.ctx))
    rc = eng.lib.d2t_decode_attn_greedy_submit(eng.ctx, _lib.ptr(mem), B, T, 1, _lib.ptr(tok), _lib.ptr(probs), None,
                                               _lib.stream_of(mem), C.byref(t))
    assert rc == 4  # D2T_ESTATE
    assert b"Attn decoder" in eng.lib.d2t_last_error(eng.ctx)
    assert int(t.value) == -1 and int(eng.lib.d2t_decode_last_ticket(eng.ctx)) == t0
    # and the Attn context refuses a memory it cannot take, before enqueueing
    _, ma = engine_model("TS0", 12)
    ea = ma.engine()
    rc = ea.lib.d2t_decode_attn_greedy_submit(ea.ctx, _lib.ptr(mem), B, 0, 1, _lib.ptr(tok), _lib.ptr(probs), None,
                                              _lib.stream_of(mem), C.byref(t))
    assert rc == 1 and int(ea.lib.d2t_decode_last_ticket(ea.ctx)) == 0  # D2T_EINVAL
