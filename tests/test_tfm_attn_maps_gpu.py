"""GPU: cross-attention maps of the TFM head (viz_attn on the head, Engine.decode_cross_attention underneath): parity with the
reference's maps (tests/golden/tfmattn_*.npz, tools/make_golden_tfm_attn.py) in fp32 and against its float64 run, the decode
itself bit for bit what it is without the flag, shapes and placement of alpha_stores / decoder_attn / cross_attn, a batch
against its rows alone, the pipelined forward, and the refusals."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, engine_model
from doc2tex_amd import _lib, synth

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "tfmattn_cases.json")) as f:
    CASES = {c["case"]: c for c in json.load(f)["cases"]}
# Engine maps against the reference's fp32 maps; the project's bar for attention probabilities (tests/test_vit_attn_maps_gpu.py).
# Measured on an MI355X, worst case 2.1e-5 (tfmattn_t1; tfmattn_t1_beam3 1.6e-5, the T2 cases 4.2e-7 ... 1.1e-6, C2 rows and row
# maxima 5.0e-8, VBT 1.1e-8), the same in both arithmetics: a model in the default split-bf16 arithmetic replays its maps over
# the crop's memory encoded in fp32 (Model._exact_memory).  Over the split-bf16 memory itself tfmattn_t1 was 2.9e-4 and
# tfmattn_t1_beam3 1.7e-4 -- above the bar, which is why; T2 7.9e-6, C2 3.5e-7.
ATOL = 1e-4
GO = _lib.TOK_GO


def _load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _inputs(c):
    cfg = synth.make_config(c["config"])
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"], channels=synth.image_channels(cfg)).cuda()
    return img, torch.full((c["B"], 1), GO, dtype=torch.long, device="cuda")


def _model(c, precision="default"):
    _, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], end_bias=c["end_bias"], beam_size=c["beam_size"] or 1)
    if precision == "fp32":
        m.conv_precision = "fp32"
    return m


def _forward(m, c, viz, heads=False, layers=None):
    pred = m.predicter.Prediction
    pred.viz_attn, pred.viz_attn_heads, pred.viz_attn_layers = viz, heads, layers
    img, text = _inputs(c)
    with torch.no_grad():
        out = m(img, text, is_train=False, is_test=c["is_test"])
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _decoded(name, precision):
    """One flagged forward per (fixture, arithmetic), shared by the tests that read it: (tokens, maps [nl, B, H, steps, T])."""
    c = CASES[name]
    prediction, _, add = _forward(_model(c, precision), c, True, heads=True)
    return prediction.cpu().numpy(), add["cross_attn"].permute(1, 0, 2, 3, 4).contiguous().cpu().numpy()


@pytest.mark.parametrize("precision", ["default", "fp32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_maps_match_reference(name, precision):
    c, z = CASES[name], _load(name)
    tokens, maps = _decoded(name, precision)
    assert np.array_equal(tokens, z["tokens"])
    assert maps.shape == (c["layers"], c["B"], c["heads"], c["steps"], c["T"])
    assert float(np.abs(maps.astype(np.float64).sum(-1) - 1).max()) <= 1e-5
    if c["kind"] == "full":
        err = float(np.abs(maps - z["maps32"]).max())
    else:
        rows = c["rows"]
        err = max(float(np.abs(maps[:, :, :, rows] - z["maps32"]).max()), float(np.abs(maps.max(-1) - z["max"]).max()))
        # the argmax may differ only where two keys are within rounding of each other
        diff = maps.argmax(-1) != z["argmax"]
        if diff.any():
            picked = np.take_along_axis(maps, z["argmax"][..., None].astype(np.int64), -1)[..., 0]
            assert float(np.abs(picked - maps.max(-1))[diff].max()) <= ATOL
    print(f"{name} ({precision}): max |dp| = {err:.2e}")
    assert err <= ATOL


@pytest.mark.parametrize("name", sorted(CASES))
def test_maps_match_float64(name):
    """fp32 arithmetic against the reference's float64 maps: within 8 x what the reference's own fp32 run is off by."""
    c, z = CASES[name], _load(name)
    _, maps = _decoded(name, "fp32")
    got = maps if c["kind"] == "full" else maps[:, :, :, c["rows"]]
    err = float(np.abs(got.astype(np.float64) - z["maps64"].astype(np.float64)).max())
    print(f"{name}: max |p - p64| = {err:.2e}, e_ref = {c['e_ref']:.2e}")
    assert err <= 8 * c["e_ref"] + 1e-6


@pytest.mark.parametrize("name", ["tfmattn_t2", "tfmattn_t1", "tfmattn_t2_early", "tfmattn_t2_beam3", "tfmattn_t1_beam3", "tfmattn_vbt"])
def test_decode_is_unchanged_by_the_flag(name):
    c = CASES[name]
    m = _model(c)
    p0, l0, a0 = _forward(m, c, False)
    assert "cross_attn" not in a0 and "decoder_attn" not in a0
    p1, l1, a1 = _forward(m, c, True)
    p2, l2, _ = _forward(m, c, False)  # a decode after a replay
    assert "cross_attn" in a1
    for p, l in ((p1, l1), (p2, l2)):
        assert torch.equal(p, p0)
        assert torch.equal(l, l0) if torch.is_tensor(l0) else l == l0  # beam: the score, a Python float
    assert np.array_equal(p0.cpu().numpy(), _load(name)["tokens"])


def test_greedy_shapes_and_placement():
    c = CASES["tfmattn_t2"]
    m = _model(c)
    pred = m.predicter.Prediction
    B, steps, T, nl, H = c["B"], c["steps"], c["T"], c["layers"], c["heads"]
    _, _, add = _forward(m, c, True)
    cross = add["cross_attn"]
    assert tuple(cross.shape) == (B, nl, steps, T) and "decoder_attn" not in add
    assert tuple(pred.alpha_stores.shape) == (B, steps, T, 1) and torch.equal(pred.alpha_stores[..., 0], cross[:, -1])
    _, _, add_h = _forward(m, c, True, heads=True)
    heads = add_h["cross_attn"]
    assert tuple(heads.shape) == (B, nl, H, steps, T)
    assert float((heads.mean(2) - cross).abs().max()) <= 1e-6
    assert tuple(pred.alpha_stores.shape) == (B, steps, T, 1) and float((pred.alpha_stores[..., 0] - cross[:, -1]).abs().max()) <= 1e-6
    # layer subsets, negative indices, order and repeats; alpha_stores stays the LAST layer's map whatever is asked for
    for layers, want in (([0], [0]), ([-1], [nl - 1]), ([-1, 0, 0], [0, nl - 1]), ((1,), [1])):
        _, _, add_l = _forward(m, c, True, layers=layers)
        assert torch.equal(add_l["cross_attn"], cross[:, want])
        assert torch.equal(pred.alpha_stores[..., 0], cross[:, -1])
    with pytest.raises(ValueError):
        _forward(m, c, True, layers=[nl])
    # an is_test decode that stops early: only the rows of the steps that ran
    ce = CASES["tfmattn_t2_early"]
    me = _model(ce)
    pe, _, add_e = _forward(me, ce, True)
    assert pe.shape[1] == ce["steps"] < ce["max_seq_len"] + 1
    assert tuple(add_e["cross_attn"].shape) == (ce["B"], ce["layers"], ce["steps"], ce["T"])
    assert tuple(me.predicter.Prediction.alpha_stores.shape) == (ce["B"], ce["steps"], ce["T"], 1)


@pytest.mark.parametrize("name", ["tfmattn_t2_beam3", "tfmattn_t2_beam3_end"])
def test_beam_map_lies_on_the_grid(name):
    c = CASES[name]
    m = _model(c)
    seq, score, add = _forward(m, c, True)
    w, h = c["output_shape"]
    assert seq.shape == (1, c["steps"]) and add["feat_width"] == w and add["feat_height"] == h
    cross = add["cross_attn"]
    assert tuple(cross.shape) == (1, c["layers"], c["steps"], c["T"]) and c["T"] == w * h + 1
    assert tuple(add["decoder_attn"].shape) == (c["steps"], w, h)
    assert torch.equal(add["decoder_attn"], cross[0, -1, :, 1:].reshape(-1, w, h))  # the cls row dropped
    # beam_search_batch with the flag: the same map per sample, not yet on the grid
    img, _ = _inputs(c)
    with torch.no_grad():
        (bseq, bscore, battn), = m.beam_search_batch(img, c["beam_size"])
    assert torch.equal(bseq, seq) and bscore == score and torch.equal(battn, cross[0, -1])
    m.predicter.Prediction.viz_attn = False
    with torch.no_grad():
        assert len(m.beam_search_batch(img, c["beam_size"])[0]) == 2
        assert torch.equal(m.beam_search_batch(img, c["beam_size"], return_attn=True)[0][2], battn)


def test_a_memory_without_a_grid_returns_no_grid_keys():
    c = CASES["tfmattn_vbt"]
    _, _, add = _forward(_model(c), c, True)
    assert sorted(add) == ["cross_attn"] and tuple(add["cross_attn"].shape) == (c["B"], c["layers"], c["steps"], c["T"])


@pytest.mark.parametrize("name", ["tfmattn_t2", "tfmattn_t1"])
def test_a_batch_equals_its_rows_alone(name):
    c, z = CASES[name], _load(name)
    m = _model(c)
    img, text = _inputs(c)
    with torch.no_grad():
        memory = m.forward_encoder(img)[0].contiguous()
    eng = m.engine()
    tokens_in = torch.cat([text, torch.from_numpy(z["tokens"].astype(np.int64)).cuda()[:, :-1]], dim=1)
    for per_head in (False, True):
        whole = eng.decode_cross_attention(memory, tokens_in, per_head=per_head)
        for b in range(c["B"]):
            alone = eng.decode_cross_attention(memory[b:b + 1], tokens_in[b:b + 1], per_head=per_head)
            assert torch.equal(alone[0], whole[b])
    # a shorter replay is the prefix of the longer one (causal: row t depends on tokens 0 .. t only)
    assert torch.equal(eng.decode_cross_attention(memory, tokens_in[:, :3]), eng.decode_cross_attention(memory, tokens_in)[:, :, :3])


def test_a_pipelined_forward_with_the_flag_runs_alone():
    c = CASES["tfmattn_t2"]
    m = _model(c)
    want_p, want_l, want_add = _forward(m, c, True)
    m.pipelined, m.decode_group = True, 2
    p0, l0, add0 = _forward(m, c, False)  # collected: the group is not full
    assert add0["decode"].done() is False
    p1, l1, add1 = _forward(m, c, True)
    assert "decode" not in add1 and torch.equal(p1, want_p) and torch.equal(l1, want_l)
    assert torch.equal(add1["cross_attn"], want_add["cross_attn"])
    assert add0["decode"].done() is True  # what had been collected was launched and has completed
    r0 = add0["decode"].result()
    assert torch.equal(r0[0], want_p) and torch.equal(r0[1], want_l)
    m.synchronize()


def test_refusals_leave_the_decode_alone():
    c = CASES["tfmattn_t2"]
    m = _model(c)
    p0, l0, _ = _forward(m, c, False)
    img, text = _inputs(c)
    with torch.no_grad():
        memory = m.forward_encoder(img)[0].contiguous()
    eng, lib = m.engine(), _lib.require_device()
    S, nl = c["max_seq_len"] + 1, c["layers"]
    tok = torch.full((c["B"], S), 5, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        eng.decode_cross_attention(memory, tok, layers=[nl])
    with pytest.raises(ValueError):
        eng.decode_cross_attention(memory, tok, layers=[])
    with pytest.raises(ValueError):
        eng.decode_cross_attention(memory, torch.cat([tok, tok], dim=1))  # S too long
    with pytest.raises(RuntimeError, match="vocabulary"):
        eng.decode_cross_attention(memory, torch.full_like(tok, eng.cfg.vocab))

    def raw(S=S, mask=1, per_head=0, mem=memory, T=None):
        maps = torch.empty(16, device="cuda")  # never written: every call below is refused
        return lib.d2t_decode_cross_attention(eng.ctx, _lib.ptr(mem), c["B"], mem.shape[1] if T is None else T, _lib.ptr(tok), S, mask,
                                              per_head, _lib.ptr(maps), _lib.stream_of(mem))
    assert raw(S=0) == _lib.D2T_EINVAL and raw(S=S + 1) == _lib.D2T_EINVAL
    assert raw(mask=0) == _lib.D2T_EINVAL and raw(mask=1 << nl) == _lib.D2T_EINVAL
    assert raw(T=4097) == _lib.D2T_EINVAL
    # the budget: three rows of 401 steps over 4096 tokens and two layers are 39 MB as a head mean and 315 MB per head
    # (the reference's word position table has 500 rows: max_seq_len stays below 499)
    cb = dict(c, max_seq_len=400)
    mb = _model(cb)
    engb = mb.engine()
    big, tokb = torch.zeros(3, 4096, memory.shape[2], device="cuda"), torch.full((3, 401), 5, dtype=torch.int64, device="cuda")
    assert engb.cross_attention_bytes(3, 401, 4096, nl, False) <= _lib.ATTN_MAP_BUDGET < engb.cross_attention_bytes(3, 401, 4096, nl, True)
    with pytest.raises(ValueError, match="split the batch"):
        engb.decode_cross_attention(big, tokb, per_head=True)
    maps = torch.empty(16, device="cuda")
    rc = lib.d2t_decode_cross_attention(engb.ctx, _lib.ptr(big), 3, 4096, _lib.ptr(tokb), 401, 3, 1, _lib.ptr(maps), _lib.stream_of(big))
    assert rc == _lib.D2T_EINVAL and b"split the batch" in lib.d2t_last_error(engb.ctx)
    # a context of another head
    _, ma = engine_model("TS0", 12)
    enga = ma.engine()
    with pytest.raises(RuntimeError, match="TFM"):
        enga.decode_cross_attention(memory, tok)
    rc = lib.d2t_decode_cross_attention(enga.ctx, _lib.ptr(memory), c["B"], memory.shape[1], _lib.ptr(tok), S, 1, 0, _lib.ptr(maps),
                                        _lib.stream_of(memory))
    assert rc == _lib.D2T_ESTATE
    p1, l1, _ = _forward(m, c, False)
    assert torch.equal(p1, p0) and torch.equal(l1, l0)
