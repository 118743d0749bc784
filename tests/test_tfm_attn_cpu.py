"""No GPU: the TFM cross-attention map fixtures (tests/golden/tfmattn_*), the host logic of viz_attn on the TFM head (Model
against a recording stand-in for its engine, as tests/test_model_host_cpu.py does), the budget arithmetic of
Engine.decode_cross_attention, and the new symbols in the header and the ctypes table."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT
from doc2tex_amd import Model, _lib, build_model, synth
from doc2tex_amd.engine import Engine, config_from_opt

with open(os.path.join(GOLD, "tfmattn_cases.json")) as f:
    CASES = {c["case"]: c for c in json.load(f)["cases"]}


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_what_it_should():
    by = {(c["config"], c["beam_size"], c["is_test"]) for c in CASES.values()}
    assert {("T2", 0, False), ("T1", 0, False), ("T2", 0, True), ("T2", 3, False), ("T1", 3, False), ("C2", 0, False),
            ("VBT", 0, False)} <= by
    assert CASES["tfmattn_t1"]["T"] == 17 and CASES["tfmattn_t2"]["T"] == 10 and CASES["tfmattn_c2"]["T"] == 261
    assert CASES["tfmattn_vbt"]["output_shape"] is None and CASES["tfmattn_c2"]["kind"] == "sampled"
    assert CASES["tfmattn_t2_early"]["steps"] < CASES["tfmattn_t2_early"]["max_seq_len"] + 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_is_sane(name):
    c, z = CASES[name], np.load(os.path.join(GOLD, name + ".npz"))
    assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < 400 * 1024
    rows = c["steps"] if c["kind"] == "full" else len(c["rows"])
    shape = (c["layers"], c["B"], c["heads"], rows, c["T"])
    assert z["maps32"].shape == shape and z["maps32"].dtype == np.float32
    assert z["maps64"].shape == shape and str(z["maps64"].dtype) == c["maps64_dtype"]
    assert z["tokens"].shape == (c["B"], c["steps"])
    assert 0 < c["e_ref"] < 1e-4 and c["row_sum_max_err"] < 1e-5 and c["torch"]
    assert float(np.abs(z["maps32"].astype(np.float64).sum(-1) - 1).max()) < 1e-5
    assert float(np.abs(z["maps64"].astype(np.float64).sum(-1) - 1).max()) < 1e-5
    assert float(np.abs(z["maps32"] - z["maps64"]).max()) <= c["e_ref"] + 1e-7  # (maps64 may be stored rounded to fp32)
    assert z["maps32"].min() >= 0
    if c["kind"] == "sampled":
        full = (c["layers"], c["B"], c["heads"], c["steps"])
        assert z["argmax"].shape == full and z["max"].shape == full
        assert np.array_equal(z["maps32"].max(-1), z["max"][..., c["rows"]])
    if c["beam_size"]:
        assert c["B"] == 1 and "score" in c


# ---- host logic -------------------------------------------------------------------------------------------------------
class StubEngine:
    """Records the decode calls Model makes; the maps are a function of the request."""
    log = []
    cross_attention_layers = Engine.cross_attention_layers
    cross_attention_bytes = Engine.cross_attention_bytes

    def __init__(self, opt, device=None):
        self.cfg = config_from_opt(opt)
        self.cfg.vocab = 11
        self.device = 0
        self.applied = {}

    def __getattr__(self, name):
        if name.startswith("set_"):
            return lambda *a, **k: None
        raise AttributeError(name)

    def sync_weights(self, module, finalize=True):
        pass

    def supports_ragged_groups(self):
        return True

    def decode_greedy(self, memory, start, is_test):
        StubEngine.log.append(("decode_greedy", tuple(memory.shape), start.tolist(), is_test))
        B, S = memory.shape[0], 4 if is_test else self.cfg.max_seq_len + 1
        return torch.arange(B * S).reshape(B, S) % 7 + 3, torch.zeros(B, S, 11)

    def decode_beam(self, memory, beam):
        StubEngine.log.append(("decode_beam", tuple(memory.shape), beam))
        return torch.LongTensor([[5, 6, 2]]), -1.5

    def decode_beam_batch(self, memory, beam):
        StubEngine.log.append(("decode_beam_batch", tuple(memory.shape), beam))
        return [(torch.LongTensor([[5, 6, 2][:3 - i]]), -1.5 - i) for i in range(memory.shape[0])]

    def decode_cross_attention(self, memory, tokens_in, layers=None, per_head=False):
        StubEngine.log.append(("decode_cross_attention", tuple(memory.shape), tokens_in.tolist(), list(layers), per_head))
        B, T, S = memory.shape[0], memory.shape[1], tokens_in.shape[1]
        shape = (B, len(layers)) + ((self.cfg.dec_heads,) if per_head else ()) + (S, T)
        g = torch.Generator().manual_seed(int(memory.sum()) + 31 * S)
        base = torch.rand(shape, generator=g)
        return base + torch.tensor(layers, dtype=torch.float32).reshape((1, -1) + (1,) * (len(shape) - 2))  # layer l lies in [l, l + 1)

    def encode(self, image, attn_maps=None):
        StubEngine.log.append(("encode", tuple(image.shape), self.applied.get("conv_precision")))
        return _memory(image.shape[0]) + 0.25, (3, 3), (0, 0)

    def decode_greedy_async_into(self, memory, start, tokens, logits, is_test=False, rows_per_batch=0):
        StubEngine.log.append(("decode_greedy_async_into", tuple(memory.shape)))
        return 1

    def decode_wait(self, host_sync=False):
        StubEngine.log.append(("decode_wait", host_sync))

    def ticket_done(self, ticket):
        return True


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(build_model, "Engine", StubEngine)
    StubEngine.log = []
    return StubEngine


def _model(name="T2", beam=None):
    return Model(synth.make_config(name, max_seq_len=8, beam_size=beam)).eval()


def _memory(B=2, T=10):
    return torch.arange(B, dtype=torch.float32).reshape(B, 1, 1).expand(B, T, 256).contiguous()


GO = torch.full((2, 1), _lib.TOK_GO, dtype=torch.long)


def test_without_the_flag_the_decoder_makes_the_calls_it_made(stub):
    m = _model()
    assert not hasattr(m.predicter.Prediction, "viz_attn")
    for off in (None, False):
        if off is not None:
            m.predicter.Prediction.viz_attn = off
        _, _, attn, add = m.forward_decoder(_memory(), GO, is_train=False)
        assert attn is None and add == {}
    assert [c[0] for c in stub.log] == ["decode_greedy", "decode_greedy"]
    assert not hasattr(m.predicter.Prediction, "alpha_stores")
    mb = _model(beam=3)
    del stub.log[:]
    assert mb.forward_decoder(_memory(1), GO[:1], is_train=False)[2:] == (None, {})
    assert mb.beam_search_batch.__self__ is mb and [c[0] for c in stub.log] == ["decode_beam"]


def test_the_flag_routes_a_greedy_decode_through_the_replay(stub):
    m = _model()
    pred = m.predicter.Prediction
    pred.viz_attn = True
    for is_test in (False, True):
        del stub.log[:]
        prediction, logits, attn, add = m.forward_decoder(_memory(), GO, is_train=False, is_test=is_test)
        steps = prediction.shape[1]
        assert attn is None and sorted(add) == ["cross_attn"]
        (name, shape, tokens_in, layers, per_head), = [c for c in stub.log if c[0] == "decode_cross_attention"]
        assert [c[0] for c in stub.log] == ["decode_greedy", "decode_cross_attention"]
        assert shape == (2, 10, 256) and layers == [0, 1] and per_head is False
        assert tokens_in == torch.cat([GO, prediction[:, :-1]], dim=1).tolist()  # [start | the decode's own tokens but the last]
        assert tuple(add["cross_attn"].shape) == (2, 2, steps, 10) and steps == (4 if is_test else 9)
        assert tuple(pred.alpha_stores.shape) == (2, steps, 10, 1) and torch.equal(pred.alpha_stores[..., 0], add["cross_attn"][:, -1])
    # a layer request without the last layer: replayed with it (alpha_stores), returned without it
    pred.viz_attn_layers, pred.viz_attn_heads = [0], True
    del stub.log[:]
    _, _, _, add = m.forward_decoder(_memory(), GO, is_train=False)
    assert stub.log[-1][3:] == ([0, 1], True)
    assert tuple(add["cross_attn"].shape) == (2, 1, 8, 9, 10) and float(add["cross_attn"].max()) < 1  # layer 0 only
    assert tuple(pred.alpha_stores.shape) == (2, 9, 10, 1) and 1 <= float(pred.alpha_stores.min())  # layer 1, head mean
    pred.viz_attn_layers = [2]
    with pytest.raises(ValueError):
        m.forward_decoder(_memory(), GO, is_train=False)


def test_a_beam_hypothesis_is_replayed_from_go_and_laid_on_the_grid(stub, monkeypatch):
    m = _model(beam=3)
    m.predicter.Prediction.viz_attn = True
    mem = _memory(1)
    seq, score, attn, add = m.forward_decoder(mem, GO[:1], is_train=False)
    assert seq.tolist() == [[5, 6, 2]] and score == -1.5
    assert stub.log[-1] == ("decode_cross_attention", (1, 10, 256), [[_lib.TOK_GO, 5, 6]], [0, 1], False)
    assert tuple(attn.shape) == (3, 10) and torch.equal(attn, add["cross_attn"][0, -1])
    monkeypatch.setattr(m, "forward_encoder", lambda x: (mem, (3, 3), (0, 0)))
    _, _, out = m(torch.zeros(1, 1, 8, 8), GO[:1], is_train=False)
    assert tuple(out["decoder_attn"].shape) == (3, 3, 3) and (out["feat_width"], out["feat_height"]) == (3, 3)
    assert torch.equal(out["decoder_attn"], out["cross_attn"][0, -1, :, 1:].reshape(3, 3, 3))  # the cls row dropped
    monkeypatch.setattr(m, "forward_encoder", lambda x: (mem, None, None))  # no grid (Seq = None / BiLSTM)
    assert sorted(m(torch.zeros(1, 1, 8, 8), GO[:1], is_train=False)[2]) == ["cross_attn"]
    # beam_search_batch: one replay per sample, each over its own hypothesis
    monkeypatch.setattr(m, "forward_encoder", lambda x: (_memory(2), (3, 3), (0, 0)))
    del stub.log[:]
    res = m.beam_search_batch(torch.zeros(2, 1, 8, 8), 3)
    assert [c[2] for c in stub.log if c[0] == "decode_cross_attention"] == [[[_lib.TOK_GO, 5, 6]], [[_lib.TOK_GO, 5]]]
    assert [tuple(r[2].shape) for r in res] == [(3, 10), (2, 10)]
    m.predicter.Prediction.viz_attn = False
    assert [len(r) for r in m.beam_search_batch(torch.zeros(2, 1, 8, 8), 3)] == [2, 2]
    assert [len(r) for r in m.beam_search_batch(torch.zeros(2, 1, 8, 8), 3, return_attn=True)] == [3, 3]


def test_model_forward_replays_over_the_memory_in_exact_fp32(stub, monkeypatch):
    """Model.forward with the flag: the crop is encoded once more with conv_precision 'fp32' for the replay only -- the decode
    reads the memory of the model's own arithmetic, which is the context's setting again when the decode is enqueued."""
    m = _model()
    m.predicter.Prediction.viz_attn = True
    img = torch.zeros(2, 1, 8, 8)
    seen = []
    monkeypatch.setattr(m, "forward_encoder", lambda x: seen.append(m.engine().applied["conv_precision"]) or (_memory(2), (3, 3), (0, 0)))
    m(img, GO, is_train=False)
    names = [c[0] for c in stub.log]
    assert names == ["encode", "decode_greedy", "decode_cross_attention"] and seen == ["bf16x3"]
    assert stub.log[0] == ("encode", (2, 1, 8, 8), "fp32") and m.engine().applied["conv_precision"] == "bf16x3"
    assert m.conv_precision == "bf16x3" and m._precision_auto is True
    # the decode saw the model's memory, the replay the exact one (the stub's differ by 0.25)
    dec, rep = stub.log[1], stub.log[2]
    assert dec[1] == rep[1] == (2, 10, 256)
    del stub.log[:]
    m.conv_precision = "fp32"  # already exact: no second encode
    m(img, GO, is_train=False)
    assert [c[0] for c in stub.log] == ["decode_greedy", "decode_cross_attention"]
    m.predicter.Prediction.viz_attn = False
    del stub.log[:]
    m._conv_precision, m._precision_auto = "bf16x3", True
    m(img, GO, is_train=False)
    assert [c[0] for c in stub.log] == ["decode_greedy"]


def test_a_pipelined_forward_with_the_flag_flushes_and_runs_alone(stub):
    m = _model()
    m.pipelined, m.decode_group = True, 3
    out = m.forward_decoder(_memory(), GO, is_train=False)
    assert "decode" in out[3] and [c[0] for c in stub.log] == []  # collected, nothing launched
    m.predicter.Prediction.viz_attn = True
    _, _, _, add = m.forward_decoder(_memory(), GO, is_train=False)
    assert [c[0] for c in stub.log] == ["decode_greedy_async_into", "decode_wait", "decode_greedy", "decode_cross_attention"]
    assert stub.log[1] == ("decode_wait", True) and sorted(add) == ["cross_attn"]
    m.decode_group = 1  # pipelined without groups: the same
    del stub.log[:]
    assert sorted(m.forward_decoder(_memory(), GO, is_train=False)[3]) == ["cross_attn"]
    assert [c[0] for c in stub.log] == ["decode_wait", "decode_greedy", "decode_cross_attention"]


def test_rows_beyond_the_budget_are_replayed_in_parts(stub, monkeypatch):
    m = _model()
    m.predicter.Prediction.viz_attn = True
    one = 2 * 9 * 10 * 4  # one row: 2 layers x 9 steps x 10 tokens
    monkeypatch.setattr(_lib, "ATTN_MAP_BUDGET", 2 * one - 1)
    _, _, _, add = m.forward_decoder(_memory(3), torch.full((3, 1), 1), is_train=False)
    assert [c[1] for c in stub.log if c[0] == "decode_cross_attention"] == [(1, 10, 256)] * 3
    assert tuple(add["cross_attn"].shape) == (3, 2, 9, 10)
    monkeypatch.setattr(_lib, "ATTN_MAP_BUDGET", one - 1)
    with pytest.raises(ValueError, match="ONE sample"):
        m.forward_decoder(_memory(3), torch.full((3, 1), 1), is_train=False)


class _BareEngine(Engine):
    """Engine without a context or a library: whatever reaches either raises AttributeError."""
    def __init__(self, cfg):
        self.cfg, self.ctx = cfg, None


def test_the_budget_is_computed_in_python_before_any_device_work():
    eng = _BareEngine(config_from_opt(synth.make_config("T2", max_seq_len=400)))
    nl, H = eng.cfg.dec_layers, eng.cfg.dec_heads
    assert eng.cross_attention_bytes(3, 5, 7, 2, False) == 3 * 2 * 5 * 7 * 4
    assert eng.cross_attention_bytes(3, 5, 7, 2, True) == 3 * 2 * H * 5 * 7 * 4
    mem, tok = torch.zeros(3, 4096, 256), torch.ones(3, 401, dtype=torch.long)  # CPU tensors: never looked at
    assert eng.cross_attention_bytes(3, 401, 4096, nl, False) <= _lib.ATTN_MAP_BUDGET
    with pytest.raises(ValueError, match="split the batch"):
        eng.decode_cross_attention(mem, tok, per_head=True)
    with pytest.raises(ValueError):
        eng.decode_cross_attention(mem, torch.ones(3, 402, dtype=torch.long))  # S > max_seq_len + 1
    with pytest.raises(ValueError):
        eng.decode_cross_attention(mem, tok[:, :4], layers=[nl])
    assert eng.cross_attention_layers(None) == list(range(nl)) and eng.cross_attention_layers([-1, 0, -1]) == [0, nl - 1]
    with pytest.raises(RuntimeError, match="must be a ROCm"):  # a request within the budget goes on to the device checks
        eng.decode_cross_attention(mem, tok[:, :4])
    other = _BareEngine(config_from_opt(synth.make_config("TS0", max_seq_len=12)))
    with pytest.raises(RuntimeError, match="TFM"):
        other.decode_cross_attention(mem, tok[:, :4])


# ---- the C surface ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d2t_decode_cross_attention", "d2t_op_cross_attn_probs"])
def test_new_symbols_are_declared_and_bound(name):
    with open(os.path.join(ROOT, "include", "d2t.h")) as f:
        header = f.read()
    decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S)
    assert decl, f"{name} is not declared in include/d2t.h"
    res, args = _lib.SIGNATURES[name]
    assert res is _lib._I and len(args) == len(decl.group(1).split(","))
    assert "D2T_ATTN_MAP_BUDGET" in header and _lib.ATTN_MAP_BUDGET == 256 << 20
