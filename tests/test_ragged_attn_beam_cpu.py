"""CPU: the interface of the LSTM-attention ragged beam search -- the three C-ABI entries in the ctypes table with the
header's argument counts, the Engine methods, and Model._beam_search_mixed's routing, which needs no device to decide."""
import os
import re

import pytest
import torch

from doc2tex_amd import Model, _lib
from doc2tex_amd.engine import Engine, pack_memories

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_args(name):
    with open(os.path.join(ROOT, "include", "d2t.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/d2t.h"
    return [a for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name", ["d2t_decode_attn_beam_batch_ragged", "d2t_decode_attn_supports_ragged_beam",
                                  "d2t_op_attn_decode_ragged"])
def test_entries_are_declared_and_bound(name):
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == len(_declared_args(name)), name


def test_engine_and_model_surface():
    assert callable(Engine.decode_attn_beam_batch_ragged) and callable(Engine.supports_ragged_attn_beam)
    assert callable(Engine.decode_beam_batch_ragged) and callable(Engine.supports_ragged_beam)  # the TFM head's stay
    assert callable(Model._beam_search_mixed)


class _Eng:
    """records which search a list is routed to"""

    def __init__(self, tfm_ok, attn_ok, keys_per_T=lambda T: T - 1):
        self.tfm_ok, self.attn_ok, self.calls, self.keys = tfm_ok, attn_ok, [], keys_per_T

    def supports_ragged_beam(self):
        return self.tfm_ok

    def supports_ragged_attn_beam(self):
        return self.attn_ok

    def attn_map_bytes(self, T, beam):
        return 15 * beam * self.keys(T) * 4

    def decode_beam_batch_ragged(self, packed, lengths, beam):
        self.calls.append(("tfm", lengths, beam))
        return ["tfm"] * len(lengths)

    def decode_attn_beam_batch_ragged(self, packed, lengths, beam, return_alpha=False):
        self.calls.append(("attn", lengths, beam, return_alpha))
        return ["attn"] * len(lengths)


class _Model:
    """Model's routing methods over a stub engine and encoder: memory length = the image's width"""
    _beam_search_mixed = Model._beam_search_mixed
    _beam_search_each = Model._beam_search_each

    def __init__(self, pred, eng):
        self.stages, self._eng, self.single = {"Pred": pred}, eng, []

    def engine(self):
        return self._eng

    def forward_encoder(self, x):
        return torch.zeros(x.shape[0], x.shape[-1], 256), None, None

    def beam_search_batch(self, x, beam, return_attn=False):
        self.single.append((tuple(x.shape), beam, return_attn))
        return ["single"] * x.shape[0]


IMGS = [torch.zeros(2, 1, 8, 20), torch.zeros(1, 1, 8, 9), torch.zeros(3, 1, 8, 20)]


def test_attn_lists_go_to_the_ragged_attn_search():
    for pred in ("Attn", "Attnv2"):
        for maps in (False, True):
            eng = _Eng(False, True)
            m = _Model(pred, eng)
            assert m._beam_search_mixed(IMGS, 5, maps) == ["attn"] * 6
            assert eng.calls == [("attn", [20, 20, 9, 20, 20, 20], 5, maps)] and not m.single


def test_tfm_lists_keep_their_search_and_unserved_contexts_fall_back():
    eng = _Eng(True, False)
    m = _Model("TFM", eng)
    assert m._beam_search_mixed(IMGS, 3) == ["tfm"] * 6 and eng.calls == [("tfm", [20, 20, 9, 20, 20, 20], 3)]
    for pred, eng in (("TFM", _Eng(False, True)), ("Attnv2", _Eng(True, False))):
        m = _Model(pred, eng)
        assert m._beam_search_mixed(IMGS, 3) == ["single"] * 6
        assert not eng.calls and [s[0][0] for s in m.single] == [2, 1, 3]
    m = _Model("Attn", _Eng(False, True))
    assert m._beam_search_mixed([], 3) == []


def test_a_map_history_over_the_budget_falls_back(monkeypatch):
    eng = _Eng(False, True)
    m = _Model("Attnv2", eng)
    # 6 samples x (15 steps x beam 5 x 19 keys x 4 bytes) at the longest memory's stride
    monkeypatch.setattr(_lib, "ATTN_MAP_BUDGET", 6 * 15 * 5 * 19 * 4)
    assert m._beam_search_mixed(IMGS, 5, True) == ["attn"] * 6
    monkeypatch.setattr(_lib, "ATTN_MAP_BUDGET", 6 * 15 * 5 * 19 * 4 - 1)
    assert m._beam_search_mixed(IMGS, 5, True) == ["single"] * 6 and len(eng.calls) == 1
    assert all(s[2] for s in m.single)
    assert m._beam_search_mixed(IMGS, 5, False) == ["attn"] * 6  # without maps there is no history


def test_pack_memories_serves_as_is():
    mems = [torch.arange(2 * 3 * 256, dtype=torch.float32).view(2, 3, 256), torch.ones(1, 5, 256)]
    packed, lengths = pack_memories(mems)
    assert lengths == [3, 3, 5] and packed.shape == (11, 256)
    assert torch.equal(packed[3:6], mems[0][1]) and torch.equal(packed[6:], mems[1][0])
