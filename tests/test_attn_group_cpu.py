"""No GPU, no library call: how a pipelined LSTM-attention head collects greedy forwards into decode groups
(Model.attn_decode_group / attn_decode_group_rows) and when it launches them -- on the count, the row budget, a change of
is_test, synchronize() and a handle's wait() --, the viz_attn flush, the defaults (the calls made are the ones made without
the switch), and the declarations of the new entries.  Model runs against the recording stand-in of
tests/test_model_host_cpu.py, extended by the calls of these heads."""
import os
import re

import pytest
import torch

import test_model_host_cpu as host
from doc2tex_amd import Model, _lib, build_model, synth
from doc2tex_amd.engine import ragged_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, V = 9, 11  # batch_max_length 8; FakeEngine's vocabulary


class FakeAttnEngine(host.FakeEngine):
    def supports_ragged_attn_greedy(self):
        self._call("supports_ragged_attn_greedy")
        return host.FakeEngine.supports.get("ragged_attn_greedy", True)

    def decode_attn_greedy_async(self, memory, is_test, return_alpha=False):
        host.FakeEngine.ticket += 1
        B, T, _ = memory.shape
        self._call("decode_attn_greedy_async", tuple(memory.shape), bool(is_test), bool(return_alpha))
        out = (torch.zeros(B, S, dtype=torch.int64), torch.zeros(B, S, V))
        if return_alpha:
            out += (torch.zeros(B, S, self.attn_keys(T)),)
        return out + (host.FakeEngine.ticket,)

    def decode_attn_greedy_ragged_into(self, packed, layout, tokens, probs, is_test=False):
        host.FakeEngine.ticket += 1
        tokens.copy_(torch.arange(tokens.shape[0]).unsqueeze(1).expand_as(tokens))  # row r of the launch reads r
        self._call("decode_attn_greedy_ragged_into", packed.clone(), list(layout), tuple(tokens.shape), tuple(probs.shape), bool(is_test))
        return host.FakeEngine.ticket

    def decode_steps(self, ticket):
        return host.FakeEngine.steps.get(ticket, [self.cfg.batch_max_length + 1])


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(build_model, "Engine", FakeAttnEngine)
    F = host.FakeEngine
    F.log, F.ticket, F.supports, F.fail_once, F.steps = [], 0, {}, set(), {}
    return F


def _model(name="TS0"):
    return Model(synth.make_config(name, max_seq_len=8)).eval()


def _forward(m, B, T, is_test=False, seed=0):
    mem = torch.randn(B, T, 256, generator=torch.Generator().manual_seed(1000 * B + T + seed))
    p, l, attn, extra = m.forward_decoder(mem, torch.zeros(B, 1, dtype=torch.long), is_train=False, is_test=is_test)
    assert attn is None
    return mem, p, l, extra["decode"]


DECODES = ("decode_attn_greedy_async", "decode_attn_greedy_ragged_into", "decode_greedy_async_into", "decode_greedy_ragged_into",
           "decode_wait", "wait_ticket", "supports_ragged_attn_greedy")


def _calls(fake, keep=DECODES[:6]):
    out = [c for c in fake.log if c[0] in keep]
    del fake.log[:]
    return out


def _shape(call):
    return (call[0], tuple(call[1].shape)) + call[2:]


def test_defaults_make_the_calls_made_today(fake):
    m = _model()
    assert m.attn_decode_group == 1 and m.attn_decode_group_rows == 256
    m.pipelined = True
    outs = [_forward(m, 3, 10), _forward(m, 2, 7, is_test=True)]
    assert _calls(fake, DECODES) == [("decode_attn_greedy_async", (3, 10, 256), False, False),
                                     ("decode_attn_greedy_async", (2, 7, 256), True, False)]  # the engine is not even asked
    assert [o[3].ticket for o in outs] == [1, 2] and m._group is None
    assert [tuple(t.shape) for t in outs[1][3].result()] == [(2, S), (2, S, V)]
    m.synchronize()
    assert _calls(fake) == [("decode_wait", True)]


@pytest.mark.parametrize("name", ["TS0", "TO0"])
def test_the_tfm_switches_stay_ignored_by_these_heads(fake, name):
    m = _model(name)
    assert (m.attn_decode_group, m.attn_decode_group_rows) == (1, 256)  # these heads' own switch is off
    m.pipelined, m.decode_group, m.decode_group_mixed, m.decode_group_rows = True, 4, True, 64
    _forward(m, 3, 10), _forward(m, 3, 10, seed=1)
    assert _calls(fake, DECODES) == [("decode_attn_greedy_async", (3, 10, 256), False, False)] * 2 and m._group is None


def test_collection_and_launch_on_the_count(fake):
    m = _model()
    m.pipelined, m.attn_decode_group = True, 3
    sizes = [(3, 10), (2, 7), (4, 10), (1, 26)]
    outs = [_forward(m, B, T, is_test=True) for B, T in sizes]
    calls = _calls(fake)
    assert [_shape(c) for c in calls] == [("decode_attn_greedy_ragged_into", (30 + 14 + 40, 256), sizes[:3], (9, S), (9, S, V), True)]
    assert torch.equal(calls[0][1], torch.cat([o[0].reshape(-1, 256) for o in outs[:3]]))
    # the layout handed to the engine is ragged_tables' input: its tables cover exactly the packed rows and the output rows
    tab = ragged_tables(calls[0][2])
    assert tab["mem_rows"] == calls[0][1].shape[0] and tab["rows"] == 9 and tab["batch_rows"] == [3, 2, 4]
    assert tab["row0"] == [0, 10, 20, 30, 37, 44, 54, 64, 74] and tab["row_batch"] == [0, 0, 0, 1, 1, 2, 2, 2, 2]
    assert [o[3].ticket for o in outs] == [1, 1, 1, None]
    # full-size views of the launch's rows, in batch order; each handle reads its own batch's step count
    assert [o[1][:, 0].tolist() for o in outs[:3]] == [[0, 1, 2], [3, 4], [5, 6, 7, 8]]
    assert all(tuple(o[1].shape) == (B, S) and tuple(o[2].shape) == (B, S, V) for o, (B, _) in zip(outs, sizes))
    fake.steps = {1: [4, 9, 6], 2: [5]}
    assert [o[3].steps() for o in outs[:3]] == [4, 9, 6]
    p, l = outs[0][3].result()
    assert p is outs[0][1] and l is outs[0][2]  # full size, as these heads' synchronous forward returns them
    m.synchronize(host_sync=False)  # launches the group of one batch that is still collecting
    calls = _calls(fake)
    assert [_shape(c) for c in calls[:1]] == [("decode_attn_greedy_ragged_into", (26, 256), [(1, 26)], (1, S), (1, S, V), True)]
    assert calls[1:] == [("decode_wait", False)] and outs[3][3].ticket == 2 and outs[3][3].steps() == 5


def test_launch_on_the_row_budget_and_on_an_is_test_change(fake):
    m = _model()
    m.pipelined, m.attn_decode_group, m.attn_decode_group_rows = True, 6, 8
    sizes = [(3, 10), (2, 7), (4, 10), (9, 5), (1, 5)]
    outs = [_forward(m, B, T) for B, T in sizes]
    assert [_shape(c)[1:3] for c in _calls(fake)] == [((44, 256), [(3, 10), (2, 7)]),  # 5 + 4 rows > 8
                                                      ((40, 256), [(4, 10)]),         # 4 + 9 rows > 8
                                                      ((45, 256), [(9, 5)])]          # beyond the budget: a group of its own
    assert [o[3].ticket for o in outs] == [1, 1, 2, 3, None]
    a = _forward(m, 2, 5, is_test=True)  # is_test flips: what has been collected goes first
    assert [_shape(c)[1:] for c in _calls(fake)] == [((5, 256), [(1, 5)], (1, S), (1, S, V), False)]
    b = _forward(m, 2, 6, is_test=True)
    assert _calls(fake) == [] and a[3].ticket is None and a[3].done() is False
    m.synchronize(flush=False)  # orders after what has been launched, launches nothing
    assert _calls(fake) == [("decode_wait", True)] and a[3].ticket is None
    b[3].wait(host_sync=True)  # a handle launches its own group
    calls = _calls(fake)
    assert [_shape(c)[1:] for c in calls[:1]] == [((22, 256), [(2, 5), (2, 6)], (4, S), (4, S, V), True)]
    assert calls[1:] == [("wait_ticket", 5, True)] and a[3].ticket == b[3].ticket == 5
    assert b[1][:, 0].tolist() == [2, 3]


def test_the_engine_limits_cap_the_group(fake):
    m = _model()
    m.pipelined, m.attn_decode_group, m.attn_decode_group_rows = True, 500, 5000
    for i in range(65):
        _forward(m, 1, 4, seed=i)
    calls = _calls(fake)
    assert len(calls) == 1 and len(calls[0][2]) == 64  # 64 batches per launch at most
    m.launch_decode_group()
    _calls(fake)
    _forward(m, 1000, 2), _forward(m, 25, 2)  # 1024 rows per launch at most, whatever the budget says
    assert [_shape(c)[2] for c in _calls(fake)] == [[(1000, 2)]]
    _forward(m, 1025, 2)  # more rows than a launch takes: what was collected goes first, then the forward alone, as today
    assert [c[0] for c in _calls(fake)] == ["decode_attn_greedy_ragged_into", "decode_attn_greedy_async"]


def test_a_memory_length_the_engine_refuses_never_joins_a_group(fake):
    """more than 4096 keys, or none: the forward launches what has been collected and goes to the ungrouped call, whose
    refusal is then its own -- the collected forwards keep their tickets"""
    m = _model()
    m.pipelined, m.attn_decode_group = True, 4
    for T in (4098, 1):  # FakeEngine.attn_keys: T - 1
        a = _forward(m, 3, 10)
        b = _forward(m, 1, T)
        calls = _calls(fake)
        assert [c[0] for c in calls] == ["decode_attn_greedy_ragged_into", "decode_attn_greedy_async"] and calls[0][2] == [(3, 10)]
        assert a[3].ticket is not None and b[3].ticket == a[3].ticket + 1 and m._group is None
    c = _forward(m, 1, 4097)  # 4096 keys: the longest memory a group takes
    assert _calls(fake) == [] and c[3].ticket is None


def test_a_viz_attn_forward_flushes_and_runs_alone(fake):
    m = _model()
    m.pipelined, m.attn_decode_group = True, 4
    a, b = _forward(m, 3, 10, is_test=True), _forward(m, 2, 7, is_test=True)
    m.predicter.Prediction.viz_attn = True
    c = _forward(m, 2, 10, is_test=True)
    calls = _calls(fake)
    assert [_shape(x) if x[0].endswith("into") else x for x in calls] == [
        ("decode_attn_greedy_ragged_into", (44, 256), [(3, 10), (2, 7)], (5, S), (5, S, V), True),
        ("decode_attn_greedy_async", (2, 10, 256), True, True)]  # order preserved: the collected forwards complete first
    assert tuple(m.predicter.Prediction.alpha_stores.shape) == (2, S, 9, 1)
    assert [a[3].ticket, b[3].ticket, c[3].ticket] == [1, 1, 2]
    m.predicter.Prediction.viz_attn = False
    d = _forward(m, 2, 10, is_test=True)
    assert _calls(fake) == [] and d[3].ticket is None  # collecting again


def test_a_context_without_the_groups_serves_as_before(fake):
    fake.supports = {"ragged_attn_greedy": False}
    m = _model()
    m.pipelined, m.attn_decode_group = True, 3
    _forward(m, 3, 10), _forward(m, 2, 7)
    assert [c[0] for c in _calls(fake, DECODES)] == ["supports_ragged_attn_greedy", "decode_attn_greedy_async"] * 2


def test_synchronous_forwards_and_the_tfm_head_are_untouched(fake):
    m = host._model()  # T2: the TFM head does not read the new attributes
    assert m.attn_decode_group == 1
    m.pipelined, m.attn_decode_group, m.decode_group = True, 4, 2
    host._forward(m, 3, 20), host._forward(m, 3, 20, seed=1)
    assert [c[0] for c in _calls(fake, DECODES)] == ["decode_greedy_async_into"]


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def _declaration(name):
    text = open(os.path.join(ROOT, "include", "d2t.h")).read()
    m = re.search(r"\n(?:int|int32_t|int64_t) " + name + r"\(([^;]*)\);", text)
    assert m, f"{name} is not declared in include/d2t.h"
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_the_new_entries_are_declared_and_bound():
    args = _declaration("d2t_decode_attn_greedy_submit_ragged")
    assert len(args) == len(_lib.SIGNATURES["d2t_decode_attn_greedy_submit_ragged"][1]) == 10
    assert args[3] == "const int32_t* batch_rows" and args[4] == "const int32_t* batch_T" and args[5] == "int32_t is_test"
    assert len(_declaration("d2t_decode_attn_supports_ragged_greedy")) == len(_lib.SIGNATURES["d2t_decode_attn_supports_ragged_greedy"][1]) == 1
    assert len(_declaration("d2t_op_attn_decode_group")) == len(_lib.SIGNATURES["d2t_op_attn_decode_group"][1]) == 8
