"""No GPU, no library call: the host logic of Model and Engine -- which set_* calls Model.engine() makes and in what order,
how the pipelined TFM head collects forwards into decode groups and when it launches them, how beam searches are routed,
and how the engine's beam-search calls turn the arrays the library filled into results.  Model runs against a recording
stand-in for doc2tex_amd.build_model.Engine; the Engine methods run against a stand-in for the library.  The logs pinned
here were recorded before the settings table and the group object existed and hold unchanged with them."""
import ctypes as C

import pytest
import torch

from doc2tex_amd import Model, _lib, build_model, synth
from doc2tex_amd.build_model import BeamSearchHandle
from doc2tex_amd.engine import Engine, config_from_opt


class FakeEngine:
    """Records every call Model makes on its engine.  Class attributes are the script of a test (reset by `fake`)."""
    log = []
    ticket = 0
    supports = {}
    fail_once = set()
    steps = {}

    def __init__(self, opt, device=None):
        self.cfg = config_from_opt(opt)
        self.cfg.vocab = 11  # (small logits)
        self.device = 0
        self.applied = {}  # the engine's record of applied settings (unused where Model keeps that record itself)

    def _call(self, name, *args):
        FakeEngine.log.append((name,) + args)
        if name in FakeEngine.fail_once:
            FakeEngine.fail_once.discard(name)
            raise RuntimeError(f"{name} failed")

    def sync_weights(self, module, finalize=True):
        self._call("sync_weights", finalize)

    def set_reserved_blocks(self, blocks):
        self._call("set_reserved_blocks", blocks)

    def set_reserved_cus(self, cus):
        self._call("set_reserved_cus", cus)

    def set_conv_precision(self, mode):
        self._call("set_conv_precision", mode)

    def set_mixed_units(self, units):
        self._call("set_mixed_units", units)

    def set_conv_kernel(self, kind):
        self._call("set_conv_kernel", kind)

    def set_beam_shared_tile(self, on):
        self._call("set_beam_shared_tile", on)

    def set_attn_beam_device(self, on):
        self._call("set_attn_beam_device", on)

    def set_conv_fusion(self, pools=True, shortcuts=True):
        self._call("set_conv_fusion", pools, shortcuts)

    def set_decode_chains(self, chains):
        self._call("set_decode_chains", chains)

    def supports_device_attn_beam(self):
        self._call("supports_device_attn_beam")
        return FakeEngine.supports.get("device_attn_beam", False)

    def supports_ragged_groups(self):
        return FakeEngine.supports.get("ragged_groups", True)

    def supports_ragged_beam(self):
        return FakeEngine.supports.get("ragged_beam", True)

    def supports_ragged_attn_beam(self):
        return FakeEngine.supports.get("ragged_attn_beam", True)

    def _launch(self, name, memory, start, tokens, logits, *rest):
        FakeEngine.ticket += 1
        tokens.copy_(torch.arange(tokens.shape[0]).unsqueeze(1).expand_as(tokens))  # row r of the launch reads r
        self._call(name, memory.clone(), tuple(start.shape), tuple(tokens.shape), tuple(logits.shape), *rest)
        return FakeEngine.ticket

    def decode_greedy_async_into(self, memory, start, tokens, logits, is_test=False, rows_per_batch=0):
        return self._launch("decode_greedy_async_into", memory, start, tokens, logits, is_test, rows_per_batch)

    def decode_greedy_ragged_into(self, memory, layout, start, tokens, logits, is_test=False):
        return self._launch("decode_greedy_ragged_into", memory, start, tokens, logits, is_test, list(layout))

    def decode_wait(self, host_sync=False):
        self._call("decode_wait", host_sync)

    def ticket_done(self, ticket):
        return True

    def wait_ticket(self, ticket, host_sync=False):
        self._call("wait_ticket", ticket, host_sync)

    def decode_steps(self, ticket):
        return FakeEngine.steps.get(ticket, [self.cfg.max_seq_len + 1])

    def attn_keys(self, T):
        return T - 1

    def attn_map_bytes(self, T, beam_size):
        return (self.cfg.batch_max_length + 1) * int(beam_size) * self.attn_keys(T) * 4

    def decode_beam_batch_ragged(self, packed, lengths, beam_size):
        self._call("decode_beam_batch_ragged", tuple(packed.shape), list(lengths), beam_size)
        return ["ragged"] * len(lengths)

    def decode_attn_beam_batch_ragged(self, packed, lengths, beam_size, return_alpha=False):
        self._call("decode_attn_beam_batch_ragged", tuple(packed.shape), list(lengths), beam_size, return_alpha)
        return ["ragged"] * len(lengths)


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(build_model, "Engine", FakeEngine)
    FakeEngine.log, FakeEngine.ticket, FakeEngine.supports, FakeEngine.fail_once, FakeEngine.steps = [], 0, {}, set(), {}
    return FakeEngine


def _model(name="T2"):
    return Model(synth.make_config(name, max_seq_len=8)).eval()


def _take(fake):
    """The calls since the last look, weight syncs left out."""
    out = [c for c in fake.log if c[0] != "sync_weights"]
    del fake.log[:]
    return out


FIRST = [("set_reserved_blocks", 0), ("set_reserved_cus", 0), ("set_conv_precision", "bf16x3"),
         ("set_conv_kernel", "pipelined16"), ("set_beam_shared_tile", False), ("set_conv_fusion", True, True),
         ("set_decode_chains", 1)]


# ---- settings -------------------------------------------------------------------------------------------------------
def test_first_engine_call_and_the_changes_after_it(fake):
    m = _model()
    m.engine()
    assert fake.log == [("sync_weights", True)] + FIRST
    del fake.log[:]
    m.engine()
    assert fake.log == [("sync_weights", True)]  # nothing changed: the weight sync and no setter
    del fake.log[:]
    m.conv_precision, m.pipelined, m.decode_chains = "mixed", True, 3
    m.engine()
    assert _take(fake) == [("set_reserved_blocks", 64), ("set_decode_chains", 3), ("set_conv_precision", "mixed"),
                           ("set_mixed_units", 3)]
    m.mixed_units, m.conv_kernel = 5, "classic"
    m.engine()
    assert _take(fake) == [("set_conv_kernel", "classic"), ("set_mixed_units", 5)]
    m.reserved_cus, m.reserved_blocks = 8, 16
    m.engine()
    assert _take(fake) == [("set_reserved_blocks", 16), ("set_reserved_cus", 8)]
    m.pipelined = False  # the reserved values are the model's only while pipelined
    m.engine()
    assert _take(fake) == [("set_reserved_blocks", 0), ("set_reserved_cus", 0)]


def test_a_late_precision_change_sends_mixed_units_again(fake):
    m = _model()
    m.conv_precision = "mixed"
    m.engine()
    assert _take(fake) == FIRST[:2] + FIRST[3:] + [("set_conv_precision", "mixed"), ("set_mixed_units", 3)]
    m.conv_precision = "bf16x3"
    m.mixed_units = 4  # only sent under 'mixed'
    m.engine()
    assert _take(fake) == [("set_conv_precision", "bf16x3")]
    m.conv_precision = "mixed"
    m.mixed_units = 3
    m.engine()
    assert _take(fake) == [("set_conv_precision", "mixed"), ("set_mixed_units", 3)]
    m.conv_precision = "fp16x2"  # a late precision too: after the kernel choice
    m.conv_kernel = "classic"
    m.engine()
    assert _take(fake) == [("set_conv_kernel", "classic"), ("set_conv_precision", "fp16x2")]
    m.conv_precision = "fp32"  # an early one: before the kernel choice
    m.conv_kernel = "pipelined16"
    m.engine()
    assert _take(fake) == [("set_conv_precision", "fp32"), ("set_conv_kernel", "pipelined16")]


def test_attn_beam_device_asks_the_engine_only_when_it_has_to(fake):
    m = _model()
    m.engine()
    assert _take(fake) == FIRST  # wanted False, applied False: the engine is not asked
    m.attn_beam_device = True
    m.engine()
    assert _take(fake) == [("supports_device_attn_beam",)]  # asked, answers no: nothing set ...
    m.engine()
    assert _take(fake) == [("supports_device_attn_beam",)]  # ... and asked again by the next call
    fake.supports = {"device_attn_beam": True}
    m.engine(finalize=False)
    assert fake.log == [("sync_weights", False)]  # only a finalized engine can answer: neither asked nor set
    del fake.log[:]
    m.engine()
    assert _take(fake) == [("supports_device_attn_beam",), ("set_attn_beam_device", True)]
    m.engine()
    assert _take(fake) == []
    m.attn_beam_device = False
    m.engine()
    assert _take(fake) == [("supports_device_attn_beam",), ("set_attn_beam_device", False)]


def test_attn_beam_device_has_its_place_in_the_first_call(fake):
    fake.supports = {"device_attn_beam": True}
    m = _model()
    m.attn_beam_device = True
    m.engine()
    assert _take(fake) == FIRST[:5] + [("supports_device_attn_beam",), ("set_attn_beam_device", True)] + FIRST[5:]


def test_fusion_and_shared_tile_switches(fake):
    m = _model()
    m.conv_fusion = (False, True)
    m.beam_shared_tile = True
    m.engine()
    assert _take(fake) == FIRST[:4] + [("set_beam_shared_tile", True), ("set_conv_fusion", False, True), FIRST[6]]
    m.conv_fusion = [False, True]  # a list with the same values is no change
    m.engine()
    assert _take(fake) == []


def test_a_setter_that_raised_is_called_again(fake):
    m = _model()
    fake.fail_once = {"set_conv_kernel"}
    with pytest.raises(RuntimeError, match="set_conv_kernel failed"):
        m.engine()
    assert _take(fake) == FIRST[:4]
    m.engine()
    assert _take(fake) == FIRST[3:]  # what had been applied is not sent again; the kernel and everything after it is


def test_autocast_takes_amp_conv_precision(fake, monkeypatch):
    m = _model()
    monkeypatch.setattr(m, "_under_amp", lambda: True)  # (torch.autocast("cuda") cannot be entered without a device)
    m.engine()
    assert _take(fake) == FIRST[:2] + FIRST[3:] + [("set_conv_precision", "fp16x2")]
    monkeypatch.setattr(m, "_under_amp", lambda: False)
    m.engine()
    assert _take(fake) == [("set_conv_precision", "bf16x3")]


# ---- decode groups --------------------------------------------------------------------------------------------------
def _forward(m, B, T, is_test=False, seed=0):
    mem = torch.randn(B, T, 256, generator=torch.Generator().manual_seed(1000 * B + T + seed))
    p, l, _, extra = m.forward_decoder(mem, torch.zeros(B, 1, dtype=torch.long), is_train=False, is_test=is_test)
    return mem, p, l, extra["decode"]


def _launches(fake):
    out = [c for c in fake.log if c[0] in ("decode_greedy_async_into", "decode_greedy_ragged_into", "decode_wait")]
    del fake.log[:]
    return out


def _shapes(call):
    return (call[0], tuple(call[1].shape)) + call[2:] if torch.is_tensor(call[1]) else call


def test_uniform_then_mixed_groups(fake):
    m = _model()
    m.pipelined, m.decode_group = True, 2
    outs = [_forward(m, 3, 20, seed=i) for i in range(3)]
    calls = _launches(fake)
    assert [_shapes(c) for c in calls] == [("decode_greedy_async_into", (6, 20, 256), (6,), (6, 9), (6, 9, 11), False, 3)]
    assert torch.equal(calls[0][1], torch.cat([o[0] for o in outs[:2]]))
    assert [o[3].ticket for o in outs] == [1, 1, None]
    m.synchronize()
    calls = _launches(fake)
    assert [_shapes(c) for c in calls[:1]] == [("decode_greedy_async_into", (3, 20, 256), (3,), (3, 9), (3, 9, 11), False, 3)]
    assert calls[1:] == [("decode_wait", True)] and torch.equal(calls[0][1], outs[2][0])
    assert [o[3].ticket for o in outs] == [1, 1, 2]
    for k, (_, p, l, _) in enumerate(outs):  # each forward's outputs are the rows of its batch in the launch
        assert tuple(p.shape) == (3, 9) and tuple(l.shape) == (3, 9, 11)
        assert p[:, 0].tolist() == [3 * (k % 2) + r for r in range(3)]

    m.decode_group_mixed, m.decode_group, m.decode_group_rows = True, 3, 8
    sizes = [(3, 20), (2, 45), (4, 7), (9, 5), (1, 5)]
    outs = [_forward(m, B, T, is_test=True) for B, T in sizes]
    m.synchronize(host_sync=False)
    calls = _launches(fake)
    assert [_shapes(c) for c in calls] == [
        ("decode_greedy_ragged_into", (150, 256), (5,), (5, 9), (5, 9, 11), True, [(3, 20), (2, 45)]),
        ("decode_greedy_ragged_into", (28, 256), (4,), (4, 9), (4, 9, 11), True, [(4, 7)]),
        ("decode_greedy_ragged_into", (45, 256), (9,), (9, 9), (9, 9, 11), True, [(9, 5)]),
        ("decode_greedy_ragged_into", (5, 256), (1,), (1, 9), (1, 9, 11), True, [(1, 5)]),
        ("decode_wait", False)]
    assert [o[3].ticket for o in outs] == [3, 3, 4, 5, 6]
    assert torch.equal(calls[0][1], torch.cat([o[0].reshape(-1, 256) for o in outs[:2]]))
    for c, o in zip(calls[1:4], outs[2:]):
        assert torch.equal(c[1], o[0].reshape(-1, 256))
    assert [o[1][:, 0].tolist() for o in outs] == [[0, 1, 2], [3, 4], [0, 1, 2, 3], list(range(9)), [0]]


def test_mixed_group_grows_its_packed_memory(fake):
    """(1, 4) sizes the packed memory at min(8, 3 * 1) * 4 = 12 rows; (2, 45) needs 94 and (1, 200) 294 > 2 * 94: the rows
    collected so far are copied both times."""
    m = _model()
    m.pipelined, m.decode_group_mixed, m.decode_group, m.decode_group_rows = True, True, 3, 8
    outs = [_forward(m, B, T) for B, T in [(1, 4), (2, 45), (1, 200)]]
    calls = _launches(fake)
    assert [_shapes(c) for c in calls] == [
        ("decode_greedy_ragged_into", (294, 256), (4,), (4, 9), (4, 9, 11), False, [(1, 4), (2, 45), (1, 200)])]
    assert torch.equal(calls[0][1], torch.cat([o[0].reshape(-1, 256) for o in outs]))
    assert [o[3].ticket for o in outs] == [1, 1, 1]
    assert [o[1][:, 0].tolist() for o in outs] == [[0], [1, 2], [3]]


def test_a_key_change_launches_the_collected_group(fake):
    m = _model()
    m.pipelined, m.decode_group = True, 3
    _forward(m, 3, 20), _forward(m, 3, 20, seed=1)
    assert _launches(fake) == []
    a = _forward(m, 3, 20, is_test=True)
    assert [_shapes(c)[1:] for c in _launches(fake)] == [((6, 20, 256), (6,), (6, 9), (6, 9, 11), False, 3)]
    b = _forward(m, 3, 21, is_test=True)  # another memory length
    assert [_shapes(c)[1:] for c in _launches(fake)] == [((3, 20, 256), (3,), (3, 9), (3, 9, 11), True, 3)]
    c = _forward(m, 2, 21, is_test=True)  # another row count
    assert [_shapes(c)[1:] for c in _launches(fake)] == [((3, 21, 256), (3,), (3, 9), (3, 9, 11), True, 3)]
    assert [a[3].ticket, b[3].ticket, c[3].ticket] == [2, 3, None]
    m.synchronize(flush=False)  # orders after what has been launched, launches nothing
    assert _launches(fake) == [("decode_wait", True)] and c[3].ticket is None
    m.decode_group_mixed = True  # the mixed collector takes over: the uniform group is launched first
    d = _forward(m, 2, 21, is_test=True)
    assert [_shapes(c)[:2] for c in _launches(fake)] == [("decode_greedy_async_into", (2, 21, 256))]
    e = _forward(m, 2, 21)  # is_test flips under the mixed switch
    assert [_shapes(c)[1:] for c in _launches(fake)] == [((42, 256), (2,), (2, 9), (2, 9, 11), True, [(2, 21)])]
    assert [c[3].ticket, d[3].ticket, e[3].ticket] == [4, 5, None]


def test_without_ragged_support_the_mixed_switch_collects_uniform_groups(fake):
    fake.supports = {"ragged_groups": False}
    m = _model()
    m.pipelined, m.decode_group_mixed, m.decode_group = True, True, 2
    _forward(m, 3, 20), _forward(m, 2, 45), _forward(m, 2, 45, seed=1)
    assert [_shapes(c)[:2] + c[-1:] for c in _launches(fake)] == [("decode_greedy_async_into", (3, 20, 256), 3),
                                                                 ("decode_greedy_async_into", (4, 45, 256), 2)]


def test_a_handle_launches_its_own_group(fake):
    m = _model()
    m.pipelined, m.decode_group = True, 3
    a, b = _forward(m, 3, 20, is_test=True), _forward(m, 3, 20, is_test=True, seed=1)
    assert a[3].done() is False and _launches(fake) == []
    fake.steps = {1: [4, 7], 2: [5]}
    assert b[3].steps() == 7  # launches the two collected batches, picks its own entry
    assert [_shapes(c)[1:] for c in _launches(fake)] == [((6, 20, 256), (6,), (6, 9), (6, 9, 11), True, 3)]
    assert a[3].ticket == b[3].ticket == 1 and a[3].steps() == 4 and a[3].done() is True
    assert [tuple(t.shape) for t in a[3].result()] == [(3, 4), (3, 4, 11)]
    _forward(m, 3, 20, is_test=True, seed=2)  # a new group: the launched one takes no more batches
    c = _forward(m, 3, 20, is_test=True, seed=3)
    c[3].wait(host_sync=True)
    assert c[3].ticket == 2 and c[3].steps() == 5  # ONE entry: that one, though this is the group's second batch
    assert [x[0] for x in fake.log if x[0] != "sync_weights"] == ["decode_greedy_async_into", "wait_ticket"]
    del fake.log[:]
    m.synchronize()
    assert _launches(fake) == [("decode_wait", True)]  # nothing left to launch


# ---- beam routing ---------------------------------------------------------------------------------------------------
def _routed(m, monkeypatch):
    """forward_encoder hands the input through as the memory; the per-tensor search is recorded."""
    each = []
    monkeypatch.setattr(m, "forward_encoder", lambda x: (x, None, None))
    monkeypatch.setattr(m, "beam_search_batch", lambda x, beam, attn: each.append((tuple(x.shape), beam, attn)) or ["each"] * len(x))
    return each


def test_beam_search_over_a_list_is_routed(fake, monkeypatch):
    xs = [torch.zeros(2, 20, 256), torch.zeros(1, 45, 256)]
    m = _model()
    each = _routed(m, monkeypatch)
    assert m._beam_search_mixed([], 3) == [] and fake.log == []
    assert m._beam_search_mixed(xs, 3) == ["ragged"] * 3
    assert _take(fake) == FIRST + [("decode_beam_batch_ragged", (85, 256), [20, 20, 45], 3)] and each == []
    assert m._beam_search_mixed(xs, 3, return_attn=True) == ["each"] * 3  # the TFM head has no maps: per tensor
    assert each == [((2, 20, 256), 3, True), ((1, 45, 256), 3, True)] and _take(fake) == []
    fake.supports = {"ragged_beam": False}
    assert m._beam_search_mixed(xs, 3) == ["each"] * 3 and _take(fake) == []

    fake.supports = {}
    m = _model("TS0")
    each = _routed(m, monkeypatch)
    assert m._beam_search_mixed(xs, 3) == ["ragged"] * 3
    assert _take(fake) == FIRST + [("decode_attn_beam_batch_ragged", (85, 256), [20, 20, 45], 3, False)]
    assert m._beam_search_mixed(xs, 3, return_attn=True) == ["ragged"] * 3
    assert _take(fake) == [("decode_attn_beam_batch_ragged", (85, 256), [20, 20, 45], 3, True)] and each == []
    monkeypatch.setattr(_lib, "ATTN_MAP_BUDGET", 3 * 9 * 3 * 44 * 4 - 1)  # one byte short of three samples at 44 keys
    assert m._beam_search_mixed(xs, 3, return_attn=True) == ["each"] * 3 and _take(fake) == []
    assert m._beam_search_mixed(xs, 3) == ["ragged"] * 3  # the budget is about maps only
    fake.supports = {"ragged_attn_beam": False}
    del fake.log[:]
    assert m._beam_search_mixed(xs, 3) == ["each"] * 3 and _take(fake) == []


def test_an_empty_submitted_beam_search(fake):
    fake.supports = {"device_attn_beam": True}
    m = _model("TS0")
    h = m.beam_search_batch_async([], 3)
    assert h.ticket is None and h.result() == [] and h.steps() == 0 and h.done() is True
    with pytest.raises(NotImplementedError):
        _model().beam_search_batch_async([], 3)  # the TFM head's search cannot be submitted


# ---- results of a beam search -----------------------------------------------------------------------------------------
S = 9
RESULTS = [([], -0.5), ([7], -1.25), (list(range(2, 2 + S)), -3.0)]  # lengths 0, 1 and S


class FakeLib:
    """Stands in for libd2t: each beam entry point fills the caller's arrays with RESULTS (cycled over the samples) and the
    alignment history, where asked for, with its own flat index."""

    def __init__(self):
        self.sizes = None

    @staticmethod
    def _val(x):
        return getattr(x, "_obj", x)  # (C.byref(v) -> v)

    def _fill(self, N, seq, n, score, alpha=None, ld=0):
        self.sizes = (len(seq), None if isinstance(self._val(n), C.c_int32) else len(n))
        for i in range(N):
            toks, sc = RESULTS[i % 3]
            for j, t in enumerate(toks):
                seq[i * S + j] = t
            if isinstance(self._val(n), C.c_int32):
                self._val(n).value, self._val(score).value = len(toks), sc
            else:
                n[i], score[i] = len(toks), sc
        if alpha is not None and alpha.value:
            flat = (C.c_float * (N * S * ld)).from_address(alpha.value)
            flat[:] = [float(k) for k in range(N * S * ld)]
        return 0

    def d2t_decode_beam(self, ctx, mem, T, beam, seq, n, score, stream):
        return self._fill(1, seq, n, score)

    d2t_decode_attn_beam = d2t_decode_beam

    def d2t_decode_beam_batch(self, ctx, mem, N, T, beam, seq, n, score, stream):
        return self._fill(N, seq, n, score)

    d2t_decode_attn_beam_batch = d2t_decode_beam_batch

    def d2t_decode_attn_beam_batch_alpha(self, ctx, mem, N, T, beam, seq, n, score, alpha, stream):
        return self._fill(N, seq, n, score, alpha, T - 1)

    def d2t_decode_beam_batch_ragged(self, ctx, packed, N, Ts, beam, seq, n, score, stream):
        return self._fill(N, seq, n, score)

    def d2t_decode_attn_beam_batch_ragged(self, ctx, packed, N, Ts, beam, seq, n, score, alpha, stream):
        return self._fill(N, seq, n, score, alpha, max(list(Ts)[:max(N, 1)]) - 1)


def _bare_engine(monkeypatch, name):
    eng = object.__new__(Engine)  # no context: only the marshalling around the library call runs
    eng.lib, eng.ctx, eng.device = FakeLib(), None, 0
    eng.cfg = config_from_opt(synth.make_config(name, max_seq_len=S - 1))
    monkeypatch.setattr(_lib, "stream_of", lambda t: None)
    return eng


def _check_results(out, N, tensor_score):
    assert len(out) == N
    for i, r in enumerate(out):
        toks, sc = RESULTS[i % 3]
        assert isinstance(r[0], torch.LongTensor) and tuple(r[0].shape) == (1, len(toks)) and r[0][0].tolist() == toks
        if tensor_score:
            assert torch.is_tensor(r[1]) and r[1].dim() == 0 and r[1].dtype == torch.float32 and float(r[1]) == sc
        else:
            assert type(r[1]) is float and r[1] == sc


def _check_maps(out, Tks, ld):
    hist = torch.arange(len(out) * S * ld, dtype=torch.float32).view(len(out), S, ld)
    for i, (r, Tk) in enumerate(zip(out, Tks)):
        assert len(r) == 3 and torch.equal(r[2], hist[i, :len(RESULTS[i % 3][0]), :Tk])


def test_tfm_beam_results_carry_a_float_score(monkeypatch):
    eng = _bare_engine(monkeypatch, "T2")
    _check_results([eng.decode_beam(torch.zeros(1, 20, 256), 3)], 1, False)
    with pytest.raises(AssertionError, match="signle source"):
        eng.decode_beam(torch.zeros(2, 20, 256), 3)
    _check_results(eng.decode_beam_batch(torch.zeros(4, 20, 256), 3), 4, False)
    assert eng.lib.sizes == (4 * S, 4)
    _check_results(eng.decode_beam_batch_ragged(torch.zeros(20 + 45 + 7, 256), [20, 45, 7], 3), 3, False)
    assert eng.lib.sizes == (3 * S, 3)
    assert eng.decode_beam_batch_ragged(torch.zeros(0, 256), [], 3) == []
    assert eng.lib.sizes == (1, 1)  # an empty list still hands the library valid arrays
    with pytest.raises(ValueError, match="does not hold the 65 rows"):
        eng.decode_beam_batch_ragged(torch.zeros(64, 256), [20, 45], 3)


def test_attn_beam_results_carry_a_tensor_score_and_cut_maps(monkeypatch):
    eng = _bare_engine(monkeypatch, "TS0")
    _check_results([eng.decode_attn_beam(torch.zeros(1, 20, 256), 3)], 1, True)
    _check_results(eng.decode_attn_beam_batch(torch.zeros(4, 20, 256), 3), 4, True)
    out = eng.decode_attn_beam_batch(torch.zeros(4, 20, 256), 3, return_alpha=True)
    _check_results(out, 4, True)
    _check_maps(out, [19] * 4, 19)
    out = eng.decode_attn_beam_batch_ragged(torch.zeros(20 + 45 + 7, 256), [20, 45, 7], 3)
    _check_results(out, 3, True)
    assert all(len(r) == 2 for r in out)
    out = eng.decode_attn_beam_batch_ragged(torch.zeros(20 + 45 + 7, 256), [20, 45, 7], 3, return_alpha=True)
    _check_results(out, 3, True)
    _check_maps(out, [19, 44, 6], 44)  # each map cut to its own sample's keys
    assert eng.decode_attn_beam_batch_ragged(torch.zeros(0, 256), [], 3, return_alpha=True) == []
    assert eng.lib.sizes == (1, 1)
    with pytest.raises(ValueError, match="does not hold the 65 rows"):
        eng.decode_attn_beam_batch_ragged(torch.zeros(66, 256), [20, 45], 3)


def test_a_submitted_search_unpacks_its_downloaded_tensors(fake):
    eng = FakeEngine(synth.make_config("TS0", max_seq_len=S - 1))
    N, lengths, ld = 3, [20, 45, 7], 44
    seq = torch.zeros(N, S, dtype=torch.int64)
    for i, (toks, _) in enumerate(RESULTS):
        seq[i, :len(toks)] = torch.tensor(toks, dtype=torch.int64)
    n = torch.tensor([len(t) for t, _ in RESULTS], dtype=torch.int32)
    score = torch.tensor([s for _, s in RESULTS])
    alpha = torch.arange(N * S * ld, dtype=torch.float32).view(N, S, ld)
    h = BeamSearchHandle(eng, 5, (seq, n, score, alpha), lengths, True)
    out = h.result()
    assert fake.log == [("wait_ticket", 5, True)] and h.result() is out
    _check_results(out, N, True)
    _check_maps(out, [19, 44, 6], ld)
    out = BeamSearchHandle(eng, 6, (seq, n, score), lengths, False).result()
    _check_results(out, N, True)
    assert all(len(r) == 2 for r in out)
