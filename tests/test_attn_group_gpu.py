"""GPU: greedy decode groups of the LSTM-attention heads -- several encoder batches of different row counts and memory
lengths in ONE launch of the step loop (the group builds of attn_decode_kernel behind d2t_op_attn_decode_group,
d2t_decode_attn_greedy_submit_ragged, Model.attn_decode_group).  The invariant at every level: a row's tokens, probs and end
step are those of its own batch's uniform launch, bit for bit, and a batch's rows stop at that batch's own stop step whatever
the other batches of the launch do.

Operator tests in the style of tests/test_recurrent_ops_gpu.py (whose helpers they use): outputs pre-filled with NaN / -1
behind a guard tail; values by that file's measured rule against recurrent_refs.attn_ref, err <= 8 e32 + 1e-6 max |y64|
(DESIGN.md 5.3a), figures printed before they are asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import recurrent_refs as RR
import test_attn_pipelined_gpu as pipe
import test_recurrent_ops_gpu as rops
from conftest import engine_model
from doc2tex_amd import _lib, synth
from doc2tex_amd.engine import ragged_tables

pytestmark = pytest.mark.gpu
DEV = "cuda"
D2T_EINVAL, D2T_ESTATE = 1, 4  # include/d2t.h
H = 256
NAN = float("nan")


# =====================================================================================================================
# 1. the operator
# =====================================================================================================================
# key_off 1: Tk = 18, 1 (one key), 1029 (the 1024-strided key loops go round twice), 4 (below the 11 taps)
OP_BATCHES = ((3, 19), (1, 2), (2, 1030), (4, 5))
OP_S, OP_KEY_OFF = 6, 1
ORDERS = {"as listed": (0, 1, 2, 3), "reversed": (3, 2, 1, 0), "large-small-large": (2, 1, 0, 3, 2)}


@functools.lru_cache(maxsize=None)
def _op_inputs(V, cell, tokgate):
    """weights of the cell and per batch (memory [rows][T][256], its key projection: a float64 product rounded to fp32)"""
    taps = 11 if cell == "coverage" else 1
    W = RR.attn_weights(V, taps, 310 + V + taps, tokgate=tokgate)
    if cell == "bahdanau":  # attention1D.py:71-118: no alignment memory -- no location term, nothing accumulated
        W["wloc"].zero_()
        W["bloc"].zero_()
    out = []
    for i, (rows, T) in enumerate(OP_BATCHES):
        mem = torch.randn(rows, T, H, generator=rops._gen(800 + i))
        out.append((mem, (mem.double() @ W["wk"].double().t() + W["bk"].double()).float()))
    return W, out


@functools.lru_cache(maxsize=None)
def _op_uniform(V, cell, tokgate, init_mode, exit_word):
    """d2t_op_attn_decode on every batch alone (computed once, never written)"""
    W, batches = _op_inputs(V, cell, tokgate)
    out = []
    for mem, kp in batches:
        rc, got = rops._decode(W, mem, kp, OP_S, key_off=OP_KEY_OFF, init_mode=init_mode, coverage=cell == "coverage",
                               exit_word=exit_word)
        assert rc == 0
        out.append(got)
    return out


class _Raw:
    """a device output that starts 4 bytes past a 16-byte boundary, filled with garbage, with a guard tail behind it"""

    def __init__(self, words, fill):
        self.words = words
        self.t = torch.full((words + 1 + rops.GUARD,), fill, dtype=torch.int32, device=DEV)
        self.fill = fill
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + 4

    def untouched(self):
        return bool((self.t.cpu() == self.fill).all())

    def get(self, dtype, shape):
        c = self.t.cpu()
        assert bool((c[1 + self.words:] == self.fill).all()) and int(c[0]) == self.fill, "a kernel wrote outside its output"
        return c[1:1 + self.words].clone().view(dtype).view(*shape)


def _group(W, batches, S, *, init_mode=0, coverage=True, exit_word=False, key_off=OP_KEY_OFF, end_token=1, misalign=False,
           tables=None, n_batches=None, steps=True, over=None):
    """one d2t_op_attn_decode_group call over `batches` = [(mem [rows][T][256], kp)]; returns rc and the outputs (CPU; the
    buffers themselves after a refusal).  misalign: tokens and probs start 4 bytes past a 16-byte boundary, full of garbage."""
    lib = _lib.require_device()
    layout = [(int(m.shape[0]), int(m.shape[1])) for m, _ in batches]
    tab = dict(ragged_tables(layout))
    tab.update(tables or {})
    B, V, taps, nb = len(tab["row0"]), W["wg_t"].shape[1], W["wloc"].shape[1], len(layout) if n_batches is None else n_batches
    keep = [rops._d(torch.cat([m.reshape(-1, H) for m, _ in batches])), rops._d(torch.cat([k.reshape(-1, H) for _, k in batches]))]
    a = _lib.D2TOpAttnDecodeArgs()
    a.mem, a.kp = keep[0].data_ptr(), keep[1].data_ptr()
    for k in rops._W_KEYS:
        if k in W:
            keep.append(rops._d(W[k]))
            setattr(a, k, keep[-1].data_ptr())
    if misalign:
        o = dict(probs=_Raw(B * S * V, 0x7FC00000), tokens=_Raw(2 * B * S, 0x7F7F7F7F))
    else:
        o = dict(probs=rops.Buf(B, S, V), tokens=rops.Buf(B, S, dtype=torch.int64))
    o["end_step"] = rops.Buf(B, dtype=torch.int32, fill=-7)
    if exit_word:
        o["exit_state"] = rops.Buf(max(nb, 1), dtype=torch.int64, fill=-1)
    for k, b in o.items():
        setattr(a, k, b.ptr)
    o["steps_dev"] = rops.Buf(max(nb, 1), dtype=torch.int32)
    a.bscore, a.out_dropscale = float(W["bscore"]), 1.0
    a.B, a.T, a.S, a.V, a.taps, a.key_off, a.init_mode = B, max(T for _, T in layout), S, V, taps, key_off, init_mode
    a.coverage, a.end_token, a.samples = int(coverage), end_token, B
    for k, v in (over or {}).items():
        setattr(a, k, v)
    dt = [rops._d(torch.as_tensor([int(v) for v in tab[k]], dtype=torch.int32)) for k in ("row0", "len", "row_batch", "batch_rows")]
    rc = lib.d2t_op_attn_decode_group(C.byref(a), *[t.data_ptr() for t in dt], nb, o["steps_dev"].ptr if steps else None, rops._stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, o
    got = {k: b.get() for k, b in o.items() if not isinstance(b, _Raw)}
    if misalign:
        got["probs"], got["tokens"] = o["probs"].get(torch.float32, (B, S, V)), o["tokens"].get(torch.int64, (B, S))
    return rc, got


def _rows_of(layout):
    """first output row of every batch of a layout"""
    return np.concatenate([[0], np.cumsum([r for r, _ in layout])]).tolist()


@pytest.mark.parametrize("tokgate", (False, True), ids=("embedded", "onehot"))
@pytest.mark.parametrize("cell", ("coverage", "bahdanau"))
@pytest.mark.parametrize("V", (37, 1025))  # the narrow and the wide build
def test_group_rows_equal_their_batch_alone(V, cell, tokgate):
    """init_mode 0, 1, 2, with and without exit words, the batches as listed, reversed and large-small-large (a batch twice in
    one launch): tokens, probs and end_step of every row are the bits of d2t_op_attn_decode on its batch alone"""
    W, batches = _op_inputs(V, cell, tokgate)
    for init_mode in (0, 1, 2):
        for exit_word in (False, True):
            uni = _op_uniform(V, cell, tokgate, init_mode, exit_word)
            for what, order in ORDERS.items():
                rc, got = _group(W, [batches[i] for i in order], OP_S, init_mode=init_mode, coverage=cell == "coverage",
                                 exit_word=exit_word)
                assert rc == 0, (what, init_mode, exit_word)
                r0 = _rows_of([OP_BATCHES[i] for i in order])
                for k, i in enumerate(order):
                    info = f"{what}, init {init_mode}, exit {exit_word}: batch {k} (rows, T) = {OP_BATCHES[i]}"
                    for name in ("tokens", "probs", "end_step"):
                        assert rops._same(got[name][r0[k]:r0[k + 1]], uni[i][name]), f"{info}: {name} differs from the batch alone"
                    want = int(uni[i]["steps_dev"][0]) if exit_word else OP_S
                    assert int(got["steps_dev"][k]) == want, (info, got["steps_dev"].tolist())


@pytest.mark.parametrize("V,cell,init_mode", [(37, "coverage", 1), (1025, "coverage", 2)])
def test_group_against_float64(V, cell, init_mode):
    """one group by the measured rule against recurrent_refs.attn_ref on every batch, greedy tokens exact under the margin
    condition (top-1 - top-2 >= 100 * 8 e32 at every (row, step), asserted on the reference first)"""
    W, batches = _op_inputs(V, cell, False)
    rc, got = _group(W, list(batches), OP_S, init_mode=init_mode, coverage=True)
    assert rc == 0
    r0 = _rows_of(OP_BATCHES)
    for k, (mem, kp) in enumerate(batches):
        y64, e32 = rops._ref_e32(W, mem, kp, OP_S, key_off=OP_KEY_OFF, init_mode=init_mode, coverage=True)
        rops._margin_ok(f"attn_group_b{k}", y64, e32)
        mine = slice(r0[k], r0[k + 1])
        assert torch.equal(got["tokens"][mine], y64["tokens"]) and torch.equal(got["end_step"][mine], y64["end_step"])
        rops._rule("attn_group_probs", got["probs"][mine], y64["probs"], e32["probs"], batch=k, T=OP_BATCHES[k][1], V=V, init=init_mode)


def test_group_op_refusals():
    """tables that would index out of range or do not describe batches, fields the group build does not take, the limits:
    D2T_EINVAL and nothing written"""
    W, batches = _op_inputs(37, "coverage", False)
    ok = ragged_tables(list(OP_BATCHES))
    assert ok["mem_rows"] == 3 * 19 + 2 + 2 * 1030 + 4 * 5

    def tab(key, idx, value):
        v = list(ok[key])
        v[idx] = value
        return {key: v}
    dummy = torch.zeros(64, device=DEV)
    cases = [dict(tables=tab("len", 3, 1)), dict(tables=tab("len", 3, 0)), dict(tables=tab("len", 0, 4098)),  # Tk = 0, -1, 4097
             dict(tables=tab("len", 4, 1031)),  # the largest length is not args->T
             dict(tables=tab("row0", 0, -1)), dict(tables=tab("row0", 9, ok["mem_rows"] - 4)),  # a slice outside the packed rows
             dict(tables=tab("row_batch", 0, 1)), dict(tables=tab("row_batch", 5, 3)), dict(tables=tab("row_batch", 9, 4)),
             dict(tables=tab("row_batch", 4, 1)),  # a row counted into its neighbour's batch
             dict(tables=tab("batch_rows", 0, 2)), dict(tables=tab("batch_rows", 3, 5)),
             dict(n_batches=0), dict(n_batches=3), dict(n_batches=65), dict(steps=False),
             dict(over=dict(T=1031)), dict(over=dict(V=16385)), dict(over=dict(step_mode=1)), dict(over=dict(S=0)),
             dict(over=dict(sv_alpha=dummy.data_ptr())), dict(over=dict(teacher=dummy.data_ptr())),
             dict(over=dict(steps_dev=dummy.data_ptr())), dict(over=dict(samples=3))]
    for c in cases:
        rc, o = _group(W, list(batches), OP_S, exit_word=True, **c)
        assert rc == D2T_EINVAL, (c, rc)
        assert all(b.untouched() for b in o.values()), c
    big = [(torch.zeros(1025, 2, H), torch.zeros(1025, 2, H))]  # more than 1024 rows
    rc, o = _group(W, big, OP_S)
    assert rc == D2T_EINVAL and all(b.untouched() for b in o.values())
    assert bool((dummy == 0).all())


# =====================================================================================================================
# 2. the exit, per batch
# =====================================================================================================================
EXIT_S, EXIT_V, EXIT_TAPS = 8, 5, 3


@functools.lru_cache(maxsize=None)
def _exit_batches():
    """Three batches chosen ON THE FLOAT64 REFERENCE from pools of candidate rows (T = 9 and T = 6, key_off 1): every row of
    batch A ends by step 2 and one at step 2, every row of B by step 4 and one at step 4, one row of C never ends -- each
    chosen row with the margin condition at every step.  Returns W, [(mem, kp)] x 3, the end token, the rows' end steps."""
    for seed in range(60, 80):
        W = RR.attn_weights(EXIT_V, EXIT_TAPS, seed)
        pools = []
        for T in (9, 6):
            mem = torch.randn(48, T, H, generator=rops._gen(seed * 10 + T))
            kp = (mem.double() @ W["wk"].double().t() + W["bk"].double()).float()
            y64, e32 = rops._ref_e32(W, mem, kp, EXIT_S, key_off=1, init_mode=2, coverage=True)
            top = y64["probs"].topk(2, -1).values
            good = (top[..., 0] - top[..., 1]).min(1).values >= 800.0 * e32["probs"]
            pools.append((mem, kp, y64["tokens"], good))
        for end in range(EXIT_V):
            first = []
            for mem, kp, toks, good in pools:
                f = torch.where((toks == end).any(1), (toks == end).float().argmax(1), torch.full((48,), -1))
                first.append([int(v) if bool(g) else None for v, g in zip(f, good)])

            def pick(pool, at, below, n):
                exact = [r for r, v in enumerate(first[pool]) if v == at]
                rest = [r for r, v in enumerate(first[pool]) if v is not None and 0 <= v < below and v != at]
                return (exact[:1] + rest[:n - 1]) if exact and len(rest) >= n - 1 else None
            never = [r for r, v in enumerate(first[0]) if v == -1]
            ended = [r for r, v in enumerate(first[0]) if v is not None and v >= 0]
            a, b = pick(0, 2, 3, 3), pick(1, 4, 5, 2)
            if a and b and never and len(ended) >= 3:
                c = ended[:2] + never[:1] + ended[2:3]
                sel = [(0, a), (1, b), (0, c)]
                return (W, [(pools[p][0][r].contiguous(), pools[p][1][r].contiguous()) for p, r in sel], end,
                        [[first[p][i] for i in r] for p, r in sel])
    raise AssertionError("no seed meets the condition: extend the seed range")


def test_every_batch_stops_at_its_own_step():
    """one launch: a batch that ends at step 2, one that ends at step 4, one with a row that never ends"""
    W, batches, end, first = _exit_batches()
    S = EXIT_S
    print("FIG attn_group_exit end token", end, "end steps", first)
    assert max(first[0]) == 2 and max(first[1]) == 4 and min(first[2]) == -1 and min(first[0] + first[1]) >= 0
    kw = dict(init_mode=2, coverage=True, end_token=end)
    full = [rops._decode(W, m, k, S, key_off=1, **kw)[1] for m, k in batches]  # every step of every batch alone
    rc, got = _group(W, batches, S, exit_word=True, **kw)
    assert rc == 0
    assert got["steps_dev"].tolist() == [3, 5, S]
    assert got["end_step"].tolist() == first[0] + first[1] + first[2]
    r0 = _rows_of([(m.shape[0], 0) for m, _ in batches])
    for k, steps in enumerate((3, 5, S)):
        mine = slice(r0[k], r0[k + 1])
        for name in ("tokens", "probs"):
            assert rops._same(got[name][mine, :steps], full[k][name][:, :steps]), (k, name)
            assert bool((rops._bits(got[name][mine, steps:]) == 0).all()), f"batch {k}: {name} not cleared behind its exit"
    assert bool((got["probs"][r0[2]:, -1] != 0).all())  # the third batch is untouched: its last step is there
    # garbage-filled buffers that start 4 bytes past a 16-byte boundary: the same result
    rc, odd = _group(W, batches, S, exit_word=True, misalign=True, **kw)
    assert rc == 0
    for name in ("tokens", "probs", "end_step", "steps_dev"):
        assert rops._same(odd[name], got[name]), name
    # without exit words: every step of every row, every entry S
    rc, plain = _group(W, batches, S, **kw)
    assert rc == 0 and plain["steps_dev"].tolist() == [S, S, S]
    for k in range(3):
        assert rops._same(plain["probs"][r0[k]:r0[k + 1]], full[k]["probs"]) and rops._same(plain["tokens"][r0[k]:r0[k + 1]], full[k]["tokens"])


def test_more_rows_than_compute_units():
    """600 rows in 64 batches: blocks that start late neither hold the early ones up nor change a result, and every batch
    still stops at its own step"""
    W, batches, end, first = _exit_batches()
    S = EXIT_S
    kw = dict(init_mode=2, coverage=True, end_token=end)
    rc, small = _group(W, batches, S, exit_word=True, **kw)
    assert rc == 0
    r0 = _rows_of([(m.shape[0], 0) for m, _ in batches])
    counts = [9, 10, 9] * 21 + [12]
    assert len(counts) == 64 and sum(counts) == 600
    many, idx = [], []
    for k, n in enumerate(counts):
        m, kp = batches[k % 3]
        rows = [r % m.shape[0] for r in range(n)]
        many.append((m[rows].contiguous(), kp[rows].contiguous()))
        idx += [r0[k % 3] + r for r in rows]
    rc, big = _group(W, many, S, exit_word=True, **kw)
    assert rc == 0
    assert big["steps_dev"].tolist() == [(3, 5, S)[k % 3] for k in range(64)]
    for name in ("tokens", "probs", "end_step"):
        assert rops._same(big[name], small[name][idx]), name


# =====================================================================================================================
# 3. the model
# =====================================================================================================================
SIZES = [3, 2, 4, 1, 3, 2]
VIT_CROPS = [(48, 64, 0.25), (32, 64, 1.0), None, (32, 32, 1.0), (48, 32, 1.0), (48, 64, 0.6)]  # None: synth.staggered_images
C0_WIDTHS = [320, 160, 96, 320, 160, 96]
# config, batch_max_length, end_bias, the reference fixture whose batch rides in position 2, whether the is_test step counts
# must differ with one batch at the limit.  Chosen on the CPU oracle (oracle.restatement, is_test):
#   TS0 at the fixture's 0.18: step counts [7, 41, 15, 41, 18, 7] of 41 -- the 32-high crops never emit [s], the 48 x 64 crops
#       scaled by 0.25 / 0.6 end at step 6 with a top-2 gap of 0.012, the fixture's batch at 14;
#   TO0 at the fixture's 0.6: [6, 1, 7, 1, 6, 6];  TB0 at 0.3: [13, 13, 13, 1, 1, 13];  C0 at 0.18: every batch 1 of 21.
MODEL_STACKS = [("TS0", 40, 0.18, "attn_serve_ts0_stagger", True), ("TO0", 40, 0.6, "attn_serve_to0_stagger", False),
                ("TB0", 12, 0.3, None, False), ("TA0", 12, 0.3, None, False), ("C0", 20, 0.18, None, False)]


def _images(cname, seed=5100):
    if cname == "C0":
        return [synth.synth_images(b, 32, w, seed=seed + 100 + i).cuda() for i, (b, w) in enumerate(zip(SIZES, C0_WIDTHS))]
    return [(synth.staggered_images(seed=1300) if c is None else synth.synth_images(b, c[0], c[1], seed=seed + i) * c[2]).cuda()
            for i, (b, c) in enumerate(zip(SIZES, VIT_CROPS))]


def _tickets(m):
    eng = m._engine  # (the context of the model's last forward)
    return int(eng.lib.d2t_decode_last_ticket(eng.ctx))


def _check(out, ref, steps, what):
    p, l, a, h = out
    h.wait(host_sync=True)
    assert h.done(), what
    assert torch.equal(p, ref[0]) and torch.equal(l, ref[1]), what
    assert h.steps() == steps, (what, h.steps(), steps)
    rp, rl = h.result()
    assert rp is p and rl is l, what  # full size, as the synchronous forward of these heads returns them


@pytest.mark.parametrize("cname,L,eb,fixture,mixed", MODEL_STACKS)
def test_grouped_forwards_equal_the_synchronous_ones(cname, L, eb, fixture, mixed):
    _, m = engine_model(cname, L, 1234, eb)
    imgs = _images(cname)
    assert len({tuple(x.shape[2:]) for x in imgs}) >= 3
    assert m.engine().supports_ragged_attn_greedy() and not m.engine().supports_ragged_groups()
    refs, steps = {}, {}
    for is_test in (False, True):
        refs[is_test] = pipe._sync_ref(m, imgs, L, is_test)
        steps[is_test] = [pipe._ref_steps(r[0], is_test) for r in refs[is_test]]
    print(f"FIG attn_group_model {cname}: is_test step counts {steps[True]} of {L + 1}")
    if mixed:  # the condition: batches of one launch stop at different steps, and one runs to the limit
        assert len(set(steps[True])) > 2 and max(steps[True]) == L + 1 and min(steps[True]) < L + 1, steps[True]
        for G in (2, 3):
            assert any(len(set(steps[True][i:i + G])) > 1 and max(steps[True][i:i + G]) == L + 1 for i in range(0, 6, G))
    if fixture:  # the reference's own batch inside a group whose other batches stop elsewhere
        c, z = pipe.SERVE[fixture], pipe._load(fixture)
        assert (c["config"], c["max_seq_len"], c["end_bias"], c["B"]) == (cname, L, eb, SIZES[2])
        assert steps[True][2] == c["steps"] and any(s != c["steps"] for s in steps[True][:2])
    for is_test in (False, True):
        ref, want = refs[is_test], steps[is_test]
        for G in (2, 3, 6):
            for chains in (1, 3):
                m.pipelined, m.decode_chains, m.attn_decode_group = True, chains, G
                t0 = _tickets(m)
                outs = []
                for x in imgs:  # six forwards in flight before the first wait
                    p, l, a, add = pipe._forward(m, x, L, is_test)
                    assert sorted(add) == ["decode"] and tuple(p.shape) == (x.shape[0], L + 1) and a is None
                    outs.append((p, l, a, add["decode"]))
                assert _tickets(m) - t0 == 6 // G  # one launch per G forwards
                for i in (4, 1, 5, 0, 3, 2):  # consumed out of order
                    _check(outs[i], ref[i], want[i], (cname, is_test, G, chains, i))
                if fixture and is_test:
                    assert np.array_equal(outs[2][0].cpu().numpy(), z["tokens"])
                    err = float(np.abs(outs[2][1].cpu().numpy() - z["probs"]).max())
                    print(f"FIG attn_group_fixture {fixture} G={G} chains={chains}: max |dprob| = {err:.2e}")
                    assert err <= pipe.LOGIT_TOL
                m.synchronize()
    # a row budget that splits the list: 3 + 2 | 4 + 1 | 3 + 2 rows, the last group launched by synchronize()
    ref, want = refs[True], steps[True]
    m.pipelined, m.decode_chains, m.attn_decode_group, m.attn_decode_group_rows = True, 3, 6, 6
    t0 = _tickets(m)
    outs = [pipe._forward(m, x, L, True) for x in imgs]
    assert _tickets(m) - t0 == 2 and outs[5][3]["decode"].ticket is None
    m.synchronize()
    assert _tickets(m) - t0 == 3
    for i in range(6):
        _check(outs[i][:3] + (outs[i][3]["decode"],), ref[i], want[i], (cname, "budget", i))
    m.attn_decode_group_rows = 256
    # a group of one batch, launched by its handle
    t0 = _tickets(m)
    out = pipe._forward(m, imgs[0], L, True)
    assert _tickets(m) == t0
    _check(out[:3] + (out[3]["decode"],), ref[0], want[0], (cname, "one batch"))
    assert _tickets(m) == t0 + 1
    # a viz_attn forward in the middle: what has been collected is launched first, then it runs alone with its maps
    pred = m.predicter.Prediction
    pred.viz_attn = True
    (vp, vl, va), = pipe._sync_ref(m, imgs[2:3], L, True)
    pred.viz_attn = False
    m.pipelined = True
    t0 = _tickets(m)
    outs = [pipe._forward(m, x, L, True) for x in imgs[:2]]
    pred.viz_attn = True
    p, l, a, add = pipe._forward(m, imgs[2], L, True)
    pred.viz_attn = False
    assert a is not None and [o[3]["decode"].ticket for o in outs] == [t0 + 1] * 2 and add["decode"].ticket == t0 + 2
    outs += [(p, l, a, add)] + [pipe._forward(m, x, L, True) for x in imgs[3:]]
    add["decode"].wait(host_sync=True)
    assert torch.equal(a, va) and torch.equal(p, vp) and torch.equal(l, vl)
    for i in (0, 1):  # the forwards before it complete without another launch
        _check(outs[i][:3] + (outs[i][3]["decode"],), ref[i], want[i], (cname, "before viz", i))
    assert _tickets(m) == t0 + 2
    m.synchronize()
    assert _tickets(m) == t0 + 3
    for i in range(6):
        _check(outs[i][:3] + (outs[i][3]["decode"],), ref[i], want[i], (cname, "viz", i))
    m.pipelined, m.attn_decode_group = False, 1


# =====================================================================================================================
# 4. refusals
# =====================================================================================================================
def _raw(eng, packed, rows, Ts, is_test=1, n=None, tokens=None, probs=None):
    S, V = eng.cfg.batch_max_length + 1, eng.cfg.vocab
    B = max(1, min(sum(r for r in rows if r > 0), 1100))
    tok = torch.full((B, S), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device=DEV) if tokens is None else tokens
    pr = torch.full((B, S, V), NAN, device=DEV) if probs is None else probs
    k = max(len(rows), 1)
    t = C.c_int64(-1)
    rc = eng.lib.d2t_decode_attn_greedy_submit_ragged(eng.ctx, _lib.ptr(packed), len(rows) if n is None else n, (C.c_int32 * k)(*rows),
                                                      (C.c_int32 * k)(*Ts), is_test, _lib.ptr(tok), _lib.ptr(pr),
                                                      _lib.stream_of(packed), C.byref(t))
    torch.cuda.synchronize()
    clean = bool((tok == 0x7F7F7F7F7F7F7F7F).all()) and bool(torch.isnan(pr).all())
    return rc, eng.lib.d2t_last_error(eng.ctx).decode(), clean, int(t.value)


def test_refusals_leave_the_context_usable():
    """Two refusals of the entry are not reached here: a pointer of another device needs a second GPU (the leg below runs
    only where there is one), and a vocabulary over the cap cannot be brought to this entry at all, because creating such a
    context is refused already (tests/test_attn_vocab_gpu.py); the cap itself is exercised on the operator entry
    (test_group_op_refusals, V = 16385)."""
    _, m = engine_model("TS0", 14, 1234, 0.3)
    eng = m.engine()
    assert eng.cfg.attn_keys == _lib.ATTN_KEYS_NOCLS_INIT_CLS  # Attnv2 behind a ViT: T = Tk + 1
    packed = torch.randn(4200, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    tok, probs, ticket = eng.decode_attn_greedy_async(packed[:40].reshape(2, 20, H), False)
    eng.wait_ticket(ticket, host_sync=True)
    for rows, Ts, n, code, words in [
        ([], [], 0, D2T_EINVAL, "1 to 64 batches"),
        ([2], [8], -1, D2T_EINVAL, "1 to 64 batches"),
        ([1] * 65, [8] * 65, None, D2T_EINVAL, "1 to 64 batches"),
        ([2, 0], [8, 8], None, D2T_EINVAL, "batch 1 of the group has 0 rows"),
        ([2, -3], [8, 8], None, D2T_EINVAL, "has -3 rows"),
        ([1000, 25], [2, 2], None, D2T_EINVAL, "at most 1024 rows"),
        ([2, 2], [8, 1], None, D2T_EINVAL, "memory length 1"),  # Tk = 0
        ([2, 2], [8, 0], None, D2T_EINVAL, "memory length 0"),
        ([2, 1], [8, 4098], None, D2T_EINVAL, "memory length 4098"),  # Tk = 4097
    ]:
        rc, msg, clean, t = _raw(eng, packed, rows, Ts, n=n)
        assert rc == code and words in msg and clean and t == -1, (rows[:3], Ts[:3], rc, msg, clean, t)
    if torch.cuda.device_count() > 1:  # (a second GPU is the only way to own a pointer of another device)
        rc, msg, clean, t = _raw(eng, torch.zeros(64, H, device="cuda:1"), [2], [8])
        assert rc == D2T_EINVAL and "device" in msg and t == -1, (rc, msg)
    assert int(eng.lib.d2t_decode_last_ticket(eng.ctx)) == int(ticket)  # nothing was enqueued
    # the TFM head's entry keeps refusing this context
    assert not eng.supports_ragged_groups()
    start = torch.zeros(4, dtype=torch.int64, device=DEV)
    tk = torch.zeros(4, 15, dtype=torch.int64, device=DEV)
    lg = torch.zeros(4, 15, eng.cfg.vocab, device=DEV)
    rc = eng.lib.d2t_decode_greedy_submit_ragged(eng.ctx, _lib.ptr(packed), 2, (C.c_int32 * 2)(2, 2), (C.c_int32 * 2)(8, 9),
                                                 _lib.ptr(start), 1, _lib.ptr(tk), _lib.ptr(lg), _lib.stream_of(packed), None)
    assert rc == D2T_ESTATE and int(eng.lib.d2t_decode_last_ticket(eng.ctx)) == int(ticket)
    # ... and the context still decodes groups, correctly
    mems = [torch.randn(b, T, H, generator=torch.Generator().manual_seed(40 + T)).to(DEV) for b, T in ((2, 9), (3, 30), (1, 4))]
    S, V = eng.cfg.batch_max_length + 1, eng.cfg.vocab
    for is_test in (True, False):
        want = [eng.decode_attn_greedy(x, is_test) for x in mems]
        tok, probs = torch.empty(6, S, dtype=torch.int64, device=DEV), torch.empty(6, S, V, device=DEV)
        t = eng.decode_attn_greedy_ragged_into(torch.cat([x.reshape(-1, H) for x in mems]), [(2, 9), (3, 30), (1, 4)], tok, probs, is_test)
        eng.wait_ticket(t, host_sync=True)
        assert torch.equal(tok, torch.cat([w[0] for w in want])) and torch.equal(probs, torch.cat([w[1] for w in want]))
        got = eng.decode_steps(t)
        assert got == ([pipe._ref_steps(w[0], True) for w in want] if is_test else [S]), got
    with pytest.raises(ValueError, match="packed memory must be"):
        eng.decode_attn_greedy_ragged_into(packed[:10], [(2, 9)], tok[:2], probs[:2])


def test_a_tfm_context_refuses_the_attn_groups():
    _, mt = engine_model("T2", 12, 1234, 1.8)
    eng = mt.engine()
    assert not eng.supports_ragged_attn_greedy()
    rc, msg, clean, t = _raw(eng, torch.zeros(64, H, device=DEV), [2, 2], [8, 9])
    assert rc == D2T_ESTATE and "Attn decoder" in msg and clean and t == -1, (rc, msg)
    assert int(eng.lib.d2t_decode_last_ticket(eng.ctx)) == 0
