"""GPU: ragged decode groups -- encoder batches of DIFFERENT row counts and memory lengths decoded by one captured step
loop (d2t_decode_greedy_submit_ragged, Model.decode_group_mixed).  The invariant of decode groups carries over: every row
is bit-identical to the synchronous single-batch decode of its batch, because a row of the ragged kernels reads its own
slice of the packed memory rows and its arithmetic depends on its own length alone.

The cross-attention's fp32-MFMA form inside the step loop (`cross_fp32`) is selected by a probe build only; here it is
covered at the operator level (kinds 1 / 2 of d2t_op_decoder_row_ragged), the shipped split-bf16 form at both levels."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import test_decode_ops_gpu as ops
from conftest import GOLD, engine_model
from doc2tex_amd import _lib, synth
from oracle import restatement as R
from test_parity_gpu import LOGIT_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
D2T_EINVAL, D2T_ESTATE = 1, 4  # include/d2t.h


def _go(B):
    return torch.full((B, 1), R.GO, dtype=torch.long, device=DEV)


def _mixed(m, group, rows=384, chains=2):
    m.pipelined, m.decode_chains, m.decode_group, m.decode_group_mixed, m.decode_group_rows = True, chains, group, True, rows


def _plain(m):
    m.pipelined, m.decode_group, m.decode_group_mixed = False, 1, False


def _case(cases, name):
    return next(c for c in cases["greedy"] if c["case"] == name)


def _sync_refs(m, imgs, is_test):
    with torch.no_grad():
        return [tuple(t.clone() for t in m(x, _go(x.shape[0]), is_train=False, is_test=is_test)[:2]) for x in imgs]


# ---------------------------------------------------------------------------------------------------------------------
# 1. reference fixtures
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_fixtures_decoded_as_one_ragged_group(cases):
    c128, c96 = _case(cases, "c4_greedy_128"), _case(cases, "c4_greedy_96")
    for c in (c128, c96):
        assert (c["config"], c["wseed"], c["max_seq_len"], c["end_bias"], c["is_test"]) == ("C4", 1234, 20, 0.0, False)
    assert (c128["B"], c128["H"], c128["W"]) == (1, 128, 512) and (c96["B"], c96["H"], c96["W"]) == (2, 96, 384)
    cfg, m = engine_model("C4", 20, 1234, 0.0, beam_size=c128["beam_size"])
    imgs = [synth.synth_images(1, 128, 512, seed=c128["iseed"]).cuda(), synth.synth_images(2, 96, 384, seed=c96["iseed"]).cuda(),
            synth.synth_images(2, 160, 640, seed=1075).cuda()]
    ref160 = _sync_refs(m, imgs[2:], False)[0]
    with torch.no_grad():
        _mixed(m, 3)
        outs = [m(x, _go(x.shape[0]), is_train=False) for x in imgs]
        assert len({o[2]["decode"].ticket for o in outs}) == 1 and outs[0][2]["decode"].ticket is not None  # ONE decode
        res = [o[2]["decode"].result() for o in outs]
        m.synchronize()
    for c, (p, l) in zip((c128, c96), res):
        z = np.load(os.path.join(GOLD, c["case"] + ".npz"))
        assert p.shape[1] == c["steps"]
        assert np.array_equal(p.cpu().numpy(), z["tokens"]), f"{c['case']}: token ids differ from the reference"
        dl = float(np.abs(l.cpu()[:, z["logit_steps"].tolist()].numpy() - z["logits_sample"]).max())
        print(f"FIG ragged_fixture {c['case']} max|dlogit|={dl:.3e}")
        assert dl <= LOGIT_TOL, f"{c['case']}: logits differ by {dl}"
    assert torch.equal(res[2][0], ref160[0]) and torch.equal(res[2][1], ref160[1])
    _plain(m)


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit identity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_test", [False, True])
@pytest.mark.parametrize("cfg_name,batches", [
    # (rows, H, W): at least three sizes, unequal row counts, an ODD row total (the two-row kernel pairs rows of different batches)
    ("T2", [(3, 48, 64), (2, 48, 32), (1, 48, 48), (1, 48, 16), (2, 32, 64)]),
    ("C2", [(2, 128, 512), (3, 96, 384), (1, 64, 256), (1, 128, 256)]),
])
def test_every_row_equals_its_single_batch_decode_at_full_length(cfg_name, batches, is_test):
    cfg, m = engine_model(cfg_name, 150, 1234, 1.81 if is_test else 0.0)
    imgs = [synth.synth_images(B, H, W, seed=2100 + i).cuda() for i, (B, H, W) in enumerate(batches)]
    assert sum(b[0] for b in batches) % 2 == 1
    eng = m.engine()
    Ts = [eng.encoder_shape(H, W)[0] for _, H, W in batches]
    assert len(set(Ts)) >= 3, Ts
    ref = _sync_refs(m, imgs, is_test)
    with torch.no_grad():
        _mixed(m, len(imgs))
        outs = [m(x, _go(x.shape[0]), is_train=False, is_test=is_test) for x in imgs]
        assert len({o[2]["decode"].ticket for o in outs}) == 1
        for o, (rp, rl) in zip(outs, ref):
            p, l = o[2]["decode"].result()
            assert p.shape == rp.shape and l.shape == rl.shape, (p.shape, rp.shape)
            assert torch.equal(p, rp), "tokens differ from the single-batch decode"
            assert torch.equal(l, rl), "logits are not bit-identical to the single-batch decode"
        m.synchronize()
    if not is_test:
        assert all(rp.shape[1] == 151 for rp, _ in ref)
    _plain(m)


def _synthetic_group(eng, layout, seed):
    g = torch.Generator().manual_seed(seed)
    mems = [torch.randn(B, T, 256, generator=g).to(DEV) for B, T in layout]
    return mems, torch.cat([x.reshape(-1, 256) for x in mems]).contiguous()


def _submit(eng, packed, layout, is_test):
    """ragged decode into poisoned buffers -> (tokens, logits, per-batch steps), complete"""
    S, V = eng.cfg.max_seq_len + 1, eng.cfg.vocab
    rows = sum(b for b, _ in layout)
    tokens = torch.full((rows, S), -7, dtype=torch.int64, device=DEV)
    logits = torch.full((rows, S, V), float("nan"), device=DEV)
    start = torch.full((rows,), R.GO, dtype=torch.int64, device=DEV)
    ticket = eng.decode_greedy_ragged_into(packed, layout, start, tokens, logits, is_test=is_test)
    steps = eng.decode_steps(ticket)
    eng.wait_ticket(ticket, host_sync=True)
    return tokens, logits, steps


def _check_against_single(eng, mems, layout, tokens, logits, steps, is_test):
    S = eng.cfg.max_seq_len + 1
    r0 = 0
    for k, ((B, T), mem) in enumerate(zip(layout, mems)):
        rp, rl = eng.decode_greedy(mem, torch.full((B,), R.GO, dtype=torch.int64, device=DEV), is_test)
        n = steps[k] if is_test else S
        assert n == rp.shape[1], f"batch {k}: {n} steps, its single-batch decode took {rp.shape[1]}"
        assert torch.equal(tokens[r0:r0 + B, :n], rp), f"batch {k} (T {T}): tokens"
        assert torch.equal(logits[r0:r0 + B, :n], rl), f"batch {k} (T {T}): logits not bit-identical"
        assert int(tokens[r0:r0 + B, n:].abs().sum()) == 0 and float(logits[r0:r0 + B, n:].abs().sum()) == 0.0, \
            f"batch {k}: output past its exit step {n} is not PAD / zeros"
        r0 += B


@pytest.mark.parametrize("is_test", [False, True])
def test_short_and_very_long_memories_in_one_block(is_test):
    """Rows 2 and 3 share a block of the two-row kernel: 7 keys (less than one tile: three of the row's four waves own no tile)
    beside 1100 keys (69 tiles).  Eleven rows: the last block repeats its row."""
    cfg, m = engine_model("T2", 150, 1234, 1.81 if is_test else 0.0)
    eng = m.engine()
    layout = [(3, 7), (2, 1100), (4, 261), (1, 16), (1, 33)]
    mems, packed = _synthetic_group(eng, layout, 5)
    tokens, logits, steps = _submit(eng, packed, layout, is_test)
    assert len(steps) == (len(layout) if is_test else 1)
    _check_against_single(eng, mems, layout, tokens, logits, steps, is_test)


# ---------------------------------------------------------------------------------------------------------------------
# 3. early exit
# ---------------------------------------------------------------------------------------------------------------------
def test_batches_of_a_ragged_group_end_at_their_own_steps(cases):
    c = _case(cases, "t2_greedy_early")  # end_bias 1.81: rows end at different steps
    cfg, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], c["end_bias"])
    full = c["max_seq_len"] + 1
    imgs = [synth.synth_images(3, c["H"], c["W"], seed=c["iseed"] + i).cuda() for i in range(6)]
    imgs.append((synth.synth_images(3, c["H"], c["W"], seed=77) * 0.05).cuda())  # a faint crop: different dynamics
    imgs += [synth.synth_images(1, 48, 32, seed=31).cuda(), synth.synth_images(2, 48, 48, seed=32).cuda(),
             synth.synth_images(1, 48, 16, seed=33).cuda()]
    imgs = [imgs[i] for i in (0, 7, 1, 8, 2, 3, 9, 4, 5, 6)]  # sizes interleaved
    ref = _sync_refs(m, imgs, True)
    want = [p.shape[1] for p, _ in ref]
    assert len(set(want)) > 1, want  # the batches really stop at different steps
    with torch.no_grad():
        _mixed(m, 5)
        outs = [m(x, _go(x.shape[0]), is_train=False, is_test=True) for x in imgs]
        eng = m.engine()
        tickets = [o[2]["decode"].ticket for o in outs]
        assert tickets[:5] == [tickets[0]] * 5 and tickets[5:] == [tickets[5]] * 5 and tickets[0] != tickets[5]
        for grp in (0, 5):
            assert eng.decode_steps(tickets[grp]) == want[grp:grp + 5]  # d2t_decode_steps: the single-batch step counts
        for (p, l, extra), (rp, rl) in zip(outs, ref):
            assert p.shape[1] == full and l.shape[1] == full  # full-size views while in flight
            cp, cl = extra["decode"].result()
            assert cp.shape == rp.shape and torch.equal(cp, rp) and torch.equal(cl, rl)
            n = rp.shape[1]
            assert int(p[:, n:].abs().sum()) == 0 and float(l[:, n:].abs().sum()) == 0.0, "output past the batch's exit"
        m.synchronize()
    _plain(m)


# ---------------------------------------------------------------------------------------------------------------------
# 4. graph reuse
# ---------------------------------------------------------------------------------------------------------------------
def test_two_size_mixes_with_one_row_total_share_a_captured_loop():
    cfg, m = engine_model("T2", 40, 1234, 0.0)
    eng = m.engine()
    mix_a, mix_b = [(2, 300), (3, 40), (1, 7)], [(1, 100), (1, 20), (4, 64)]  # six rows each; A holds more memory rows
    (mems_a, packed_a), (mems_b, packed_b) = _synthetic_group(eng, mix_a, 11), _synthetic_group(eng, mix_b, 12)
    for _ in range(4):  # every memory slot has seen the larger mix: buffers have their final size, loops are captured
        out_a = _submit(eng, packed_a, mix_a, False)
    n0 = eng.graph_count()
    assert n0 >= 1
    results = []
    for i in range(6):  # back to back, alternating
        mix, mems, packed = (mix_b, mems_b, packed_b) if i % 2 == 0 else (mix_a, mems_a, packed_a)
        results.append((mix, mems, _submit(eng, packed, mix, False)))
    assert eng.graph_count() == n0, "a different size mix with the same row total re-captured the step loop"
    n1 = eng.graph_count()
    for mix, mems, (tokens, logits, steps) in results:
        _check_against_single(eng, mems, mix, tokens, logits, steps, False)
    assert eng.graph_count() >= n1  # (the single-batch references capture loops of their own)


# ---------------------------------------------------------------------------------------------------------------------
# 5. operator level
# ---------------------------------------------------------------------------------------------------------------------
def _ragged_row_run(kind, parts, Lmax, step):
    """parts: uniform sub-problems (ops._row_problem, row b -> sample b) of different T; one ragged launch over all their rows"""
    lib = _lib.require_device()
    cat = lambda k: torch.cat([P[k] for P in parts]).contiguous().to(DEV)
    dv = {k: ops._d(parts[0][k]) for k in ops.ROW_KEYS}
    qkv, xres, sk, sv = cat("qkv"), cat("xres"), cat("sk"), cat("sv")
    mem = torch.cat([P["mem"].reshape(-1, 256) for P in parts]).contiguous().to(DEV)
    row0, length, base = [], [], 0
    for P in parts:
        for b in range(P["M"]):
            row0.append(base + b * P["T"])
            length.append(P["T"])
        base += P["M"] * P["T"]
    M = len(row0)
    y2 = torch.full((M, 256), ops.NAN, device=DEV)
    st = ops._d(ops._i32([step]))
    p = _lib.ptr
    rc = lib.d2t_op_decoder_row_ragged(kind, p(qkv), p(xres), p(sk), p(sv), p(mem), p(dv["ca_in_w"]), p(dv["ca_in_b"]),
                                       p(dv["sa_out_w"]), p(dv["sa_out_b"]), p(dv["ca_out_w"]), p(dv["ca_out_b"]), p(dv["ln_g"]),
                                       p(dv["ln_b"]), 1e-5, p(y2), p(st), M, Lmax, M, base, (C.c_int32 * M)(*row0),
                                       (C.c_int32 * M)(*length), _lib.stream_of(y2))
    torch.cuda.synchronize()
    assert rc == 0, f"d2t_op_decoder_row_ragged kind {kind}: rc {rc}"
    return y2.cpu()


# (rows, T) per part: a one-row part, T < 16, T % 16 != 0, more than 64 tiles, an odd row total
RAGGED_ROW_PARTS = [(2, 15), (1, 1), (3, 261), (1, 1695), (2, 16), (2, 513)]


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_ragged_row_op_vs_float64(kind):
    """The tolerance is the one tests/test_decode_ops_gpu.py uses for the uniform kinds (its `measured` rule; for the
    split-bf16 kinds against the split float64 evaluation, plus 1e-3 relative against plain float64), per part."""
    Lmax, step = 64, 5
    parts = [ops._row_problem(M, 256, T, Lmax, step, seed=400 + i) for i, (M, T) in enumerate(RAGGED_ROW_PARTS)]
    y = _ragged_row_run(kind, parts, Lmax, step)
    bx3 = kind in (3, 4)
    r0 = 0
    for i, P in enumerate(parts):
        yi = y[r0:r0 + P["M"]]
        r0 += P["M"]
        refs = ops._row_refs(("ragged", i), P, split=bx3)
        y64, y32 = refs[0], refs[1]
        info = dict(M=P["M"], T=P["T"], step=step, D=256)
        if bx3:
            e32 = float((y32.double() - y64).abs().max())
            ops._measured(f"ragged_row_kind{kind}_vs_split64", yi, refs[2], e32=e32, **info)
            rel = float((yi.double() - y64).abs().max() / y64.abs().max())
            ops._fig(f"ragged_row_kind{kind}_vs_plain64", rel=rel, **info)
            assert rel <= 1e-3
        else:
            ops._measured(f"ragged_row_kind{kind}", yi, y64, y32, **info)
        # ... and every part equals the uniform op on that part alone, bit for bit
        assert torch.equal(ops._bits(yi), ops._bits(ops._row_run(kind, P, check_cache=False))), f"part {i} differs from the uniform op"


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
@pytest.mark.parametrize("M,T", [(5, 261), (2, 7), (64, 1695)])
def test_ragged_row_op_with_equal_lengths_is_the_uniform_op(kind, M, T):
    P = ops._row_problem(M, 256, T, 64, 3, seed=77 + M)
    assert torch.equal(ops._bits(_ragged_row_run(kind, [P], 64, 3)), ops._bits(ops._row_run(kind, P, check_cache=False)))


def test_ragged_row_op_refuses_slices_outside_the_memory():
    lib = _lib.require_device()
    P = ops._row_problem(2, 256, 16, 64, 0, seed=1)
    dv = {k: ops._d(P[k]) for k in ops.ROW_KEYS + ("qkv", "xres", "sk", "sv")}
    mem = P["mem"].reshape(-1, 256).contiguous().to(DEV)
    y2 = torch.zeros(2, 256, device=DEV)
    st = ops._d(ops._i32([0]))
    p = _lib.ptr

    def call(row0, length, kind=3, mem_rows=32):
        return lib.d2t_op_decoder_row_ragged(kind, p(dv["qkv"]), p(dv["xres"]), p(dv["sk"]), p(dv["sv"]), p(mem), p(dv["ca_in_w"]),
                                             p(dv["ca_in_b"]), p(dv["sa_out_w"]), p(dv["sa_out_b"]), p(dv["ca_out_w"]),
                                             p(dv["ca_out_b"]), p(dv["ln_g"]), p(dv["ln_b"]), 1e-5, p(y2), p(st), 2, 64, 2, mem_rows,
                                             (C.c_int32 * 2)(*row0), (C.c_int32 * 2)(*length), _lib.stream_of(y2))
    assert call([0, 16], [16, 16]) == 0
    for row0, length in (([0, 17], [16, 16]), ([0, 16], [16, 0]), ([-1, 16], [16, 16]), ([0, 0], [16, 4097])):
        assert call(row0, length) == D2T_EINVAL, (row0, length)
    assert call([0, 16], [16, 16], kind=0) == D2T_EINVAL and call([0, 16], [16, 16], kind=5) == D2T_EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _raw_submit(eng, packed, rows, Ts, n=None, start=None, tokens=None, logits=None):
    S, V = eng.cfg.max_seq_len + 1, max(eng.cfg.vocab, 1)
    B = max(1, sum(max(r, 0) for r in rows))
    start = torch.full((B,), R.GO, dtype=torch.int64, device=DEV) if start is None else start
    tokens = torch.zeros((B, S), dtype=torch.int64, device=DEV) if tokens is None else tokens
    logits = torch.zeros((B, S, V), device=DEV) if logits is None else logits
    n = len(rows) if n is None else n
    k = max(len(rows), 1)
    t = C.c_int64(0)
    rc = eng.lib.d2t_decode_greedy_submit_ragged(eng.ctx, _lib.ptr(packed), n, (C.c_int32 * k)(*rows), (C.c_int32 * k)(*Ts),
                                                 _lib.ptr(start), 0, _lib.ptr(tokens), _lib.ptr(logits), _lib.stream_of(packed),
                                                 C.byref(t))
    return rc, eng.lib.d2t_last_error(eng.ctx).decode()


def test_refusals_leave_the_context_usable():
    cfg, m = engine_model("T2", 12, 1234, 0.0)
    eng = m.engine()
    packed = torch.randn(4096, 256, generator=torch.Generator().manual_seed(3)).to(DEV)
    t0 = int(eng.lib.d2t_decode_last_ticket(eng.ctx))
    for rows, Ts, n, code, words in [
        ([2, 1], [8, 0], None, D2T_EINVAL, "memory length 0"),
        ([2, 1], [8, -3], None, D2T_EINVAL, "memory length -3"),
        ([1, 1], [8, 4097], None, D2T_EINVAL, "memory length 4097 > 4096"),
        ([1] * 65, [4] * 65, None, D2T_EINVAL, "at most 64 batches"),
        ([], [], 0, D2T_EINVAL, "at least one row"),
        ([2, 0], [8, 8], None, D2T_EINVAL, "has 0 rows"),
    ]:
        rc, msg = _raw_submit(eng, packed, rows, Ts, n)
        assert rc == code and words in msg, (rows, Ts, rc, msg)
    if torch.cuda.device_count() > 1:  # (a second GPU is the only way to own a pointer of another device)
        other = torch.zeros(64, 256, device="cuda:1")
        rc, msg = _raw_submit(eng, other, [1], [8])
        assert rc == D2T_EINVAL and "device" in msg, (rc, msg)
    assert int(eng.lib.d2t_decode_last_ticket(eng.ctx)) == t0  # nothing was enqueued
    # a context without the TFM decoder
    _, ma = engine_model("TS0", 12, 1234, 0.0)
    ea = ma.engine()
    rc, msg = _raw_submit(ea, packed, [1], [8])
    assert rc == D2T_ESTATE and "TFM decoder" in msg, (rc, msg)
    # the first context still decodes, and correctly
    layout = [(2, 9), (1, 30)]
    mems, pk = _synthetic_group(eng, layout, 21)
    tokens, logits, steps = _submit(eng, pk, layout, False)
    _check_against_single(eng, mems, layout, tokens, logits, steps, False)


def test_projected_kv_decoder_refuses_and_the_model_falls_back(cases):
    """d_model 512 (T1 / C1) lays its cross K / V out by memory length: the ragged entry says so, and Model keeps today's
    flush-on-change grouping whatever decode_group_mixed says -- same results as before."""
    c = _case(cases, "t1_greedy")
    cfg, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], c["end_bias"])
    eng = m.engine()
    assert not eng.supports_ragged_groups()
    rc, msg = _raw_submit(eng, torch.zeros(64, 512, device=DEV), [1, 1], [8, 9])
    assert rc == D2T_ESTATE and "d_model 256" in msg and "memory length" in msg, (rc, msg)
    imgs = [synth.synth_images(B, H, W, seed=600 + i).cuda() for i, (B, H, W) in enumerate([(2, 32, 64), (2, 32, 64), (1, 32, 32), (2, 32, 64)])]
    ref = _sync_refs(m, imgs, False)
    with torch.no_grad():
        _mixed(m, 3)
        outs = [m(x, _go(x.shape[0]), is_train=False) for x in imgs]
        tk = [o[2]["decode"].ticket for o in outs]
        # every change of size launched what was collected before it: batches 0-1 together, batch 2 alone, batch 3 still waits
        assert tk[0] is not None and tk[0] == tk[1] and tk[2] == tk[0] + 1 and tk[3] is None
        for o, (rp, rl) in zip(outs, ref):
            p, l = o[2]["decode"].result()
            assert torch.equal(p, rp) and torch.equal(l, rl)
        m.synchronize()
    _plain(m)


# ---------------------------------------------------------------------------------------------------------------------
# 7. default off
# ---------------------------------------------------------------------------------------------------------------------
def test_without_the_switch_a_change_of_size_flushes_the_group(cases):
    c = _case(cases, "t2_greedy")
    cfg, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], c["end_bias"])
    imgs = [synth.synth_images(2, 48, 64, seed=700).cuda(), synth.synth_images(2, 48, 32, seed=701).cuda(),
            synth.synth_images(1, 48, 32, seed=702).cuda()]
    ref = _sync_refs(m, imgs, False)
    with torch.no_grad():
        m.pipelined, m.decode_chains, m.decode_group = True, 2, 3
        assert m.decode_group_mixed is False
        eng = m.engine()
        t0 = int(eng.lib.d2t_decode_last_ticket(eng.ctx))
        h = []
        for i, x in enumerate(imgs):
            h.append(m(x, _go(x.shape[0]), is_train=False)[2]["decode"])
            # a new memory length, then a new row count: each launches what was collected before it
            assert [q.ticket is not None for q in h] == [True] * i + [False]
        m.synchronize()
        assert int(eng.lib.d2t_decode_last_ticket(eng.ctx)) - t0 == 3
        for q, (rp, rl) in zip(h, ref):
            p, l = q.result()
            assert torch.equal(p, rp) and torch.equal(l, rl)
        # the same three forwards with the switch on: one group, one decode
        m.decode_group_mixed = True
        h = [m(x, _go(x.shape[0]), is_train=False)[2]["decode"] for x in imgs]
        assert len({q.ticket for q in h}) == 1 and h[0].ticket == t0 + 4
        for q, (rp, rl) in zip(h, ref):
            p, l = q.result()
            assert torch.equal(p, rp) and torch.equal(l, rl)
        # the row budget: 2 + 2 rows fit decode_group_rows = 4, the fifth row starts a new group
        m.decode_group_rows, m.decode_group = 4, 6
        h = [m(x, _go(x.shape[0]), is_train=False)[2]["decode"] for x in imgs]
        assert h[0].ticket is not None and h[0].ticket == h[1].ticket and h[2].ticket is None
        m.synchronize()
        for q, (rp, rl) in zip(h, ref):
            p, l = q.result()
            assert torch.equal(p, rp) and torch.equal(l, rl)
    _plain(m)
