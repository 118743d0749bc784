"""GPU: TFM beam search over samples whose encoder memories have DIFFERENT lengths, in one captured step loop
(d2t_decode_beam_batch_ragged, Model.beam_search_batch on a list of image tensors).  The invariant: every sample's tokens,
length and score are those of its own d2t_decode_beam call bit for bit -- a row of the per-sample ragged build of the one-row
kernel reads its sample's slice of the packed memory rows through the row map, and its arithmetic depends on that sample's
length alone, wherever the row sits after the live rows have been compacted.

The fp32-MFMA cross-attention inside the step loop (`cross_fp32`) is selected by a probe build only; here it is covered at
the operator level (kind 2 of d2t_op_decoder_row_ragged_beam), the shipped split-bf16 form at both levels."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_decode_ops_gpu as ops
from conftest import engine_model
from doc2tex_amd import Model, _lib, synth
from doc2tex_amd.engine import pack_memories
from oracle import restatement as R
from test_parity_gpu import _case, _score_tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
D2T_EINVAL, D2T_ESTATE = 1, 4  # include/d2t.h


def _fbits(v):
    return int(np.float32(v).view(np.int32))


def _same(got, want, what):
    """(seq [1, len], score) pairs: tokens, length and the score's float bits"""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, ((s1, v1), (s2, v2)) in enumerate(zip(got, want)):
        assert s1.shape == s2.shape and torch.equal(s1, s2), f"{what}: sample {i}: {s1.tolist()} != {s2.tolist()}"
        assert _fbits(v1) == _fbits(v2), f"{what}: sample {i}: score {v1!r} != {v2!r}"


def _per_sample(eng, mems, beam):
    """d2t_decode_beam on every sample alone"""
    return [eng.decode_beam(m[j:j + 1].contiguous(), beam) for m in mems for j in range(m.shape[0])]


def _encode(m, imgs):
    with torch.no_grad():
        return [m.forward_encoder(x)[0].contiguous() for x in imgs]


def _end_steps(results):
    """per sample: the step at which its returned hypothesis emitted [s] (None: it ran into the length limit)"""
    return [s.shape[1] - 1 if int(s[0, -1]) == R.END else None for s, _ in results]


# ---------------------------------------------------------------------------------------------------------------------
# 1. reference fixtures
# ---------------------------------------------------------------------------------------------------------------------
def test_three_reference_fixtures_in_one_search(cases):
    cs = [_case(cases, "beam", n) for n in ("c4_beam5_160", "c4_beam5_128", "c4_beam5_96")]
    for c in cs:
        assert (c["config"], c["wseed"], c["max_seq_len"], c["end_bias"], c["beam_size"]) == ("C4", 1234, 24, 1.8, 5)
    assert len({(c["H"], c["W"]) for c in cs}) == 3
    cfg, m = engine_model("C4", 24, 1234, 1.8, beam_size=5)
    imgs = [synth.synth_images(1, c["H"], c["W"], seed=c["iseed"]).cuda() for c in cs]
    eng = m.engine()
    assert eng.supports_ragged_beam()
    g0 = eng.graph_count()
    with torch.no_grad():
        out = m.beam_search_batch(imgs, 5)
    assert eng.graph_count() == g0 + 1  # ONE search
    assert len(out) == 3
    for c, (seq, score) in zip(cs, out):
        assert seq.shape[0] == 1 and seq[0].tolist() == c["seq"], (c["case"], seq.tolist())
        print(f"FIG ragged_beam_fixture {c['case']} dscore={abs(score - c['score']):.3e}")
        assert abs(score - c["score"]) <= _score_tol(m, len(c["seq"])), (c["case"], score, c["score"])
    # the 160 crop completes at once while the others run to the end: its rows drop out in the middle of the search
    assert out[0][0][0].tolist() == [R.END] and out[1][0].shape[1] == 25 and out[2][0].shape[1] == 25


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit identity to the per-sample call
# ---------------------------------------------------------------------------------------------------------------------
# (samples, H, W): five sizes, unequal sample counts.  Seeds 3100 + i at end_bias 1.8, max_seq_len 16, chosen on the CPU oracle
# (oracle.restatement's beam search): at beam 3 the samples' hypotheses end at steps 0, 0, 0, 9, 10, 0, 2 and two never end;
# at beam 5 at steps 2, 11, 2, 2, 2, 2, 2 and two never end
T2_CROPS = [(3, 48, 64), (2, 48, 32), (1, 48, 48), (1, 48, 16), (2, 32, 64)]


@pytest.mark.parametrize("beam", [3, 5])
def test_every_sample_equals_its_own_beam_search(beam):
    cfg, m = engine_model("T2", 16, 1234, 1.8, beam_size=beam)
    eng = m.engine()
    imgs = [synth.synth_images(n, H, W, seed=3100 + i).cuda() for i, (n, H, W) in enumerate(T2_CROPS)]
    mems = _encode(m, imgs)
    assert len({x.shape[1] for x in mems}) >= 4, [x.shape for x in mems]
    want = _per_sample(eng, mems, beam)
    ends = _end_steps(want)
    print("FIG ragged_beam_end_steps", beam, ends)
    done = sorted({e for e in ends if e is not None})
    assert len(done) >= 2, ends  # samples complete at different steps ...
    assert any(s.shape[1] - 1 > done[0] for s, _ in want), ends  # ... and one completes while others are still live
    with torch.no_grad():
        got = m.beam_search_batch(imgs, beam)  # list form: encode each tensor, pack, ONE search
    _same(got, want, f"T2 beam {beam}")
    _same(eng.decode_beam_batch_ragged(*pack_memories(mems), beam), want, f"T2 beam {beam} (engine call)")
    # a tuple, and the single-tensor form is still today's call
    with torch.no_grad():
        _same(m.beam_search_batch(tuple(imgs[1:3]), beam), want[3:6], "tuple")
        _same(m.beam_search_batch(imgs[0], beam), want[:3], "single tensor")


def _synthetic(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, T, 256, generator=g).to(DEV) for T in lengths]


@pytest.mark.parametrize("beam", [3, 5])
def test_short_and_very_long_memories_in_one_search(beam):
    """7 keys (less than one tile: three of a row's four waves own no tile), 1100 (69 tiles), 261 and 33 (no multiple of 16),
    16 (exactly one tile) and ONE key."""
    cfg, m = engine_model("T2", 16, 1234, 1.8, beam_size=beam)
    eng = m.engine()
    mems = _synthetic([7, 1100, 261, 16, 33, 1], 5)
    want = _per_sample(eng, mems, beam)
    _same(eng.decode_beam_batch_ragged(*pack_memories(mems), beam), want, f"synthetic beam {beam}")
    # the same samples in another order: other offsets, other rows, the same results
    order = [3, 1, 5, 0, 4, 2]
    _same(eng.decode_beam_batch_ragged(*pack_memories([mems[i] for i in order]), beam), [want[i] for i in order], "reordered")


def test_nothing_completes_and_a_single_sample(cases):
    c = _case(cases, "beam", "t2_beam3_nofinish")
    assert (c["end_bias"], c["max_seq_len"], c["beam_size"]) == (0.0, 6, 3)
    cfg, m = engine_model("T2", 6, 1234, 0.0, beam_size=3)
    eng = m.engine()
    imgs = [synth.synth_images(n, H, W, seed=3200 + i).cuda() for i, (n, H, W) in enumerate(T2_CROPS)]
    imgs.append(synth.synth_images(1, c["H"], c["W"], seed=c["iseed"]).cuda())  # the fixture's crop
    mems = _encode(m, imgs)
    want = _per_sample(eng, mems, 3)
    assert all(e is None for e in _end_steps(want)) and all(s.shape[1] == 7 for s, _ in want)
    assert want[-1][0][0].tolist() == c["seq"]
    with torch.no_grad():
        _same(m.beam_search_batch(imgs, 3), want, "nothing completes")
    # N = 1, for every size
    for i, mem in enumerate(mems):
        for j in range(mem.shape[0]):
            one = eng.decode_beam_batch_ragged(mem[j].contiguous(), [mem.shape[1]], 3)
            _same(one, [eng.decode_beam(mem[j:j + 1].contiguous(), 3)], f"N = 1, tensor {i}")
    with torch.no_grad():
        _same(m.beam_search_batch([imgs[3]], 3), want[6:7], "a list of one tensor")
        assert m.beam_search_batch([], 3) == []


# ---------------------------------------------------------------------------------------------------------------------
# 3. equal lengths = the uniform call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,beam", [(5, 33, 5), (1, 261, 3), (4, 16, 2)])
def test_equal_lengths_give_what_the_uniform_call_gives(N, T, beam):
    cfg, m = engine_model("T2", 16, 1234, 1.8, beam_size=beam)
    eng = m.engine()
    mem = torch.randn(N, T, 256, generator=torch.Generator().manual_seed(N + T)).to(DEV)
    _same(eng.decode_beam_batch_ragged(mem.reshape(-1, 256), [T] * N, beam), eng.decode_beam_batch(mem, beam), "uniform")


# ---------------------------------------------------------------------------------------------------------------------
# 4. graph reuse
# ---------------------------------------------------------------------------------------------------------------------
def test_two_length_mixes_with_one_sample_count_share_a_captured_loop():
    cfg, m = engine_model("T2", 16, 1234, 1.8, beam_size=3)
    eng = m.engine()
    mems_a, mems_b = _synthetic([300, 40, 7, 64], 11), _synthetic([100, 20, 64, 5], 12)  # four samples each; A holds more rows
    first = eng.decode_beam_batch_ragged(*pack_memories(mems_a), 3)
    n0 = eng.graph_count()
    assert n0 >= 1
    runs = [(mems_b, eng.decode_beam_batch_ragged(*pack_memories(mems_b), 3)),
            (mems_a, eng.decode_beam_batch_ragged(*pack_memories(mems_a), 3)),
            (mems_b, eng.decode_beam_batch_ragged(*pack_memories(mems_b), 3))]
    assert eng.graph_count() == n0, "another mix of lengths with the same N and beam re-captured the step loop"
    eng.decode_beam_batch_ragged(*pack_memories(mems_b), 5)
    assert eng.graph_count() == n0 + 1  # (another beam width is another loop)
    _same(first, _per_sample(eng, mems_a, 3), "first run")
    for mems, got in runs:
        _same(got, _per_sample(eng, mems, 3), "replayed loop")


# ---------------------------------------------------------------------------------------------------------------------
# 5. operator level
# ---------------------------------------------------------------------------------------------------------------------
# (rows, T, samples, row map) per part: several rows on one sample, a map that is not the identity, T < 16, T % 16 != 0,
# more than 64 tiles, a one-row part of one key
BEAM_ROW_PARTS = [(2, 15, 1, [0, 0]), (1, 1, 1, [0]), (3, 261, 2, [1, 0, 1]), (1, 1695, 1, [0]), (2, 16, 2, [1, 0]), (2, 513, 1, [0, 0])]
OP_LMAX, OP_STEP = 64, 5
_PARTS = {}


def _parts():
    """the uniform sub-problems (inputs only: shared by both kinds, never written)"""
    if not _PARTS:
        for i, (M, T, S, rm) in enumerate(BEAM_ROW_PARTS):
            anc = np.random.RandomState(40 + i).randint(0, M, size=(M, OP_LMAX))  # earlier positions live in other cache rows
            _PARTS[i] = ops._row_problem(M, 256, T, OP_LMAX, OP_STEP, samples=S, row_map=rm, rows=M, anc=anc, seed=500 + i)
    return [_PARTS[i] for i in range(len(BEAM_ROW_PARTS))]


def _ragged_beam_row_call(kind, t, M, Lmax, rows, mem_rows, samples, row0, length, with_anc=True, row_map="row_map"):
    lib = _lib.require_device()
    p = _lib.ptr
    return lib.d2t_op_decoder_row_ragged_beam(
        kind, p(t["qkv"]), p(t["xres"]), p(t["sk"]), p(t["sv"]), p(t["mem"]), p(t["ca_in_w"]), p(t["ca_in_b"]), p(t["sa_out_w"]),
        p(t["sa_out_b"]), p(t["ca_out_w"]), p(t["ca_out_b"]), p(t["ln_g"]), p(t["ln_b"]), 1e-5, p(t["y2"]), p(t["step"]), M, Lmax, rows,
        mem_rows, samples, (C.c_int32 * len(row0))(*row0), (C.c_int32 * len(length))(*length), p(t.get(row_map)),
        p(t["anc"]) if with_anc else None, t["anc"].shape[1] if with_anc else 0, _lib.stream_of(t["y2"]))


def _combined(parts, perm):
    """ONE launch over all parts' rows in the order `perm`: the rows of a sample are scattered, the row map and the ancestry
    rows follow them, the per-sample tables and the caches stay where they are"""
    src = [(i, b) for i, P in enumerate(parts) for b in range(P["M"])]
    row_off = np.concatenate([[0], np.cumsum([P["M"] for P in parts])])  # cache rows: part after part
    smp_off = np.concatenate([[0], np.cumsum([P["samples"] for P in parts])])
    row0, length, base = [], [], 0
    for P in parts:
        for _ in range(P["samples"]):
            row0.append(base)
            length.append(P["T"])
            base += P["T"]
    t = {k: ops._d(parts[0][k]) for k in ops.ROW_KEYS}
    pick = lambda k: torch.stack([parts[i][k][b] for i, b in (src[g] for g in perm)]).contiguous().to(DEV)
    t["qkv"], t["xres"] = pick("qkv"), pick("xres")
    t["sk"] = torch.cat([P["sk"] for P in parts]).contiguous().to(DEV)
    t["sv"] = torch.cat([P["sv"] for P in parts]).contiguous().to(DEV)
    t["mem"] = torch.cat([P["mem"].reshape(-1, 256) for P in parts]).contiguous().to(DEV)
    t["row_map"] = ops._d(ops._i32([int(smp_off[i]) + int(parts[i]["row_map"][b]) for i, b in (src[g] for g in perm)]))
    t["anc"] = ops._d(ops._i32(np.stack([parts[i]["anc"][b].numpy() + int(row_off[i]) for i, b in (src[g] for g in perm)])))
    t["y2"] = torch.full((len(perm), 256), ops.NAN, device=DEV)
    t["step"] = ops._d(ops._i32([OP_STEP]))
    return t, src, row0, length, base, int(smp_off[-1]), int(row_off[-1])


@pytest.mark.parametrize("kind", [2, 4])
def test_ragged_beam_row_op_vs_float64(kind):
    """The tolerance is the one tests/test_decode_ops_gpu.py uses for the uniform kinds (its `measured` rule; for the
    split-bf16 kind against the split float64 evaluation, plus 1e-3 relative against plain float64), per part."""
    parts = _parts()
    total = sum(P["M"] for P in parts)
    perm = np.random.RandomState(3).permutation(total).tolist()
    assert perm != sorted(perm)
    t, src, row0, length, mem_rows, samples, rows = _combined(parts, perm)
    assert samples == 8 and rows == total == 11 and mem_rows == sum(P["samples"] * P["T"] for P in parts)
    rc = _ragged_beam_row_call(kind, t, total, OP_LMAX, rows, mem_rows, samples, row0, length)
    torch.cuda.synchronize()
    assert rc == 0, f"d2t_op_decoder_row_ragged_beam kind {kind}: rc {rc}"
    y = t["y2"].cpu()
    bx3 = kind == 4
    for i, P in enumerate(parts):
        yi = torch.stack([y[perm.index(g)] for g in range(len(src)) if src[g][0] == i])
        refs = ops._row_refs(("ragged_beam", i), P, split=bx3)
        y64, y32 = refs[0], refs[1]
        info = dict(M=P["M"], T=P["T"], step=OP_STEP, D=256)
        if bx3:
            e32 = float((y32.double() - y64).abs().max())
            ops._measured(f"ragged_beam_row_kind{kind}_vs_split64", yi, refs[2], e32=e32, **info)
            rel = float((yi.double() - y64).abs().max() / y64.abs().max())
            ops._fig(f"ragged_beam_row_kind{kind}_vs_plain64", rel=rel, **info)
            assert rel <= 1e-3
        else:
            ops._measured(f"ragged_beam_row_kind{kind}", yi, y64, y32, **info)
        # ... and every part equals the uniform op on that part alone, bit for bit
        assert torch.equal(ops._bits(yi), ops._bits(ops._row_run(kind, P, check_cache=False))), f"part {i} differs from the uniform op"
    # this step's k / v went to the launched rows' own cache rows, everything else is untouched
    for name, off in (("sk", 256), ("sv", 512)):
        want = torch.cat([P[name] for P in parts]).clone()
        want[:total, :, OP_STEP, :] = t["qkv"].cpu()[:, off:off + 256].view(total, 8, 32)
        assert torch.equal(ops._bits(t[name].cpu()), ops._bits(want)), f"{name}: cache differs from (old contents + this step's row)"


def test_ragged_beam_row_op_refuses_what_it_cannot_serve():
    parts = _parts()[:2]  # (2, 15) and (1, 1): three rows, two samples, 16 packed memory rows
    t, src, row0, length, mem_rows, samples, rows = _combined(parts, [0, 1, 2])
    assert (row0, length, mem_rows, samples, rows) == ([0, 15], [15, 1], 16, 2, 3)
    call = lambda kind=4, r0=row0, ln=length, mr=mem_rows, Lmax=OP_LMAX, **kw: _ragged_beam_row_call(kind, t, 3, Lmax, rows, mr, samples,
                                                                                                 r0, ln, **kw)
    assert call() == 0 and call(kind=2) == 0 and call(with_anc=False) == 0
    for kind in (0, 1, 3, 5):  # the two-row builds know neither row map nor ancestry
        assert call(kind=kind) == D2T_EINVAL, kind
    assert call(r0=[0, 16]) == D2T_EINVAL  # a slice that would run past the packed buffer
    assert call(ln=[17, 1]) == D2T_EINVAL  # ... likewise
    assert call(mr=15) == D2T_EINVAL
    assert call(r0=[-1, 15]) == D2T_EINVAL and call(ln=[15, 0]) == D2T_EINVAL and call(ln=[4097, 1]) == D2T_EINVAL
    assert call(row_map="none") == D2T_EINVAL  # no row map: these are the greedy builds' tables (d2t_op_decoder_row_ragged)
    t["bad_map"] = ops._d(ops._i32([0, 2, 1]))
    assert call(row_map="bad_map") == D2T_EINVAL  # a sample the tables do not hold
    assert call(Lmax=513) == D2T_EINVAL  # an ancestry row longer than the kernel keeps (ANC_MAX)
    t["anc"] = t["anc"] + 3
    assert call() == D2T_EINVAL  # an ancestry row that points past the cache
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _raw(eng, packed, Ts, beam, N=None):
    n = len(Ts) if N is None else N
    S = eng.cfg.max_seq_len + 1
    k = max(len(Ts), 1)
    seq, ln, score = (C.c_int64 * (max(n, 1) * S))(), (C.c_int32 * max(n, 1))(), (C.c_float * max(n, 1))()
    rc = eng.lib.d2t_decode_beam_batch_ragged(eng.ctx, _lib.ptr(packed), n, (C.c_int32 * k)(*Ts), beam, seq, ln, score,
                                              _lib.stream_of(packed))
    return rc, eng.lib.d2t_last_error(eng.ctx).decode()


def test_refusals_leave_the_context_usable():
    cfg, m = engine_model("T2", 12, 1234, 1.8, beam_size=3)
    eng = m.engine()
    packed = torch.randn(4200, 256, generator=torch.Generator().manual_seed(3)).to(DEV)
    g0 = eng.graph_count()
    for Ts, beam, N, code, words in [
        ([], 3, 0, D2T_EINVAL, "1 to 1024 samples"),
        ([4], 3, -2, D2T_EINVAL, "1 to 1024 samples"),
        ([1] * 1025, 3, None, D2T_EINVAL, "1 to 1024 samples"),
        ([8, 0], 3, None, D2T_EINVAL, "memory length 0"),
        ([8, -3], 3, None, D2T_EINVAL, "memory length -3"),
        ([8, 4097], 3, None, D2T_EINVAL, "memory length 4097"),
        ([8, 9], 0, None, D2T_EINVAL, "beam_size must be in [1,16]"),
        ([8, 9], 17, None, D2T_EINVAL, "beam_size must be in [1,16]"),
    ]:
        rc, msg = _raw(eng, packed, Ts, beam, N)
        assert rc == code and words in msg, (Ts, beam, rc, msg)
    if torch.cuda.device_count() > 1:  # (a second GPU is the only way to own a pointer of another device)
        rc, msg = _raw(eng, torch.zeros(64, 256, device="cuda:1"), [8], 3)
        assert rc == D2T_EINVAL and "device" in msg, (rc, msg)
    # one cross-attention block per sample (beam_shared_tile) keeps the host-side loop: refused while it is on
    eng.set_beam_shared_tile(True)
    assert not eng.supports_ragged_beam()
    rc, msg = _raw(eng, packed, [8, 9], 3)
    assert rc == D2T_ESTATE and "beam_shared_tile" in msg and "d2t_decode_beam_batch" in msg, (rc, msg)
    eng.set_beam_shared_tile(False)
    assert eng.supports_ragged_beam()
    assert eng.graph_count() == g0  # nothing was captured, nothing enqueued
    # ... and the context still searches, correctly
    mems = _synthetic([9, 30, 4], 21)
    _same(eng.decode_beam_batch_ragged(*pack_memories(mems), 3), _per_sample(eng, mems, 3), "after the refusals")


def test_contexts_that_the_ragged_search_does_not_serve(cases):
    packed = torch.zeros(64, 512, device=DEV)
    # beam_size * vocab over the uniform call's cap: 16 x 4100 > 16 x 4096 (weights as constructed: nothing is decoded)
    cfg = synth.make_config("T2", device=DEV, max_seq_len=8, beam_size=16)
    cfg["num_class"] = 4100
    big = Model(cfg).to(DEV).eval()
    rc, msg = _raw(big.engine(), packed, [8, 9], 16)
    assert rc == D2T_EINVAL and "beam_size * vocab too large" in msg, (rc, msg)
    # max_seq_len + 2 > 512 (ancestry rows that no longer fit the row kernel) cannot be reached through the interface: a
    # context is created with max_seq_len <= 510. The longest one that the model's 500-row position table lets the
    # engine build (max_seq_len + 2 <= 500) is served
    with pytest.raises(RuntimeError, match="max_seq_len must be <= 510"):
        Model(synth.make_config("T2", device=DEV, max_seq_len=511, beam_size=3)).to(DEV).eval().engine()
    assert Model(synth.make_config("T2", device=DEV, max_seq_len=498, beam_size=3)).to(DEV).eval().engine().supports_ragged_beam()
    # a context without the TFM decoder
    _, ma = engine_model("TS0", 12, 1234, 0.3, beam_size=3)
    assert not ma.engine().supports_ragged_beam()
    rc, msg = _raw(ma.engine(), packed, [8], 3)
    assert rc == D2T_ESTATE and "TFM decoder" in msg, (rc, msg)
    # d_model 512 (projected cross K / V, host-side beam loop): the entry refuses, Model serves the list tensor by tensor
    _, m = engine_model("T1", 12, 1234, 2.9, beam_size=4)
    eng = m.engine()
    assert not eng.supports_ragged_beam()
    rc, msg = _raw(eng, packed, [8, 9], 4)
    assert rc == D2T_ESTATE and "d_model 256" in msg and "d2t_decode_beam_batch" in msg, (rc, msg)
    imgs = [synth.synth_images(2, 32, 64, seed=701).cuda(), synth.synth_images(1, 32, 32, seed=703).cuda(),
            synth.synth_images(2, 32, 64, seed=705).cuda()]
    with torch.no_grad():
        want = [r for x in imgs for r in m.beam_search_batch(x)]
        got = m.beam_search_batch(imgs)
    _same(got, want, "T1 falls back")
    assert len(got) == 5
    # ... and so do the LSTM-attention heads
    imgs = [synth.synth_images(2, 48, 64, seed=711).cuda(), synth.synth_images(1, 48, 32, seed=712).cuda()]
    with torch.no_grad():
        want = [r for x in imgs for r in ma.beam_search_batch(x)]
        got = ma.beam_search_batch(imgs)
    assert len(got) == 3
    for (s1, v1), (s2, v2) in zip(got, want):
        assert torch.equal(s1, s2) and float(v1) == float(v2)
