"""GPU: the recurrent kernels (csrc/recurrent.hip, train_recurrent.hip, recurrent_common.h) ONE AT A TIME through the
d2t_op_* test entries, against references written in float64 from each operation's definition at the kernels' layouts
(tests/recurrent_refs.py, pinned to oracle.restatement by tests/test_recurrent_refs_cpu.py): the BiLSTM recurrence with its
training saves and backward, the LSTM-attention decoder loop (teacher-forced, greedy, step mode, early exit), its backward,
the finalize and alpha-gather kernels and the location-filter unfold.

Outputs are pre-filled with NaN (floats) / -1 (ints) and allocated with a guard tail: an element a kernel should have written
and did not fails, and so does a write behind the specified region.

Tolerances (none of them taken from the code under test):
  exact     integers, tokens, copies, zeroed ranges, gathers, and results that must not depend on the launch: bit for bit.
  measured  err = max |y - y64| <= 8 e32 + 1e-6 max |y64|, e32 = the largest max |y32 - y64| over three fp32 CPU
            evaluations of the same function on the same inputs: torch's own, every reduction axis reversed, every reduction
            split into 16 chunks summed left to right (one sequential evaluation does not sample the kernels' part-wise
            sums).  The factor 8 is the project's margin of DESIGN.md 5.3a.  The backward references are torch.autograd on
            the float64 forward (retain_grad on the pre-activation gates, the query projection, the embedding rows and the
            initial state), never a hand-derived formula.
  derived   loc_unfold_bwd, one dot product deep: (K + 4) 2^-24 sum |a| |b| with K = B + H, the longest chain.
  greedy    token feedback is compared exactly, on inputs whose float64 top-1 - top-2 logit margin at EVERY (row, step) is
            at least 100 * 8 e32 -- asserted on the reference before the kernel's result is looked at.
Every figure is printed (`FIG ...` lines, pytest -s) before it is asserted; DESIGN.md 5.5a has the table from an MI355X.

Shown to fail when the kernel is made subtly wrong (scratch builds, one mutation at a time, every address in range, each
build run once on an MI355X; the numbers are those of DESIGN.md 5.5a):
   1 argmax_better `i < bi` -> `i > bi`       -> all nine test_first_maximum_under_exact_ties cases
   2 WIDE cross-wave scan from w = 2          -> test_first_maximum_under_exact_ties[wide-waves] (the winner lives in wave 1),
                                                 test_attn_greedy_tokens_exact (V 1025)
   3 softmax loops bounded by min(Tk, 1024)   -> test_attn_forward_teacher_forced (Tk 1030, 4096), test_attn_greedy_tokens_exact (Tk 1030)
   4 `half + 1` handed to loc_term            -> test_attn_forward_teacher_forced (the seven cases with Tk > 1), ..._use_teacher_flags_and_dropmask,
                                                 all of test_attn_greedy_tokens_exact, test_step_mode_chain, test_early_exit
   5 coverage accumulation dropped            -> test_attn_forward_teacher_forced (the four coverage cases with Tk > 1), ..._flags_and_dropmask,
                                                 test_attn_greedy_tokens_exact (coverage), test_step_mode_chain, test_early_exit
   6 init_mode 1 mean divided by Tk           -> test_attn_forward_teacher_forced (the two key_off 1, init_mode 1 cases)
   7 kp not offset by key_off                 -> test_attn_forward_teacher_forced (the three key_off 1 cases with Tk > 1), test_step_mode_chain
   8 BiLSTM reverse direction reading t = step -> test_bilstm_vs_float64 (the ten cases with T > 1)
   9 BiLSTM backward cp at step >= 0          -> test_bilstm_vs_float64 (all fifteen: the first processed step of each direction)
  10 sum_parts<15> for dhprev                 -> all eight test_attn_lstm_bwd cases
  11 location-aware `dcov_s[j] +=`            -> test_attn_lstm_bwd (the three cases without coverage)
  12 acc_bs not accumulated                   -> NOT caught, and cannot be: dbscore is zero in exact arithmetic (see attn_bwd_ref),
                                                 the statement accumulates a rounding residue, and without it the kernel returns 0.0
  13 finalize `mx + 1u <= S`                  -> NOT caught: an equivalent mutant (mx + 1 == S gives steps = S either way)
  14 zero_words tail loop removed             -> test_finalize_alone (the seven cases whose cleared ranges end off a 16-byte boundary)
  15 alpha gather `(src & 3) == 0` -> `true`  -> NOT caught: a 16-byte global load from a 4-byte aligned address returns the same
                                                 data on gfx950; the branch is a performance choice without an observable effect
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import recurrent_refs as RR
from doc2tex_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = 1  # include/d2t.h D2T_EINVAL
U = 2.0 ** -24
NAN = float("nan")
H = 256
GUARD = 64
F64 = torch.float64


def _fig(name, **kv):
    print("FIG " + name + " " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _d(t):
    return None if t is None else t.contiguous().to(DEV)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Buf:
    """a device output of `shape` filled with a sentinel, with a guard tail behind it"""

    def __init__(self, *shape, dtype=torch.float32, fill=None):
        self.shape, self.n = shape, int(np.prod(shape))
        self.fill = fill if fill is not None else (NAN if dtype == torch.float32 else -1)
        self.t = torch.full((self.n + GUARD,), self.fill, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def untouched(self):
        c = self.t.cpu()
        return bool(torch.isnan(c).all()) if c.dtype == torch.float32 and self.fill != self.fill else bool((c == self.fill).all())

    def get(self):
        c = self.t.cpu()
        g = c[self.n:]
        ok = torch.isnan(g).all() if (g.dtype == torch.float32 and self.fill != self.fill) else (g == self.fill).all()
        assert ok, "a kernel wrote behind its output"
        return c[:self.n].view(*self.shape)


def _p(x):
    return None if x is None else (x.ptr if isinstance(x, Buf) else x.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rule(name, y, y64, e32, **kv):
    """the measured rule; returns err / e32"""
    assert not torch.isnan(y).any(), f"{name}: unwritten / NaN elements"
    err = float((y.double() - y64).abs().max())
    mx = float(y64.abs().max())
    ratio = err / e32 if e32 > 0 else 0.0
    _fig(name, e32=e32, err=err, ratio=ratio, max=mx, **kv)
    assert err <= 8.0 * e32 + 1e-6 * mx, f"{name}: |y - y64| = {err:.3e}, e32 = {e32:.3e}, max |y64| = {mx:.3e}"
    return ratio


# =====================================================================================================================
# BiLSTM
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def _bilstm_case(B, T, seed=0):
    g = _gen(100 + 31 * B + T + seed)
    gates = torch.randn(B, T, 8 * H, generator=g)
    whh_t = torch.randn(2, H, 4 * H, generator=g) * H ** -0.5
    dout = torch.randn(B, T, 2 * H, generator=g)

    def fwd(dt, mode):
        out, sg, sc = RR.bilstm_ref(gates.to(dt), whh_t.to(dt), mode)
        return dict(out=out, sv_gates=sg, sv_c=sc)

    def bwd(dt, mode):
        return RR.bilstm_bwd_ref(gates.to(dt), whh_t.to(dt), dout.to(dt), mode)
    y64, e32 = RR.e32_of(fwd)
    d64, de32 = RR.e32_of(bwd)
    return gates, whh_t, dout, y64, e32, d64, de32


def _bilstm_fwd(gates, whh_t, save, B=None, T=None, Hh=H):
    lib = _lib.require_device()
    Bq, Tq = gates.shape[0], gates.shape[1]
    B, T = (Bq if B is None else B), (Tq if T is None else T)
    gd, wd = _d(gates), _d(whh_t)
    out = Buf(Bq, Tq, 2 * H)
    sg, sc = (Buf(Bq, Tq, 8 * H), Buf(Bq, Tq, 2 * H)) if save else (None, None)
    rc = lib.d2t_op_bilstm(_p(gd), _p(wd), _p(out), _p(sg), _p(sc), B, T, Hh, _stream())
    torch.cuda.synchronize()
    return rc, out, sg, sc


def _bilstm_bwd(dout, sv_gates, sv_c, whh_t, B=None, T=None, Hh=H):
    lib = _lib.require_device()
    Bq, Tq = dout.shape[0], dout.shape[1]
    B, T = (Bq if B is None else B), (Tq if T is None else T)
    raw = whh_t.transpose(1, 2).contiguous()  # [2][4H][H] as stored
    dd, gd, cd, wf, wr = _d(dout), _d(sv_gates), _d(sv_c), _d(raw[0]), _d(raw[1])
    dg = Buf(Bq, Tq, 8 * H)
    rc = lib.d2t_op_bilstm_bwd(_p(dd), _p(gd), _p(cd), _p(wf), _p(wr), _p(dg), B, T, Hh, _stream())
    torch.cuda.synchronize()
    return rc, dg


@pytest.mark.parametrize("T", (1, 2, 7))
@pytest.mark.parametrize("B", (1, 3, 4, 5, 9))
def test_bilstm_vs_float64(B, T):
    """forward, forward with the training saves, and the backward fed once with the kernel's saves and once with the float64
    reference's rounded to fp32; blocks of 1-3 live rows and T = 1 (the backward's first-step branch) included"""
    gates, whh_t, dout, y64, e32, d64, de32 = _bilstm_case(B, T)
    rc, out, _, _ = _bilstm_fwd(gates, whh_t, save=False)
    assert rc == 0
    _rule("bilstm_out", out.get(), y64["out"], e32["out"], B=B, T=T)
    rc, out2, sg, sc = _bilstm_fwd(gates, whh_t, save=True)
    assert rc == 0
    _rule("bilstm_save_out", out2.get(), y64["out"], e32["out"], B=B, T=T)
    _rule("bilstm_sv_gates", sg.get(), y64["sv_gates"], e32["sv_gates"], B=B, T=T)
    _rule("bilstm_sv_c", sc.get(), y64["sv_c"], e32["sv_c"], B=B, T=T)
    for src, (svg, svc) in (("kernel", (sg.get(), sc.get())), ("ref", (y64["sv_gates"].float(), y64["sv_c"].float()))):
        rc, dg = _bilstm_bwd(dout, svg, svc, whh_t)
        assert rc == 0
        _rule("bilstm_dgates_" + src, dg.get().view(B, T, 8 * H), d64, de32, B=B, T=T)


def test_bilstm_partial_block():
    """rows of a partly filled block: B = 5 equals rows 0-4 of B = 8 bit for bit, forward, saves and backward"""
    gates, whh_t, dout, *_ = _bilstm_case(8, 7)
    rc8, o8, g8, c8 = _bilstm_fwd(gates, whh_t, save=True)
    rc5, o5, g5, c5 = _bilstm_fwd(gates[:5], whh_t, save=True)
    assert rc8 == 0 and rc5 == 0
    for a, b in ((o5, o8), (g5, g8), (c5, c8)):
        assert not torch.isnan(a.get()).any() and not torch.isnan(b.get()).any()
        assert _same(a.get(), b.get()[:5])
    rc8, d8 = _bilstm_bwd(dout, g8.get(), c8.get(), whh_t)
    rc5, d5 = _bilstm_bwd(dout[:5], g5.get(), c5.get(), whh_t)
    assert rc8 == 0 and rc5 == 0
    assert not torch.isnan(d5.get()).any() and not torch.isnan(d8.get()).any()
    assert _same(d5.get(), d8.get()[:5])
    rcn, on, _, _ = _bilstm_fwd(gates[:5], whh_t, save=False)
    assert rcn == 0 and not torch.isnan(on.get()).any()


@pytest.mark.parametrize("B,T", [(1, 1), (3, 7), (5, 2), (2, 1)])
def test_bilstm_hprev_exact(B, T):
    lib = _lib.require_device()
    out = torch.randn(B, T, 2 * H, generator=_gen(B * 10 + T))
    od = _d(out)
    hf, hr = Buf(B * T, H), Buf(B * T, H)
    assert lib.d2t_op_bilstm_hprev(_p(od), _p(hf), _p(hr), B, T, H, _stream()) == 0
    torch.cuda.synchronize()
    rf, rr = RR.bilstm_hprev_ref(out)
    assert _same(hf.get().view(B, T, H), rf) and _same(hr.get().view(B, T, H), rr)


def test_bilstm_refusals():
    gates, whh_t, dout, y64, *_ = _bilstm_case(3, 2)
    svg, svc = y64["sv_gates"].float(), y64["sv_c"].float()
    lib = _lib.require_device()
    for B, T, Hh in ((3, 2, 128), (3, 2, 512), (0, 2, H), (-1, 2, H), (3, 0, H)):
        for save in (False, True):
            rc, out, sg, sc = _bilstm_fwd(gates, whh_t, save, B=B, T=T, Hh=Hh)
            assert rc == EINVAL and out.untouched() and (sg is None or (sg.untouched() and sc.untouched()))
        rc, dg = _bilstm_bwd(dout, svg, svc, whh_t, B=B, T=T, Hh=Hh)
        assert rc == EINVAL and dg.untouched()
    od = _d(y64["out"].float())
    hf, hr = Buf(6, H), Buf(6, H)
    for B, T, Hh in ((0, 2, H), (3, 0, H), (3, 2, 0)):
        assert lib.d2t_op_bilstm_hprev(_p(od), _p(hf), _p(hr), B, T, Hh, _stream()) == EINVAL
    assert lib.d2t_op_bilstm_hprev(None, _p(hf), _p(hr), 3, 2, H, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert hf.untouched() and hr.untouched()
    gd, wd = _d(gates), _d(whh_t)
    out, sg = Buf(3, 2, 2 * H), Buf(3, 2, 8 * H)
    assert lib.d2t_op_bilstm(_p(gd), _p(wd), _p(out), _p(sg), None, 3, 2, H, _stream()) == EINVAL  # one save buffer only
    assert lib.d2t_op_bilstm(None, _p(wd), _p(out), None, None, 3, 2, H, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert out.untouched() and sg.untouched()


# =====================================================================================================================
# LSTM-attention decoder loop: the launch
# =====================================================================================================================
_W_KEYS = ("wq_t", "bq", "wloc", "bloc", "wscore", "wx_t", "bx", "wg_t", "bg", "wih_t", "bih", "wic_t", "bic", "emb", "tokgate")


def _inputs(N, T, V, taps, seed, tokgate=False):
    """weights, memory N(0, 1) and its key projection (float64 product rounded to fp32: an INPUT of the kernel)"""
    W = RR.attn_weights(V, taps, seed, tokgate=tokgate)
    mem = torch.randn(N, T, H, generator=_gen(seed + 7))
    kp = (mem.double() @ W["wk"].double().t() + W["bk"].double()).float()
    return W, mem, kp


def _decode(W, mem, kp, S, *, B=None, key_off=0, init_mode=0, coverage=True, end_token=1, teacher=None, use_teacher=None,
            dropmask=None, dropscale=1.0, save=False, alpha=False, step=None, exit_word=False, over=None):
    """one d2t_op_attn_decode call; returns rc and a dict of the outputs (CPU).  step = dict(first, rows, state, tok_in);
    over: struct fields overridden last (refusal tests)."""
    lib = _lib.require_device()
    N, T, _ = mem.shape
    B = (len(step["rows"]) if step and step.get("rows") is not None else (step["B"] if step else N)) if B is None else B
    V, taps, Tk = W["wg_t"].shape[1], W["wloc"].shape[1], T - key_off
    keep = [_d(mem), _d(kp)]
    a = _lib.D2TOpAttnDecodeArgs()
    a.mem, a.kp = keep[0].data_ptr(), keep[1].data_ptr()
    for k in _W_KEYS:
        if k in W:
            keep.append(_d(W[k]))
            setattr(a, k, keep[-1].data_ptr())
    o = dict(probs=Buf(B, S, V), tokens=Buf(B, S, dtype=torch.int64), end_step=Buf(B, dtype=torch.int32, fill=-7))
    if save:
        o.update(sv_hprev=Buf(B, S, H), sv_cprev=Buf(B, S, H), sv_hafter=Buf(B, S, H), sv_cafter=Buf(B, S, H),
                 sv_gates=Buf(B, S, 4 * H), sv_hq=Buf(B, S, H), sv_x=Buf(B, S, 2 * H))
        if teacher is not None:
            o["sv_tok"] = Buf(B, S, dtype=torch.int64)
    if save or alpha:
        o["sv_alpha"] = Buf(B, S, Tk)
    if teacher is not None:
        keep.append(_d(teacher.to(torch.int64)))
        a.teacher = keep[-1].data_ptr()
    if use_teacher is not None:
        keep.append(_d(torch.as_tensor(use_teacher, dtype=torch.uint8)))
        a.use_teacher = keep[-1].data_ptr()
    if dropmask is not None:
        keep.append(_d(dropmask.to(torch.uint8)))
        a.out_dropmask = keep[-1].data_ptr()
    a.samples = N
    if step:
        a.step_mode, a.first = 1, int(step["first"])
        o.update(st_h_out=Buf(B, H), st_c_out=Buf(B, H), st_mem_out=Buf(B, Tk))
        if step.get("rows") is not None:
            keep.append(_d(torch.as_tensor(step["rows"], dtype=torch.int32)))
            a.row_sample = keep[-1].data_ptr()
        if not step["first"]:
            for k, v in zip(("st_h_in", "st_c_in", "st_mem_in"), step["state"]):
                keep.append(_d(v))
                setattr(a, k, keep[-1].data_ptr())
            keep.append(_d(step["tok_in"].to(torch.int64)))
            a.tok_in = keep[-1].data_ptr()
    if exit_word:
        o["exit_state"] = Buf(1, dtype=torch.int64, fill=-1)
        o["steps_dev"] = Buf(1, dtype=torch.int32)
    for k, b in o.items():
        setattr(a, k, b.ptr)
    a.bscore, a.out_dropscale = float(W["bscore"]), float(dropscale)
    a.B, a.T, a.S, a.V, a.taps, a.key_off, a.init_mode = B, T, S, V, taps, key_off, init_mode
    a.coverage, a.end_token = int(coverage), end_token
    for k, v in (over or {}).items():
        setattr(a, k, v)
    rc = lib.d2t_op_attn_decode(C.byref(a), _stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, o
    return rc, {k: b.get() for k, b in o.items()}


_SV = dict(sv_hprev="hprev", sv_cprev="cprev", sv_hafter="hafter", sv_cafter="cafter", sv_gates="gates", sv_alpha="alpha",
           sv_hq="hq", sv_x="x")


def _ref_e32(W, mem, kp, S, **kw):
    def fn(dt, mode):
        return RR.attn_ref(RR.cast(W, dt), mem.to(dt), kp.to(dt), S, mode=mode, **kw)
    keys = ["probs", "mem"] + list(_SV.values())
    return RR.e32_of(fn, keys)


def _check_values(name, got, y64, e32, **kv):
    worst = _rule(name + "_probs", got["probs"], y64["probs"], e32["probs"], **kv)
    for k, r in _SV.items():
        if k in got:
            worst = max(worst, _rule(f"{name}_{k}", got[k], y64[r], e32[r], **kv))
    return worst


def _margin_ok(name, y64, e32):
    """the greedy condition, on the reference: top-1 - top-2 >= 100 * 8 e32 at every (row, step)"""
    top = y64["probs"].topk(2, -1).values
    margin = float((top[..., 0] - top[..., 1]).min())
    _fig(name + "_margin", margin=margin, need=800.0 * e32["probs"])
    assert margin >= 800.0 * e32["probs"], f"{name}: pick another seed (margin {margin:.3e}, e32 {e32['probs']:.3e})"


# (B, T, S, V, taps, coverage, key_off, init_mode, tokgate)
TEACHER_CASES = [
    (3, 5, 6, 37, 11, 1, 0, 0, False),      # Tk < taps
    (2, 1030, 4, 37, 3, 0, 0, 1, False),    # the 1024-strided loops go round twice; location-aware memory
    (2, 4096, 3, 37, 3, 1, 0, 2, False),    # the longest memory
    (3, 1, 5, 1024, 1, 1, 0, 0, False),     # Tk = 1, one tap, the last narrow vocabulary
    (3, 18, 6, 1025, 11, 0, 1, 1, False),   # key_off 1 with the mean over all T tokens; the first WIDE vocabulary
    (3, 6, 6, 2500, 3, 1, 1, 2, True),      # one-hot targets (tokgate)
    (2, 17, 8, 37, 11, 1, 1, 0, True),
    (2, 2, 4, 37, 11, 0, 1, 1, False),      # Tk = 1 behind the dropped token
    (3, 17, 6, 1024, 1, 0, 0, 2, False),
]


@pytest.mark.parametrize("B,T,S,V,taps,cov,key_off,init_mode,tokgate", TEACHER_CASES)
def test_attn_forward_teacher_forced(B, T, S, V, taps, cov, key_off, init_mode, tokgate):
    """probs and every sv_* of the training forward; teacher-forced, so no token flip can fork the sequence"""
    W, mem, kp = _inputs(B, T, V, taps, seed=11 + T + V + taps, tokgate=tokgate)
    teacher = torch.randint(0, V, (B, S), generator=_gen(T + V))
    kw = dict(key_off=key_off, init_mode=init_mode, coverage=bool(cov), teacher=teacher)
    y64, e32 = _ref_e32(W, mem, kp, S, **kw)
    rc, got = _decode(W, mem, kp, S, save=True, **kw)
    assert rc == 0
    assert torch.equal(got["sv_tok"], teacher)
    _check_values("attn_tf", got, y64, e32, Tk=T - key_off, V=V, taps=taps, cov=cov, init=init_mode, tokgate=int(tokgate))


def test_attn_use_teacher_flags_and_dropmask():
    """use_teacher with zeros (scheduled sampling: the step's input is the previous argmax), under the margin condition; then
    out_dropmask with a fixed random keep mask"""
    B, T, S, V, taps = 3, 17, 8, 37, 11
    W, mem, kp = _inputs(B, T, V, taps, seed=1)
    teacher = torch.randint(0, V, (B, S), generator=_gen(3))
    flags = [1, 0, 1, 0, 0, 1, 1, 0]
    kw = dict(coverage=True, teacher=teacher, use_teacher=flags)
    y64, e32 = _ref_e32(W, mem, kp, S, **kw)
    _margin_ok("attn_flags", y64, e32)
    rc, got = _decode(W, mem, kp, S, save=True, **kw)
    assert rc == 0
    assert torch.equal(got["tokens"], y64["tokens"]) and torch.equal(got["sv_tok"], y64["tok"])
    assert torch.equal(got["end_step"], y64["end_step"])
    _check_values("attn_flags", got, y64, e32)
    mask = torch.rand(B, S, V, generator=_gen(4)) >= 0.3
    kw = dict(coverage=True, teacher=teacher, dropmask=mask, dropscale=1.0 / 0.7)
    y64, e32 = _ref_e32(W, mem, kp, S, **kw)
    rc, got = _decode(W, mem, kp, S, save=True, **kw)
    assert rc == 0
    assert bool((got["probs"][~mask] == 0).all())
    _check_values("attn_dropmask", got, y64, e32)


# (B, T, S, V, taps, coverage, seed)
GREEDY_CASES = [(3, 17, 8, 37, 11, 1, 4), (3, 5, 8, 2500, 11, 1, 5), (2, 1030, 6, 1025, 3, 0, 3)]


@pytest.mark.parametrize("B,T,S,V,taps,cov,seed", GREEDY_CASES)
def test_attn_greedy_tokens_exact(B, T, S, V, taps, cov, seed):
    """greedy feedback: tokens and end_step exact under the margin condition, values by the measured rule; no row or step left out"""
    W, mem, kp = _inputs(B, T, V, taps, seed=seed)
    y64, e32 = _ref_e32(W, mem, kp, S, coverage=bool(cov))
    _margin_ok("attn_greedy", y64, e32)
    rc, got = _decode(W, mem, kp, S, coverage=bool(cov), alpha=True)
    assert rc == 0
    assert torch.equal(got["tokens"], y64["tokens"])
    assert torch.equal(got["end_step"], y64["end_step"])
    _check_values("attn_greedy", got, y64, e32, V=V, Tk=T)


# narrow build (one class per thread, wave 0 scans i = lane, lane + 64, ...): the same lane of the scan, different lanes, beyond 64;
# WIDE build (thread tid takes tid, tid + 1024, ...): the same thread, different lanes of one wave, different waves
TIE_CASES = [("narrow-same-lane", 200, 5, 69), ("narrow-lanes", 200, 3, 9), ("narrow-beyond-64", 200, 100, 165),
             ("narrow-two-rounds", 200, 70, 198), ("wide-same-thread", 2500, 7, 1031), ("wide-lanes", 2500, 130, 150),
             ("wide-waves", 2500, 70, 700), ("wide-waves-second-round", 2500, 1500, 2300), ("wide-wave0-wave1", 2500, 63, 64)]


@pytest.mark.parametrize("name,V,lo,hi", TIE_CASES)
def test_first_maximum_under_exact_ties(name, V, lo, hi):
    """generator columns and biases duplicated at (lo, hi) and raised above the rest: identical weights summed by the same
    thread sequence give bit-identical logits, and the lower index must win at every (row, step)"""
    B, T, S, taps = 2, 5, 4, 3
    W, mem, kp = _inputs(B, T, V, taps, seed=5)
    W["wg_t"][:, hi] = W["wg_t"][:, lo]
    W["bg"][lo] = W["bg"][hi] = 40.0
    rc, got = _decode(W, mem, kp, S)
    assert rc == 0
    assert _same(got["probs"][:, :, lo], got["probs"][:, :, hi]), "the tie is not exact: the test's premise fails"
    assert bool((got["probs"].argmax(-1) == lo).all()), "the duplicated pair is not the maximum: the test's premise fails"
    assert bool((got["tokens"] == lo).all()), f"{name}: tokens {got['tokens'].tolist()}, expected {lo} everywhere"


@pytest.mark.parametrize("with_map", (True, False))
def test_step_mode_chain(with_map):
    """S = 1 launches chained through st_*_out -> st_*_in: equal bit for bit to steps 0-2 of the loop on the same rows fed the
    same tokens, and within the measured rule of the float64 reference.  6 hypothesis rows over 2 samples (row_sample), or all
    on sample 0 (no map)."""
    T, V, taps, key_off = 19, 37, 11, 1
    W, mem, kp = _inputs(2, T, V, taps, seed=21)
    rows = [0, 1, 0, 1, 1, 0] if with_map else [0] * 6
    fed = torch.randint(0, V, (6, 3), generator=_gen(8))
    fed[:, 0] = 0  # [GO]: what a first step starts from
    kw = dict(key_off=key_off, init_mode=2, coverage=True)
    def fn(dt, mode):  # every step's outputs under their own keys: e32 is measured per step
        r = RR.attn_ref(RR.cast(W, dt), mem.to(dt), kp.to(dt), 3, rows=rows, teacher=fed, mode=mode, **kw)
        return {f"{k}{s}": r[k][:, s] for k in ("probs", "hafter", "cafter", "mem") for s in range(3)}
    y64, e32 = RR.e32_of(fn)
    rc, loop = _decode(W, mem[rows], kp[rows], 3, teacher=fed, save=True, **kw)
    assert rc == 0
    state = None
    m32 = torch.zeros(6, T - key_off)
    for s in range(3):
        st = dict(first=s == 0, rows=rows if with_map else None, B=6, state=state, tok_in=fed[:, s])
        rc, got = _decode(W, mem, kp, 1, alpha=True, step=st, **kw)
        assert rc == 0
        m32 = m32 + loop["sv_alpha"][:, s]  # the coverage memory: fp32 adds in step order
        for a, b in ((got["probs"][:, 0], loop["probs"][:, s]), (got["tokens"][:, 0], loop["tokens"][:, s]),
                     (got["sv_alpha"][:, 0], loop["sv_alpha"][:, s]), (got["st_h_out"], loop["sv_hafter"][:, s]),
                     (got["st_c_out"], loop["sv_cafter"][:, s]), (got["st_mem_out"], m32)):
            assert _same(a, b), f"step {s}: step mode differs from the loop"
        _rule("attn_step_probs", got["probs"][:, 0], y64[f"probs{s}"], e32[f"probs{s}"], step=s)
        _rule("attn_step_h", got["st_h_out"], y64[f"hafter{s}"], e32[f"hafter{s}"], step=s)
        _rule("attn_step_c", got["st_c_out"], y64[f"cafter{s}"], e32[f"cafter{s}"], step=s)
        _rule("attn_step_mem", got["st_mem_out"], y64[f"mem{s}"], e32[f"mem{s}"], step=s)
        state = (got["st_h_out"], got["st_c_out"], got["st_mem_out"])


def _exit_inputs(want_all_end):
    """V = 5 inputs and an end token for which, IN THE FLOAT64 REFERENCE, every row ends before S - 2 (or one row never does),
    with the margin condition; chosen from the reference alone"""
    B, T, S, V, taps = 3, 9, 8, 5, 3
    for seed in range(40, 60):
        W, mem, kp = _inputs(B, T, V, taps, seed=seed)
        y64, e32 = _ref_e32(W, mem, kp, S, coverage=True)
        top = y64["probs"].topk(2, -1).values
        if float((top[..., 0] - top[..., 1]).min()) < 800.0 * e32["probs"]:
            continue
        for end in range(V):
            ends = [(y64["tokens"][b] == end).nonzero() for b in range(B)]
            first = [int(e[0]) if len(e) else -1 for e in ends]
            if want_all_end and min(first) >= 0 and max(first) < S - 2 and len(set(first)) > 1:
                return W, mem, kp, S, end, y64, e32, first
            if not want_all_end and min(first) < 0 <= max(first):
                return W, mem, kp, S, end, y64, e32, first
    raise AssertionError("no seed meets the condition: extend the seed range")


@pytest.mark.parametrize("all_end", (True, False))
def test_early_exit(all_end):
    """the build with an exit word against the build without: the same on [0, steps), zeros behind; how far single blocks ran
    past the exit does not show.  Second case: one row never ends -> steps = S, nothing cleared."""
    W, mem, kp, S, end, y64, e32, first = _exit_inputs(all_end)
    _margin_ok("attn_exit", y64, e32)
    steps = max(first) + 1 if all_end else S
    assert (steps < S - 1) if all_end else (min(first) < 0)
    rc, full = _decode(W, mem, kp, S, end_token=end, alpha=True)
    rc2, ex = _decode(W, mem, kp, S, end_token=end, alpha=True, exit_word=True)
    assert rc == 0 and rc2 == 0
    assert int(ex["steps_dev"][0]) == steps
    assert torch.equal(full["tokens"], y64["tokens"])
    assert ex["end_step"].tolist() == first and full["end_step"].tolist() == first
    for k in ("tokens", "probs", "sv_alpha"):
        assert _same(ex[k][:, :steps], full[k][:, :steps]), k
        assert bool((_bits(ex[k][:, steps:]) == 0).all()), f"{k}: not cleared behind the exit"
    _rule("attn_exit_probs", ex["probs"][:, :steps], y64["probs"][:, :steps], e32["probs"], steps=steps)


def test_attn_decode_refusals():
    """arguments the launcher refuses or that would index out of range: D2T_EINVAL and nothing written"""
    B, T, S, V, taps = 2, 5, 3, 37, 3
    W, mem, kp = _inputs(B, T, V, taps, seed=2)
    teacher = torch.randint(0, V, (B, S), generator=_gen(1))
    bad_teacher = teacher.clone()
    bad_teacher[1, 2] = V
    neg_teacher = teacher.clone()
    neg_teacher[0, 0] = -1
    st = torch.zeros(B, H), torch.zeros(B, H), torch.zeros(B, T)
    cases = [dict(teacher=bad_teacher), dict(teacher=neg_teacher), dict(over=dict(T=4097)), dict(over=dict(taps=12)),
             dict(over=dict(taps=0)), dict(over=dict(V=16385)), dict(over=dict(B=0)), dict(over=dict(S=0)), dict(key_off=1, over=dict(T=1)),
             dict(over=dict(end_token=V)), dict(over=dict(init_mode=3)), dict(init_mode=1, over=dict(wih_t=None)),
             dict(over=dict(emb=None)), dict(over=dict(mem=None)), dict(over=dict(probs=None)), dict(over=dict(samples=3)),
             dict(teacher=teacher, exit_word=True), dict(use_teacher=[1, 1, 1]),
             dict(step=dict(first=True, rows=[0, 2], B=2)), dict(step=dict(first=True, rows=[0, -1], B=2)),
             dict(step=dict(first=False, rows=[0, 1], B=2, state=st, tok_in=torch.tensor([0, V]))),
             dict(step=dict(first=False, rows=None, B=2, state=st, tok_in=torch.tensor([-1, 0]))),
             dict(step=dict(first=True, rows=None, B=2), over=dict(S=2)),
             dict(step=dict(first=False, rows=None, B=2, state=st, tok_in=torch.tensor([0, 0])), over=dict(st_mem_in=None))]
    for kw in cases:
        rc, o = _decode(W, mem, kp, 1 if "step" in kw else S, **kw)
        assert rc == EINVAL, kw
        assert all(b.untouched() for b in o.values()), kw


# =====================================================================================================================
# finalize alone, alpha gather
# =====================================================================================================================
FINALIZE_CASES = [  # (B, S, V, Tk, count (None = B), mx, with alpha)
    (1, 7, 37, 5, None, 2, True), (3, 7, 37, 5, None, 2, True), (300, 7, 37, 5, None, 0, True), (3, 7, 37, 5, None, 4, False),
    (3, 7, 37, 5, None, 6, True), (3, 7, 37, 5, None, 5, True), (3, 7, 37, 5, 2, 2, True), (300, 7, 37, 5, 299, 2, True),
    (3, 8, 64, 16, None, 3, True), (300, 5, 3, 1, None, 1, True), (3, 7, 37, 5, None, 7, True), (2, 6, 1025, 1030, None, 2, True)]


@pytest.mark.parametrize("B,S,V,Tk,count,mx,with_alpha", FINALIZE_CASES)
def test_finalize_alone(B, S, V, Tk, count, mx, with_alpha):
    """exit words built by hand on sentinel-filled buffers: steps and the cleared ranges exact, everything else untouched
    (unaligned heads and tails of the 16-byte clears at odd V / Tk / steps; B > 256 rows stride over gridDim.y)"""
    lib = _lib.require_device()
    count = B if count is None else count
    word = _d(torch.tensor([(count << 32) | mx], dtype=torch.int64))
    steps_dev = Buf(1, dtype=torch.int32)
    tokens, probs = Buf(B, S, dtype=torch.int64), Buf(B, S, V)
    alpha = Buf(B, S, Tk) if with_alpha else None
    rc = lib.d2t_op_attn_decode_finalize(_p(word), _p(steps_dev), B, S, V, Tk, _p(tokens), _p(probs), _p(alpha), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    steps = mx + 1 if (count == B and mx + 1 < S) else S
    assert int(steps_dev.get()[0]) == steps
    for buf in (tokens, probs, alpha):
        if buf is None:
            continue
        got = buf.get()
        want = torch.full_like(got, buf.fill)
        want[:, steps:] = 0
        assert _same(got, want)


def test_finalize_refusals():
    lib = _lib.require_device()
    word = _d(torch.tensor([(3 << 32) | 1], dtype=torch.int64))
    sd, tokens, probs = Buf(1, dtype=torch.int32), Buf(3, 7, dtype=torch.int64), Buf(3, 7, 37)
    ok = [_p(word), _p(sd), 3, 7, 37, 5, _p(tokens), _p(probs), None]
    for i, v in ((0, None), (1, None), (6, None), (7, None), (2, 0), (3, 0), (4, 0), (5, 0), (2, -1)):
        a = list(ok)
        a[i] = v
        assert lib.d2t_op_attn_decode_finalize(*a, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert sd.untouched() and tokens.untouched() and probs.untouched()


def _gather_call(hist, path, length, N, S, cap, Tk, out_off=0, hist_off=0):
    lib = _lib.require_device()
    hbuf = torch.zeros(hist.numel() + 4)
    hbuf[hist_off:hist_off + hist.numel()] = hist.flatten()
    hd, pd, ld = _d(hbuf), _d(path.to(torch.int32)), _d(length.to(torch.int32))
    out = Buf(N, S, Tk)
    rc = lib.d2t_op_attn_alpha_gather(hd.data_ptr() + 4 * hist_off, _p(pd), _p(ld), out.ptr + 4 * out_off, N, S, cap, Tk, _stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("N,S,cap,Tk", [(3, 5, 4, 1), (2, 4, 7, 3), (3, 3, 5, 4), (5, 6, 9, 7), (2, 8, 6, 64), (3, 3, 5, 7), (1, 1, 1, 3),
                                        (4, 5, 3, 1030)])
def test_alpha_gather_exact(N, S, cap, Tk):
    """chunks that straddle rows, unaligned sources, numel % 4 tails; len of 0, partial and S; paths to the last cap row"""
    g = _gen(N * 100 + S * 10 + Tk)
    hist = torch.randn(S, cap, Tk, generator=g)
    path = torch.randint(0, cap, (N, S), generator=g)
    path[0, :] = cap - 1
    length = torch.randint(0, S + 1, (N,), generator=g)
    length[0] = S
    if N > 1:
        length[1] = 0
    if N > 2:
        length[2] = max(1, S // 2)
    path[length[:, None] <= torch.arange(S)[None, :]] = -5  # entries behind len are never read
    rc, out = _gather_call(hist, path, length, N, S, cap, Tk)
    assert rc == 0
    want = torch.zeros(N, S, Tk)
    for i in range(N):
        for j in range(int(length[i])):
            want[i, j] = hist[j, path[i, j]]
    assert _same(out.get(), want)


def test_alpha_gather_from_a_4_byte_aligned_history():
    """only `out` needs 16 bytes: a history whose base is offset by 4 bytes is gathered exactly as well"""
    N, S, cap, Tk = 3, 4, 5, 8
    g = _gen(77)
    hist = torch.randn(S, cap, Tk, generator=g)
    path = torch.randint(0, cap, (N, S), generator=g)
    length = torch.tensor([S, 2, 0])
    rc, out = _gather_call(hist, path, length, N, S, cap, Tk, hist_off=1)
    assert rc == 0
    want = torch.zeros(N, S, Tk)
    for i in range(N):
        for j in range(int(length[i])):
            want[i, j] = hist[j, path[i, j]]
    assert _same(out.get(), want)


def test_alpha_gather_refusals():
    N, S, cap, Tk = 2, 4, 3, 5
    hist = torch.randn(S, cap, Tk, generator=_gen(1))
    path, length = torch.zeros(N, S, dtype=torch.int64), torch.tensor([S, 2])
    rc, out = _gather_call(hist, path, length, N, S, cap, Tk, out_off=1)  # a base pointer offset by 4 bytes
    assert rc == EINVAL and out.untouched()
    for p, ln in ((path + cap, length), (path - 1, length), (path, torch.tensor([S + 1, 0])), (path, torch.tensor([-1, 0]))):
        rc, out = _gather_call(hist, p, ln, N, S, cap, Tk)
        assert rc == EINVAL and out.untouched()
    for dims in ((0, S, cap, Tk), (N, 0, cap, Tk), (N, S, 0, Tk), (N, S, cap, 0)):
        rc, out = _gather_call(hist, path, length, *dims)
        assert rc == EINVAL and out.untouched()


# =====================================================================================================================
# LSTM-attention backward
# =====================================================================================================================
_BWD_OUT = ("dgates", "dhq", "demb", "dh0", "dc0", "dmem", "dkp", "dwloc", "dbloc", "dwscore", "dbscore")


def _lstm_bwd(W, mem, kp, dlogits, sv, S, *, key_off, coverage, with_demb, dhl=None, over=None):
    lib = _lib.require_device()
    B, T, _ = mem.shape
    V, taps = W["wg_t"].shape[1], W["wloc"].shape[1]
    a = _lib.D2TOpAttnLstmBwdArgs()
    wih_raw = W["wx_t"][:2 * H].t().contiguous()  # [4H][D + E] as stored
    whh_raw = W["wx_t"][2 * H:].t().contiguous()
    src = dict(dlogits=dlogits, mem=mem, kp=kp, wg_t=W["wg_t"], wih_raw=wih_raw, whh_raw=whh_raw, wq_raw=W["wq_t"].t().contiguous(),
               wloc=W["wloc"], bloc=W["bloc"], wscore=W["wscore"], sv_cprev=sv["cprev"], sv_cafter=sv["cafter"], sv_gates=sv["gates"],
               sv_alpha=sv["alpha"], sv_hq=sv["hq"], dhl=dhl)
    keep = {k: _d(v.float()) for k, v in src.items() if v is not None}
    for k, v in keep.items():
        setattr(a, k, v.data_ptr())
    o = dict(dmem=Buf(B, T, H), dkp=Buf(B, T, H), dgates=Buf(B, S, 4 * H), dhq=Buf(B, S, H), dh0=Buf(B, H), dc0=Buf(B, H),
             dwloc=Buf(B, H, taps), dbloc=Buf(B, H), dwscore=Buf(B, H), dbscore=Buf(B))
    if with_demb:
        o["demb"] = Buf(B, S, H)
    for k, b in o.items():
        setattr(a, k, b.ptr)
    a.B, a.T, a.S, a.V, a.taps, a.key_off, a.coverage = B, T, S, V, taps, key_off, int(coverage)
    for k, v in (over or {}).items():
        setattr(a, k, v)
    rc = lib.d2t_op_attn_lstm_bwd(C.byref(a), _stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, o
    return rc, {k: b.get() for k, b in o.items()}


# (T, S, V, taps, coverage, key_off, with demb, with dhl)
BWD_CASES = [
    (5, 6, 37, 11, 1, 0, True, False), (5, 6, 37, 11, 1, 0, True, True), (18, 6, 37, 1, 0, 1, False, False),
    (1030, 3, 37, 11, 0, 0, True, True), (2, 5, 2500, 1, 1, 1, False, True), (1031, 3, 37, 1, 1, 1, False, False),
    (17, 6, 2500, 11, 0, 0, True, True), (1, 4, 37, 11, 1, 0, True, False)]


@pytest.mark.parametrize("T,S,V,taps,cov,key_off,with_demb,with_dhl", BWD_CASES)
def test_attn_lstm_bwd(T, S, V, taps, cov, key_off, with_demb, with_dhl):
    """every output of the backward kernel against torch.autograd on the float64 forward, one row at a time for the per-row
    partials; saved tensors once the kernel forward's own (the end-to-end pair) and once the float64 reference's rounded"""
    B = 3
    W, mem, kp = _inputs(B, T, V, taps, seed=31 + taps + key_off)  # the same inputs for the dhl / in-kernel pair
    g = _gen(T + S)
    teacher = torch.randint(0, V, (B, S), generator=g)
    dlogits = torch.randn(B, S, V, generator=g) * 0.1
    kw = dict(key_off=key_off, coverage=bool(cov))

    def fn(dt, mode):
        return RR.attn_bwd_ref(RR.cast(W, dt), mem.to(dt), kp.to(dt), teacher, dlogits.to(dt), mode=mode, **kw)
    d64, e32 = RR.e32_of(fn)
    # the score bias' gradient is zero in exact arithmetic; its fp32 residue depends on the association of the sum, and the
    # kernel's (steps first within a thread, keys across threads afterwards) is one autograd does not take: see attn_bwd_ref
    e32["dbscore"] = max(e32["dbscore"], e32["dbscore_steps_first"])
    f64 = RR.attn_ref(RR.cast(W, F64), mem.double(), kp.double(), S, teacher=teacher, **kw)
    rc, fwd = _decode(W, mem, kp, S, teacher=teacher, save=True, **kw)
    assert rc == 0
    dhl = (dlogits.double() @ W["wg_t"].double().t()).float() if with_dhl else None
    w_emb = W["wx_t"][H:2 * H].double()  # [E][4H]: demb = dgates . W_ih[:, D:]
    if key_off:
        assert float(d64["dmem"][:, 0].abs().max()) == 0.0 and float(d64["dkp"][:, 0].abs().max()) == 0.0
    for src, sv in (("kernel", {v: fwd[k] for k, v in _SV.items()}), ("ref", f64)):
        rc, got = _lstm_bwd(W, mem, kp, dlogits, sv, S, with_demb=with_demb, dhl=dhl, **kw)
        assert rc == 0
        if not with_demb:  # the caller's GEMM on the saved dgates, in float64
            got["demb"] = (got["dgates"].double() @ w_emb.t()).float()
        if key_off:  # the dropped token's rows stay zero
            assert bool((got["dmem"][:, 0] == 0).all()) and bool((got["dkp"][:, 0] == 0).all())
        for k in _BWD_OUT:
            _rule(f"attn_bwd_{src}_{k}", got[k], d64[k], e32[k], Tk=T - key_off, V=V, taps=taps, cov=cov, demb=int(with_demb),
                  dhl=int(with_dhl))


def test_attn_lstm_bwd_refusals():
    B, T, S, V, taps = 3, 5, 3, 2500, 3
    W, mem, kp = _inputs(B, T, V, taps, seed=2)
    teacher = torch.randint(0, V, (B, S), generator=_gen(1))
    f64 = RR.attn_ref(RR.cast(W, F64), mem.double(), kp.double(), S, teacher=teacher)
    dlogits = torch.zeros(B, S, V)
    dhl = torch.zeros(B, S, H)
    cases = [dict(), dict(dhl=dhl, over=dict(T=4097)), dict(dhl=dhl, over=dict(taps=12)), dict(dhl=dhl, over=dict(B=0)),
             dict(dhl=dhl, over=dict(V=16385)), dict(dhl=dhl, over=dict(dmem=None)), dict(dhl=dhl, over=dict(sv_alpha=None)),
             dict(dhl=dhl, key_off=1, over=dict(T=1))]
    for c in cases:
        kw = dict(key_off=0, coverage=True, with_demb=True)
        kw.update(c)
        rc, o = _lstm_bwd(W, mem, kp, dlogits, f64, S, **kw)  # the first: V = 2500 without dhl
        assert rc == EINVAL, c
        assert all(b.untouched() for b in o.values()), c


# =====================================================================================================================
# location filter unfold
# =====================================================================================================================
@pytest.mark.parametrize("B", (1, 5))
@pytest.mark.parametrize("taps", (1, 3, 11))
@pytest.mark.parametrize("kd", (1, 16, 100))
def test_loc_unfold_bwd(kd, taps, B):
    """against autograd through wloc = Wp Wc, bloc = bp + Wp bc in float64, under the derived one-dot-product bound"""
    lib = _lib.require_device()
    g = _gen(kd * 100 + taps * 10 + B)
    cw, cb, pw = torch.randn(kd, taps, generator=g), torch.randn(kd, generator=g), torch.randn(H, kd, generator=g) * kd ** -0.5
    dwloc, dbloc = torch.randn(B, H, taps, generator=g), torch.randn(B, H, generator=g)
    leaves = [t.double().requires_grad_(True) for t in (cw, cb, pw, torch.zeros(H))]
    Wc, bc, Wp, bp = leaves
    ((Wp @ Wc) * dwloc.double().sum(0)).sum().add(((bp + Wp @ bc) * dbloc.double().sum(0)).sum()).backward()
    aw, ab = dwloc.double().abs().sum(0), dbloc.double().abs().sum(0)
    mag = [pw.double().abs().t() @ aw, pw.double().abs().t() @ ab, aw @ cw.double().abs().t() + ab[:, None] * cb.double().abs()[None], ab]
    ins = [_d(t) for t in (dwloc, dbloc, cw, cb, pw)]
    outs = [Buf(kd, taps), Buf(kd), Buf(H, kd), Buf(H)]
    rc = lib.d2t_op_loc_unfold_bwd(_p(ins[0]), _p(ins[1]), B, _p(ins[2]), _p(ins[3]), _p(ins[4]), H, kd, taps, *[_p(o) for o in outs],
                                   _stream())
    torch.cuda.synchronize()
    assert rc == 0
    for name, o, leaf, m in zip(("d_conv_w", "d_conv_b", "d_proj_w", "d_proj_b"), outs, leaves, mag):
        got = o.get().double()
        assert not torch.isnan(got).any(), name
        tol = (B + H + 4) * U * m
        over = float(((got - leaf.grad).abs() - tol).max())
        _fig("loc_unfold_" + name, kd=kd, taps=taps, B=B, err=float((got - leaf.grad).abs().max()), tol_min=float(tol.min()))
        assert over <= 0, f"{name}: |y - y64| exceeds the derived bound by {over:.3e}"
    for bad in (dict(B=0), dict(kd=0), dict(taps=0), dict(Hh=0)):
        outs2 = [Buf(kd, taps), Buf(kd), Buf(H, kd), Buf(H)]
        rc = lib.d2t_op_loc_unfold_bwd(_p(ins[0]), _p(ins[1]), bad.get("B", B), _p(ins[2]), _p(ins[3]), _p(ins[4]), bad.get("Hh", H),
                                       bad.get("kd", kd), bad.get("taps", taps), *[_p(o) for o in outs2], _stream())
        torch.cuda.synchronize()
        assert rc == EINVAL and all(o.untouched() for o in outs2)
