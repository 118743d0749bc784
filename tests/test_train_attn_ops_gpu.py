"""GPU: the five kernels of csrc/train_attn.hip -- forward with K / V in LDS or read from global memory (GKV); backward "fast"
(coalesced), plain LDS, or GKV -- at every wave count their launchers choose, with and without the dropout of
nn.MultiheadAttention on the probabilities, in the separate (q, kv) and the packed (one qkv tensor as both operands) layout,
through d2t_op_train_attention_ex, which runs Tr::attention and Tr::bwd_attn themselves.  References: tests/train_attn_refs.py
(float64 torch, pinned by tests/test_train_attn_refs_cpu.py).

Every tape buffer of the entry starts as NaN and every output of a test is a NaN-filled buffer with a guard tail: an element the
kernels should have written and did not fails, and so does a write behind the specified region.  Every case asserts the `plan`
the entry reports (forward form, waves, backward form, waves), so a case reaches the kernel its comment claims.

Tolerances (none of them taken from the code under test):
  measured  y, probs, ds, dq, dk, dv:  max |x - x64| <= 8 e32 + 1e-6 max |x64|, e32 = the largest max |x32 - x64| over three fp32
            CPU evaluations of forward and explicit backward on the same inputs and mask (torch's own reductions, every
            reduction reversed, every reduction in 16 chunks summed left to right).
  exact     zero at causally masked and PAD positions of probs and ds, zero dk / dv rows of keys no query may look at; a query
            row whose keys are all dropped has a zero y, ds and dq row; a key dropped for every query has a zero dv row (its dk
            row is NOT zero and follows the measured rule: the softmax Jacobian reaches a dropped entry);
  bitwise   an all-ones mask with dropscale 1 against no mask; the packed layout against the separate one (only addresses
            differ); a batch item alone against its slice of the batched run.
Every figure is printed (`FIG ...` lines, pytest -s) before it is asserted; DESIGN.md 5.5e has the table from an MI355X.

Shown to fail when a kernel is made subtly wrong (scratch builds, one mutation of train_attn.hip at a time, every address in
range, each build run once on an MI355X on this file and on test_train_ops_gpu.py::test_attention_backward, "old" below;
DESIGN.md 5.5e has the table):
   1 forward: dropout also applied to the saved probs     -> 98 float64 cases (every masked one) + 20 designed; old passes
   2 fast backward: mask ignored in dV                     -> 54 float64 cases + 8 designed (the fast kernel's); old passes
   3 plain backward only: mask dropped from the 2nd dp loop -> 10 float64 cases + 2 designed (exactly the plain ones); old passes
   4 GKV backward: dropscale omitted                       -> 34 float64 cases + 10 designed (exactly the GKV ones); old passes
   5 colred stepping 64 * 4, not 64 * nkg                  -> all 14 shapes on a fast rung below 16 waves (NaN: keys never written),
                                                              42 float64 cases, 26 others; old passes (it has 16 waves only)
   6 GKV: head offset dropped from the K pointer           -> 30 float64 cases + 4 designed; old fails too (2 of 10)
   7 fast backward: dS zeroed at dropped entries           -> 50 float64 cases + 8 designed; old passes
   8 plain / GKV backward: the same                        -> 44 float64 cases + 12 designed; old passes
   9 colred: a zero sum is not stored                      -> 76 cases, NaN in dk / dv rows of masked keys, in both layouts; old
                                                              passes (its entry zeroes the gradients first)
  11 forward: row maximum not subtracted                   -> test_large_scores_do_not_overflow (all 3) and Lk = 1, where the
                                                              probability is no longer exactly 1; old passes
NOT caught: 10 (expf -> __expf in the forward): a precision choice inside the rule -- probs ratio at most 1.25 either way,
y 5.7 -> 6.4 in the GKV forward.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import train_attn_refs as AR
from doc2tex_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = 1  # include/d2t.h D2T_EINVAL
NAN = float("nan")
GUARD = 64
LDS, GKV = 0, 1            # forward forms (include/d2t.h)
FAST, PLAIN, BGKV = 0, 1, 2  # backward forms
FORM = {("f", LDS): "fwd_lds", ("f", GKV): "fwd_gkv", ("b", FAST): "bwd_fast", ("b", PLAIN): "bwd_plain", ("b", BGKV): "bwd_gkv"}


def _fig(name, **kv):
    print("FIG " + name + " " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class Buf:
    """a device output of `shape` filled with NaN, with a guard tail behind it"""

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.t = torch.full((self.n + GUARD,), NAN, dtype=torch.float32, device=DEV)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def untouched(self):
        return bool(torch.isnan(self.t.cpu()).all())

    def get(self):
        c = self.t.cpu()
        assert bool(torch.isnan(c[self.n:]).all()), "a kernel wrote behind its output"
        return c[:self.n].view(*self.shape)


# ---------------------------------------------------------------------------------------------------------------------
# cases: (nb, Lq, Lk, heads, hd, causal, pad), the plan they must reach (forward form, waves, backward form, waves)
# 160 KB of LDS decide the plan (launch_attn_train_fwd / _bwd); the entry reports it and _run asserts it
# ---------------------------------------------------------------------------------------------------------------------
def _rung(Lk, hd, plan, Lq=8, heads=2, causal=0, pad=False, nb=1):
    return ((nb, Lq, Lk, heads, hd, causal, pad), plan)


CASES = [
    # the model's own shapes (tests/test_train_ops_gpu.py::test_attention_backward)
    ((3, 37, 37, 8, 32, 0, False), (LDS, 16, FAST, 16)),    # ViT block
    ((2, 261, 261, 8, 32, 0, False), (LDS, 16, FAST, 16)),  # ViT at the headline token count
    ((3, 25, 25, 8, 32, 1, True), (LDS, 16, FAST, 16)),     # decoder self-attention: causal + PAD
    ((2, 23, 23, 8, 64, 1, True), (LDS, 16, FAST, 16)),     # ... at d_model 512
    ((3, 25, 70, 8, 32, 0, False), (LDS, 16, FAST, 16)),    # decoder cross-attention
    ((1, 320, 320, 2, 32, 1, True), (LDS, 16, PLAIN, 4)),   # dO and Q no longer fit beside K and V: the plain kernel, Lq large
    ((1, 160, 160, 2, 64, 0, False), (LDS, 16, PLAIN, 4)),
    # self-attention where the fast backward steps down: the crops just below the plain kernel's
    ((1, 285, 285, 2, 32, 1, False), (LDS, 16, FAST, 12)),
    ((1, 292, 292, 2, 32, 0, False), (LDS, 16, FAST, 8)),
    ((2, 300, 300, 2, 32, 1, True), (LDS, 16, FAST, 4)),
    ((1, 152, 152, 2, 64, 0, False), (LDS, 16, FAST, 8)),
    # every rung of the launchers at Lq = 8, head size 32 ...
    _rung(448, 32, (LDS, 16, FAST, 16)), _rung(493, 32, (LDS, 16, FAST, 16)),
    _rung(500, 32, (LDS, 16, FAST, 12)),
    _rung(511, 32, (LDS, 12, FAST, 12)),
    _rung(525, 32, (LDS, 12, FAST, 8)),
    _rung(539, 32, (LDS, 8, FAST, 8), pad=True, nb=2),
    _rung(555, 32, (LDS, 8, FAST, 4)),
    _rung(570, 32, (LDS, 4, FAST, 4)),
    _rung(581, 32, (LDS, 4, PLAIN, 4), pad=True, nb=2),
    _rung(590, 32, (LDS, 4, BGKV, 16)),
    _rung(600, 32, (GKV, 16, BGKV, 16)), _rung(640, 32, (GKV, 16, BGKV, 16)),
    _rung(600, 32, (GKV, 16, BGKV, 16), causal=1, pad=True, nb=2),
    _rung(610, 32, (GKV, 16, BGKV, 16), pad=True, nb=2),
    _rung(2600, 32, (GKV, 12, BGKV, 12), Lq=4, heads=1),
    _rung(3500, 32, (GKV, 8, BGKV, 8), Lq=4, heads=1),
    _rung(5200, 32, (GKV, 4, BGKV, 4), Lq=4, heads=1),
    _rung(10240, 32, (GKV, 4, BGKV, 4), Lq=4, heads=1),     # the largest Lk the launchers take
    # ... and 64
    _rung(277, 64, (LDS, 16, FAST, 12)),
    _rung(286, 64, (LDS, 12, FAST, 8)),
    _rung(295, 64, (LDS, 8, FAST, 4)),
    _rung(302, 64, (LDS, 4, PLAIN, 4)),
    _rung(306, 64, (LDS, 4, BGKV, 16)),
    _rung(311, 64, (GKV, 16, BGKV, 16)), _rung(320, 64, (GKV, 16, BGKV, 16)),
    _rung(333, 64, (GKV, 16, BGKV, 16), pad=True, nb=2),
    _rung(2561, 64, (GKV, 12, BGKV, 12), Lq=4, heads=1),
    _rung(3414, 64, (GKV, 8, BGKV, 8), Lq=4, heads=1),
    _rung(5121, 64, (GKV, 4, BGKV, 4), Lq=4, heads=1),
    # edges: one key, one query, fewer queries than waves, around one 64-key block
    ((2, 5, 1, 2, 32, 0, False), (LDS, 16, FAST, 16)),
    ((1, 1, 1, 1, 64, 1, False), (LDS, 16, FAST, 16)),
    ((2, 1, 37, 2, 32, 0, True), (LDS, 16, FAST, 16)),
    ((1, 3, 570, 2, 32, 0, False), (LDS, 4, FAST, 4)),
    ((1, 1, 585, 2, 32, 0, False), (LDS, 4, PLAIN, 4)),
    ((1, 2, 600, 2, 32, 0, False), (GKV, 16, BGKV, 16)),
    ((2, 63, 63, 2, 32, 1, True), (LDS, 16, FAST, 16)),
    ((2, 64, 64, 2, 32, 0, False), (LDS, 16, FAST, 16)),
    ((2, 65, 65, 2, 64, 1, False), (LDS, 16, FAST, 16)),
]
SHAPES = [c for c, _ in CASES]
PLAN = dict(CASES)
assert len(PLAN) == len(CASES)
SELF = [c for c in SHAPES if c[1] == c[2]]
DROPS = [None, 0.1, 0.5]


def _id(c):
    return "x".join(map(str, c[:5])) + ("-causal" if c[5] else "") + ("-pad" if c[6] else "")


def _pid(p):
    return "nomask" if p is None else f"p{p}"


def _pick(pred):
    """the first case of every (forward form, backward form, backward waves) that pred admits: one of each kernel and rung"""
    seen, out = set(), []
    for c, pl in CASES:
        key = (pl[0], pl[2], pl[3], c[4])
        if pred(c) and key not in seen:
            seen.add(key)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def _inputs(case):
    nb, Lq, Lk, heads, hd, causal, pad = case
    q, kv, dy, keytok = AR.make_inputs(nb, Lq, Lk, heads, hd, pad, seed=1000 + 7 * Lq + 11 * Lk + hd + nb + causal)
    return dict(q=q, kv=kv, dy=dy, keytok=keytok)


@functools.lru_cache(maxsize=None)
def _keep(case, p):
    nb, Lq, Lk, heads, hd, causal, pad = case
    return None if p is None else AR.keep_mask(nb, heads, Lq, Lk, p, seed=int(1000 * p) + Lq + Lk)


def _scale(p):
    return 1.0 if p is None else float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))  # 1.f / (1.f - p) as train.hip forms it


def _reference(case, keep, dropscale):
    nb, Lq, Lk, heads, hd, causal, pad = case
    return AR.attn_ref_and_e32(nb=nb, Lq=Lq, Lk=Lk, heads=heads, hd=hd, causal=causal, keep=keep, dropscale=dropscale,
                               **_inputs(case))


def _ref(case, p):
    return _reference(case, _keep(case, p), _scale(p))


def _launch(case, k, keep, dropscale, layout, plan_init=(-1, -1, -1, -1), override=None):
    """the entry on NaN-filled outputs; returns (rc, plan, outputs as Bufs)"""
    nb, Lq, Lk, heads, hd, causal, pad = case
    D = heads * hd
    lib = _lib.require_device()
    a = _lib.D2TOpTrainAttentionArgs()
    keepalive = []

    def dev(t):
        t = t.contiguous().to(DEV)
        keepalive.append(t)
        return t.data_ptr()
    out = dict(y=Buf(nb * Lq, D), probs=Buf(nb, heads, Lq, Lk), ds=Buf(nb, heads, Lq, Lk))
    if layout == 1:
        a.qkv = dev(torch.cat([k["q"], k["kv"]], 1))
        out["dqkv"] = Buf(nb * Lq, 3 * D)
    else:
        a.q, a.kv = dev(k["q"]), dev(k["kv"])
        out["dq"], out["dkv"] = Buf(nb * Lq, D), Buf(nb * Lk, 2 * D)
    a.dy = dev(k["dy"])
    if k["keytok"] is not None:
        a.keytok = dev(k["keytok"])
    if keep is not None:
        a.dropmask = dev(keep)
    for name, b in out.items():
        setattr(a, name, b.ptr)
    plan = (C.c_int32 * 4)(*plan_init)
    a.plan = C.addressof(plan)
    a.dropscale = dropscale
    a.layout, a.nb, a.Lq, a.Lk, a.heads, a.hd, a.causal = layout, nb, Lq, Lk, heads, hd, causal
    for name, v in (override or {}).items():
        setattr(a, name, v)
    rc = lib.d2t_op_train_attention_ex(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, tuple(plan), out


def _outputs(case, k, keep, dropscale, layout):
    """a run that must succeed with the plan the case claims: y, probs, ds, dq, dk, dv on the host (guard tails checked)"""
    rc, plan, out = _launch(case, k, keep, dropscale, layout)
    assert rc == 0
    if case in PLAN:
        assert plan == PLAN[case], f"{_id(case)} reaches plan {plan}, not {PLAN[case]}"
    D = case[3] * case[4]
    r = {n: out[n].get() for n in ("y", "probs", "ds")}
    if layout == 1:
        g = out["dqkv"].get()
        r.update(dq=g[:, :D], dk=g[:, D:2 * D], dv=g[:, 2 * D:])
    else:
        r.update(dq=out["dq"].get(), dk=out["dkv"].get()[:, :D], dv=out["dkv"].get()[:, D:])
    for n, t in r.items():
        assert not torch.isnan(t).any(), f"{n}: unwritten / NaN elements"
    return r


@functools.lru_cache(maxsize=None)
def _run(case, p, layout=0):
    return _outputs(case, _inputs(case), _keep(case, p), _scale(p), layout)


def _rule(name, case, got, y64, e32, **kv):
    """the measured rule on the six outputs; figures are tagged with the kernel that wrote the output"""
    pl = PLAN[case]
    fwd, bwd = FORM["f", pl[0]] + f"/{pl[1]}", FORM["b", pl[2]] + f"/{pl[3]}"
    bad = []
    for n in AR.OUTPUTS:
        err = float((got[n].double() - y64[n]).abs().max())
        mx = float(y64[n].abs().max())
        _fig(f"{name}_{n}", kernel=fwd if n in ("y", "probs") else bwd, hd=case[4], e32=e32[n], err=err,
             ratio=err / e32[n] if e32[n] > 0 else 0.0, max=mx, case=_id(case), **kv)
        if not err <= 8.0 * e32[n] + 1e-6 * mx:
            bad.append(f"{n}: |x - x64| = {err:.3e}, e32 = {e32[n]:.3e}, max |x64| = {mx:.3e}")
    assert not bad, f"{name} {_id(case)}: " + "; ".join(bad)


def _masked_zeros(case, got):
    """exact zeros where the masks say so"""
    nb, Lq, Lk, heads, hd, causal, pad = case
    valid = AR.valid_keys(nb, Lq, Lk, causal, _inputs(case)["keytok"]).expand(nb, heads, Lq, Lk)
    assert bool((got["probs"][~valid] == 0).all()), "probs at masked positions"
    assert bool((got["ds"][~valid] == 0).all()), "ds at masked positions"
    dead = ~valid.any(2)  # [nb][heads][Lk]: keys no query may look at (PAD, or behind the last query of a causal mask)
    for n in ("dk", "dv"):
        rows = got[n].view(nb, Lk, heads, hd).transpose(1, 2)[dead]
        assert bool((rows == 0).all()), f"{n} rows of masked keys"
    return int((~valid).sum()), int(dead.sum())


# =====================================================================================================================
@pytest.mark.parametrize("p", DROPS, ids=_pid)
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_forward_and_backward_against_float64(case, p):
    """every form and rung, without a mask and with random masks at p = 0.1 and 0.5: the measured rule on y, probs, ds, dq, dk,
    dv; exact zeros at masked positions"""
    got = _run(case, p)
    y64, e32 = _ref(case, p)
    masked, dead = _masked_zeros(case, got)
    _rule("attn", case, got, y64, e32, p=_pid(p), masked=masked, dead_keys=dead)


@pytest.mark.parametrize("p", DROPS, ids=_pid)
@pytest.mark.parametrize("case", SELF, ids=_id)
def test_packed_layout_is_bitwise_the_separate_one(case, p):
    """one qkv [nb*L][3D] tensor as both operands (the call of the ViT blocks and of the decoder's self-attention): bwd_attn
    takes own_grad twice on one tensor, whose NaN-filled gradient the three kernels' stores must cover between them"""
    sep, packed = _run(case, p), _run(case, p, 1)
    for n in AR.OUTPUTS:
        bad = int((_bits(sep[n]) != _bits(packed[n])).sum())
        _fig(f"packed_{n}", differing=bad, n=sep[n].numel(), case=_id(case), p=_pid(p))
        assert bad == 0, f"{n}: {bad} elements differ between the layouts"


ONE_OF_EACH = _pick(lambda c: True)


@pytest.mark.parametrize("case", ONE_OF_EACH, ids=_id)
def test_all_ones_mask_with_scale_one_is_no_mask(case):
    nb, Lq, Lk, heads, hd, causal, pad = case
    got = _outputs(case, _inputs(case), torch.ones(nb, heads, Lq, Lk, dtype=torch.uint8), 1.0, 0)
    want = _run(case, None)
    for n in AR.OUTPUTS:
        bad = int((_bits(got[n]) != _bits(want[n])).sum())
        _fig(f"ones_{n}", differing=bad, n=want[n].numel(), case=_id(case))
        assert bad == 0, f"{n}: {bad} elements differ from the unmasked run"


@pytest.mark.parametrize("case", _pick(lambda c: c[1] >= 2 and c[2] >= 2), ids=_id)
def test_designed_keep_masks(case):
    """a query row with every key dropped; a key column dropped for every query"""
    nb, Lq, Lk, heads, hd, causal, pad = case
    r, col = Lq - 1, 0  # (key 0 is never masked: every query looks at it)
    keep = AR.keep_mask(nb, heads, Lq, Lk, 0.1, seed=Lq + Lk).clone()
    keep[:, :, r, :] = 0
    keep[:, :, :, col] = 0
    scale = _scale(0.1)
    got = _outputs(case, _inputs(case), keep, scale, 0)
    y64, e32 = _reference(case, keep, scale)
    _masked_zeros(case, got)
    _rule("designed", case, got, y64, e32)
    D = heads * hd
    for n in ("y", "dq"):
        assert bool((got[n].view(nb, Lq, D)[:, r] == 0).all()), f"{n} row of a query whose keys are all dropped"
    assert bool((got["ds"][:, :, r] == 0).all())
    assert bool((got["dv"].view(nb, Lk, D)[:, col] == 0).all()), "dv row of a key dropped for every query"
    # ... while its dk row is alive: held to the rule with the e32 of that row alone, which a zero row must miss by far
    row = lambda t: t.view(nb, Lk, D)[:, col].double()
    dk64 = row(y64["dk"])
    args = dict(nb=nb, Lq=Lq, Lk=Lk, heads=heads, hd=hd, causal=causal, keep=keep, dropscale=scale, **_inputs(case))
    e32_row = max(float((row(AR.attn_eval(torch.float32, m, **args)["dk"]) - dk64).abs().max()) for m in AR.MODES)
    err, mx = float((row(got["dk"]) - dk64).abs().max()), float(dk64.abs().max())
    bound = 8.0 * e32_row + 1e-6 * mx
    _fig("designed_dk_dropped_key", e32=e32_row, err=err, ratio=err / e32_row if e32_row > 0 else 0.0, max=mx, case=_id(case))
    assert mx > 100.0 * bound, "the designed column does not test anything"
    assert err <= bound


@pytest.mark.parametrize("case", [(3, 25, 25, 8, 32, 1, True), (3, 25, 70, 8, 32, 0, False), (1, 8, 600, 2, 32, 0, False)], ids=_id)
def test_large_scores_do_not_overflow(case):
    """queries times 40: scores beyond 100, where exp(score) itself is inf in fp32 (from 88.8) -- the row maximum has to come off
    first, in the LDS and in the GKV forward"""
    nb, Lq, Lk, heads, hd, causal, pad = case
    k = dict(_inputs(case))
    k["q"] = k["q"] * 40.0
    D = heads * hd
    s = AR.heads_of(k["q"].double(), nb, Lq, heads, hd) @ AR.heads_of(k["kv"][:, :D].double(), nb, Lk, heads, hd).transpose(-1, -2)
    s = (s * hd ** -0.5)[AR.valid_keys(nb, Lq, Lk, causal, k["keytok"]).expand_as(s)]
    _fig("hot_scores", lo=float(s.min()), hi=float(s.max()), case=_id(case))
    assert float(s.max()) > 100.0
    keep, scale = _keep(case, 0.1), _scale(0.1)
    got = _outputs(case, k, keep, scale, 0)
    y64, e32 = AR.attn_ref_and_e32(nb=nb, Lq=Lq, Lk=Lk, heads=heads, hd=hd, causal=causal, keep=keep, dropscale=scale, **k)
    _rule("hot", case, got, y64, e32)


@pytest.mark.parametrize("case", [c for c in SHAPES if c[0] > 1], ids=_id)
def test_batch_item_alone_is_its_slice(case):
    nb, Lq, Lk, heads, hd, causal, pad = case
    k, keep, D = _inputs(case), _keep(case, 0.1), heads * hd
    whole = _run(case, 0.1)
    b = nb - 1
    one = dict(q=k["q"][b * Lq:(b + 1) * Lq], kv=k["kv"][b * Lk:(b + 1) * Lk], dy=k["dy"][b * Lq:(b + 1) * Lq],
               keytok=None if k["keytok"] is None else k["keytok"][b:b + 1])
    alone = _outputs((1,) + case[1:], one, keep[b:b + 1], _scale(0.1), 0)
    for n in AR.OUTPUTS:
        L = Lq if n in ("y", "dq") else Lk
        want = whole[n][b:b + 1] if n in ("probs", "ds") else whole[n][b * L:(b + 1) * L]
        bad = int((_bits(alone[n]) != _bits(want)).sum())
        _fig(f"alone_{n}", differing=bad, n=want.numel(), case=_id(case))
        assert bad == 0, f"{n}: {bad} elements differ from the batched run"


def test_every_form_and_rung_is_reached():
    """the plans asserted above, between them: every kernel at every wave count, with and without a mask (DROPS)"""
    fwd = {(pl[0], pl[1], c[4]) for c, pl in CASES}
    bwd = {(pl[2], pl[3], c[4]) for c, pl in CASES}
    for hd in (32, 64):
        assert {(LDS, w, hd) for w in (16, 12, 8, 4)} | {(GKV, w, hd) for w in (16, 12, 8, 4)} <= fwd
        assert {(FAST, w, hd) for w in (16, 12, 8, 4)} | {(BGKV, w, hd) for w in (16, 12, 8, 4)} | {(PLAIN, 4, hd)} <= bwd
    both = {(pl[0], pl[2]) for c, pl in CASES}
    assert (LDS, BGKV) in both  # the mixed pair


def _all_untouched(out):
    return all(b.untouched() for b in out.values())


def test_launcher_refusal_leaves_every_buffer_alone():
    """Lk = 10241: not four rows of Lk floats in 160 KB.  The launcher refuses; the status is not zero and nothing is written"""
    case = (1, 1, 10241, 1, 32, 0, False)
    for p in (None, 0.5):
        rc, plan, out = _launch(case, _inputs(case), _keep(case, p), _scale(p), 0)
        _fig("refusal", rc=rc, plan=plan, p=_pid(p))
        assert rc not in (0, EINVAL) and plan == (GKV, 0, BGKV, 0)
        assert _all_untouched(out)
    rc, plan, out = _launch((1, 1, 10240, 1, 32, 0, False), _inputs((1, 1, 10240, 1, 32, 0, False)), None, 1.0, 0)
    assert rc == 0 and plan == (GKV, 4, BGKV, 4)


INVALID = [
    ("hd 48", 0, dict(hd=48)), ("hd 0", 0, dict(hd=0)), ("no batch", 0, dict(nb=0)), ("no query", 0, dict(Lq=0)),
    ("no key", 0, dict(Lk=0)), ("no head", 0, dict(heads=0)), ("negative Lk", 0, dict(Lk=-5)), ("layout 2", 0, dict(layout=2)),
    ("packed, Lq != Lk", 1, dict(Lk=8)), ("packed without qkv", 1, dict(qkv=None)), ("separate without kv", 0, dict(kv=None)),
    ("no dy", 0, dict(dy=None)), ("dropscale 0", 0, dict(dropscale=0.0)), ("dropscale negative", 0, dict(dropscale=-1.0)),
    ("dropscale inf", 0, dict(dropscale=math.inf)), ("dropscale NaN", 0, dict(dropscale=math.nan))]


@pytest.mark.parametrize("what,layout,override", INVALID, ids=[w[0].replace(" ", "_").replace(",", "") for w in INVALID])
def test_invalid_arguments_write_nothing(what, layout, override):
    case = (2, 9, 9, 2, 32, 1, True)
    rc, plan, out = _launch(case, _inputs(case), _keep(case, 0.5), _scale(0.5), layout, override=override)
    assert rc == EINVAL, what
    assert plan == (-1, -1, -1, -1) and _all_untouched(out)
    if not what.startswith("dropscale"):
        return
    rc, plan, out = _launch(case, _inputs(case), None, override["dropscale"], layout)  # without a mask the scale is not read
    assert rc == 0 and not torch.isnan(out["y"].get()).any()
