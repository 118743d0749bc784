"""GPU: the fused LAMB, AdamP, MADGRAD and Lookahead steps of doc2tex_amd.optim (include/d2t.h, "the optimizer family") against
the float64 restatements of tests/optim_family_refs.py (held against the reference's own classes in test_optim_family_cpu).

The bound of every update comparison is optim_refs.within_yardstick: the yardstick is the SAME restatement run eagerly in
float32 on the same device and inputs, and the fused kernel's largest absolute error against float64 may be at most twice
the yardstick's on that tensor plus one fp32 ulp of the tensor's largest magnitude.  Where a global norm scales the
gradients each side is held against the float64 step scaled by its OWN norm; the norm is bounded separately.  AdamP's
decisions are compared by ==: the inputs are built so that every comparison behind a decision has a margin of at least 25 %
of its threshold (asserted), which no fp32 rounding can cross.  The measured errors are in DESIGN.md §5.5c."""
import ctypes as C
import functools
import math

import pytest
import torch

import optim_family_refs as FR
import optim_refs as OR
from conftest import engine_model
from doc2tex_amd import _lib, synth
from doc2tex_amd import optim as O
from test_oracle_golden import _case, train_step_labels

pytestmark = pytest.mark.gpu
DEV = "cuda"
CH = O.CHUNK
# (shape, gradient kind of optim_family_refs.fixture_grad); "padrow": random with an all-zero row whose gradient row is zero
# too (an embedding's padding row); "zerop": an all-zero tensor (LAMB's trust ratio is 1; AdamP's cosine is 0)
SPECS = [((1,), "random"), ((3,), "random"), ((4,), "random"), ((5,), "random"), ((255,), "random"), ((257,), "random"),
         ((CH - 1,), "random"), ((CH,), "random"), ((CH + 1,), "random"), ((2 * CH + 7,), "random"),
         ((6,), "random"), ((9,), "zero"),
         ((1, 7), "random"), ((5, 9), "channel"), ((8, 257), "layer"), ((2, CH + 3), "channel"), ((300, 130), "channel"),
         ((6, 4, 3, 3), "layer"), ((6, 5), "padrow"), ((4, 3), "zerop"), ((7, 33), "random")]
# the tensor whose grad is None, the one with an all-zero gradient (entries of their own: every size the others name is
# stepped with a real gradient); tensors [:SPLIT] (one dimension) form group 0, which always decays or has momentum, the
# rest group 1
NO_GRAD, ZERO_GRAD, PADROW, ZEROP, SPLIT = 10, 11, 18, 19, 12
STATE = {"lamb": ("exp_avg", "exp_avg_sq"), "adamp": ("exp_avg", "exp_avg_sq"), "madgrad": ("grad_sum_sq", "s", "x0")}
CLASSES = {"lamb": O.FusedLamb, "adamp": O.FusedAdamP, "madgrad": O.FusedMADGRAD}
# name -> (optimizer, constructor arguments, overrides of group 0 and group 1, max_grad_norm)
CONFIGS = {
    # LAMB: the norm above max_grad_norm; weight_decay 0 without always_adapt (group 0: no trust ratio) and > 0; two groups
    "lamb_clip": ("lamb", dict(lr=2e-3, weight_decay=0.01, max_grad_norm=1.0), ({"weight_decay": 0.0}, {"lr": 3e-3}), None),
    # the norm below it; weight_decay 0 WITH always_adapt, no bias correction, no gradient averaging
    "lamb_adapt": ("lamb", dict(lr=2e-3, betas=(0.8, 0.95), weight_decay=0.0, max_grad_norm=1e4, always_adapt=True,
                                bias_correction=False, grad_averaging=False), ({}, {"weight_decay": 0.1}), None),
    # trust_clip where it acts: every tensor adapts, and their trust ratios lie on both sides of 1 (asserted in the test)
    "lamb_trust_clip": ("lamb", dict(lr=2e-3, weight_decay=0.01, max_grad_norm=1.0, always_adapt=True, trust_clip=True),
                        ({"weight_decay": 0.0}, {"lr": 3e-3}), None),
    "adamp_nesterov": ("adamp", dict(lr=2e-3, weight_decay=0.05, wd_ratio=0.01, nesterov=True), ({}, {"lr": 1e-3}), 5.0),
    "adamp_plain": ("adamp", dict(lr=2e-3, betas=(0.8, 0.95), weight_decay=0.0), ({}, {}), None),
    "madgrad_momentum": ("madgrad", dict(lr=1e-2, momentum=0.9, weight_decay=0.01), ({}, {"weight_decay": 0.0}), 5.0),
    "madgrad_plain": ("madgrad", dict(lr=1e-2, momentum=0.0, weight_decay=0.01, decoupled_decay=True), ({}, {"weight_decay": 0.0}), None),
    "madgrad_noclip": ("madgrad", dict(lr=5e-3, momentum=0.9, weight_decay=0.02, decoupled_decay=True), ({}, {}), 1e4),
}


@functools.lru_cache(maxsize=None)
def _problem(seed=17):
    """Seeded CPU fp32 tensors, never written: per tensor p, g and every state tensor any of the optimizers needs."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, (shape, kind) in enumerate(SPECS):
        r = lambda scale=1.0: scale * torch.randn(shape, generator=gen)  # noqa: E731
        p = r()
        t = {"exp_avg": r(0.1), "exp_avg_sq": r(0.1) ** 2, "grad_sum_sq": 0.5 + r().abs(), "s": r(0.05)}
        if kind == "padrow":
            p[2] = 0.0
            for v in t.values():
                v[2] = 0.0
        if kind == "zerop":
            p.zero_()
        t["x0"] = p + r(0.05) * (kind != "zerop")
        g = FR.fixture_grad({"padrow": "random", "zerop": "random"}.get(kind, kind), p, 3, i).float()
        if kind == "padrow":
            g[2] = 0.0
        out.append(dict(t, p=p, g=g))
    return out


def _instantiate(prob, flip=0):
    """Fresh device parameters with their gradients set: every second tensor's gradient (the odd ones, with `flip` the even
    ones) is a view that starts one float into a larger buffer (4-byte aligned only: the kernels' scalar path)."""
    ps = []
    for i, t in enumerate(prob):
        q = torch.nn.Parameter(t["p"].to(DEV).clone())
        if i == NO_GRAD:
            q.grad = None
        elif (i + flip) % 2 == 1:
            buf = torch.zeros(t["g"].numel() + 1, device=DEV)
            buf[1:] = t["g"].to(DEV).reshape(-1)
            q.grad = buf[1:].view(t["g"].shape)
            assert q.grad.data_ptr() % 16 == 4 and q.grad.is_contiguous()
        else:
            q.grad = t["g"].to(DEV).clone()
            assert q.grad.data_ptr() % 16 == 0
        ps.append(q)
    return ps


def _hyper(name):
    """Per tensor: the constructor's defaults overlaid with the configuration and its group's overrides."""
    kind, args, overrides, _ = CONFIGS[name]
    defaults = dict(CLASSES[kind]([torch.nn.Parameter(torch.zeros(1))]).defaults, **args)
    return [dict(defaults, **overrides[i >= SPLIT]) for i in range(len(SPECS))]


def _fused_step(name, start):
    """One step from the loaded state at step count `start`.  At start 0 the odd tensors' gradients are the misaligned views,
    at any other start the even ones: over the two starts of a test every tensor takes the 16-byte and the scalar path."""
    kind, args, overrides, mgn = CONFIGS[name]
    prob = _problem()
    ps = _instantiate(prob, flip=int(start != 0))
    groups = [dict(params=ps[:SPLIT], **overrides[0]), dict(params=ps[SPLIT:], **overrides[1])]
    opt = CLASSES[kind](groups, **args) if kind == "lamb" else CLASSES[kind](groups, max_grad_norm=mgn, **args)
    hyper = _hyper(name)
    keys = [k for k in STATE[kind]]
    sd = opt.state_dict()
    sd["state"] = {i: dict({k: t[k].clone() for k in keys if k != "x0" or hyper[i]["momentum"] != 0},
                           **({} if kind == "lamb" else {"step": start})) for i, t in enumerate(prob)}
    if kind == "lamb":
        for g in sd["param_groups"]:
            g["step"] = start
    opt.load_state_dict(sd)
    grads_before = [None if p.grad is None else p.grad.clone() for p in ps]
    opt.step()
    torch.cuda.synchronize()
    for p, g in zip(ps, grads_before):  # the gradients are only read, bit for bit
        assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))
    out = {"p": [p.detach().cpu() for p in ps], "norm": None if opt.grad_norm is None else opt.grad_norm.cpu(),
           "state_keys": [sorted(opt.state[p]) for p in ps],
           "modes": opt.projection_modes().cpu().tolist() if kind == "adamp" else None,
           "steps": [g["step"] for g in opt.param_groups] if kind == "lamb" else [opt.state[p]["step"] for p in ps]}
    for k in keys:
        out[k] = [opt.state[p][k].cpu() if k in opt.state[p] else None for p in ps]
    return out


_fused_step_cached = functools.lru_cache(maxsize=None)(_fused_step)


def _restate(name, i, step, scale, dtype):
    """Tensor i's step by the restatement in `dtype` on the device: {quantity: tensor}, and AdamP's (mode, margin)."""
    kind = CONFIGS[name][0]
    t, h = {k: v.to(DEV) for k, v in _problem()[i].items()}, _hyper(name)[i]
    if kind == "lamb":
        p, m, v = FR.lamb_step(t["p"], t["g"], t["exp_avg"], t["exp_avg_sq"], step, h["lr"], h["betas"], h["eps"], h["weight_decay"],
                               scale, h["bias_correction"], h["grad_averaging"], h["trust_clip"], h["always_adapt"], dtype=dtype)
        return {"p": p, "exp_avg": m, "exp_avg_sq": v}, None
    if kind == "adamp":
        p, m, v, mode, margin = FR.adamp_step(t["p"], t["g"], t["exp_avg"], t["exp_avg_sq"], step, h["lr"], h["betas"], h["eps"],
                                              h["weight_decay"], h["delta"], h["wd_ratio"], h["nesterov"], scale, dtype=dtype)
        return {"p": p, "exp_avg": m, "exp_avg_sq": v}, (mode, margin)
    p, q, s = FR.madgrad_step(t["p"], t["g"], t["grad_sum_sq"], t["s"], t["x0"] if h["momentum"] else None, step, h["lr"],
                              h["momentum"], h["eps"], h["weight_decay"], h["decoupled_decay"], scale, dtype=dtype)
    return {"p": p, "grad_sum_sq": q, "s": s}, None


def _scales(name, norm_fused):
    """(what scales the gradients in the fused step, in the yardstick): LAMB's divisor or clip_grad_norm_'s coefficient, each
    from its own side's norm -- the yardstick's is the eager fp32 norm on the device."""
    kind, args, _, mgn = CONFIGS[name]
    grads = [t["g"].to(DEV) for i, t in enumerate(_problem()) if i != NO_GRAD]
    norm_yard = float(torch.sqrt(sum((g * g).sum() for g in grads)))
    if kind == "lamb":
        return FR.lamb_divisor(norm_fused, args["max_grad_norm"]), FR.lamb_divisor(norm_yard, args["max_grad_norm"])
    if mgn is None:
        return 1.0, 1.0
    return OR.clip_coef(norm_fused, mgn), OR.clip_coef(norm_yard, mgn)


def _check(name, start):
    r = _fused_step_cached(name, start)
    kind = CONFIGS[name][0]
    s_fused, s_yard = _scales(name, None if r["norm"] is None else float(r["norm"]))
    worst, modes, margins = {}, [], []
    for i in range(len(SPECS)):
        if i == NO_GRAD:
            modes.append(0)
            continue
        ref_f, decision = _restate(name, i, start + 1, s_fused, torch.float64)
        ref_y = ref_f if s_fused == s_yard else _restate(name, i, start + 1, s_yard, torch.float64)[0]
        yard, _ = _restate(name, i, start + 1, s_yard, torch.float32)
        if decision:
            modes.append(decision[0])
            margins.append(decision[1])
        for q in ref_f:
            ok, e_got, e_yard, allowed = OR.within_yardstick(r[q][i], ref_f[q], yard[q], ref_y[q])
            if q not in worst or e_got - allowed > worst[q][0] - worst[q][2]:
                worst[q] = (e_got, e_yard, allowed, i)
            assert ok, (name, start, i, SPECS[i], q, "fused", e_got, "yardstick", e_yard, "allowed", allowed)
    print(f"[optim] {name} step={start + 1}: " + "  ".join(f"{k}: fused {w[0]:.3e} eager fp32 {w[1]:.3e} allowed {w[2]:.3e} (tensor {w[3]})"
                                                          for k, w in sorted(worst.items())))
    return r, modes, margins


def _untouched(r, kind, start):
    """The tensor without a gradient: parameter, state and step count as loaded; every other step count moved by one."""
    t = _problem()[NO_GRAD]
    assert torch.equal(r["p"][NO_GRAD], t["p"])
    for k in STATE[kind]:
        assert r[k][NO_GRAD] is None or torch.equal(r[k][NO_GRAD], t[k])
    if kind == "lamb":
        assert r["steps"] == [start + 1] * 2
    else:
        assert r["steps"] == [start if i == NO_GRAD else start + 1 for i in range(len(SPECS))]
        assert all(type(s) is int for s in r["steps"])
    assert not torch.equal(r["p"][ZERO_GRAD], _problem()[ZERO_GRAD]["p"])  # a zero gradient still moves its tensor (momentum)


# ---- the norm ------------------------------------------------------------------------------------------------------------
def test_norms_are_the_float64_norm():
    """2e-5 relative, derived as in test_optim_gpu: a thread's serial fp32 sum has at most CHUNK / 256 = 128 terms at 2^-24
    each (7.6e-6), all above it is double, the square root halves the relative error, one fp32 rounding stores it."""
    want = OR.grad_norm([t["g"] for i, t in enumerate(_problem()) if i != NO_GRAD])
    for name in ("lamb_clip", "adamp_nesterov", "madgrad_momentum"):
        got = float(_fused_step_cached(name, 0)["norm"])
        print(f"[optim] {name} norm: fused {got!r} float64 {want!r} rel {abs(got - want) / want:.3e}")
        assert abs(got - want) <= 2e-5 * want
    assert want > 5.0  # the clamp of max_grad_norm 5 (and LAMB's 1) is active, that of 1e4 is not
    assert _fused_step_cached("adamp_plain", 0)["norm"] is None and _fused_step_cached("madgrad_plain", 0)["norm"] is None


# ---- LAMB ----------------------------------------------------------------------------------------------------------------
def _trust_ratios(name, start, norm):
    """{tensor: |p| / |u| in float64 before trust_clip, None where the tensor does not adapt} of the step `_check` restates."""
    out = {}
    for i, (t, h) in enumerate(zip(_problem(), _hyper(name))):
        if i != NO_GRAD:
            out[i] = FR.lamb_trust_ratio(t["p"], t["g"], t["exp_avg"], t["exp_avg_sq"], start + 1, h["betas"], h["eps"], h["weight_decay"],
                                         FR.lamb_divisor(norm, h["max_grad_norm"]), h["bias_correction"], h["grad_averaging"],
                                         h["always_adapt"])
    return out


@pytest.mark.parametrize("start", [0, 999])
@pytest.mark.parametrize("name", ["lamb_clip", "lamb_adapt", "lamb_trust_clip"])
def test_lamb_within_twice_the_eager_error(name, start):
    r, _, _ = _check(name, start)
    ratios = _trust_ratios(name, start, float(r["norm"]))
    assert all((x is None) == (i < SPLIT and name == "lamb_clip") for i, x in ratios.items())  # weight_decay 0, no always_adapt
    if CONFIGS[name][1].get("trust_clip"):
        # a condition on the inputs: the clip acts on some tensors (ratio well above 1) and leaves others alone (well below)
        print(f"[optim] {name} step={start + 1}: trust ratios before the clip {min(ratios.values()):.3f} .. {max(ratios.values()):.3f}")
        assert max(ratios.values()) >= 1.25 and min(ratios.values()) <= 0.8
    _untouched(r, "lamb", start)
    assert all(keys == ["exp_avg", "exp_avg_sq"] for keys in r["state_keys"])
    # the all-zero tensor: |p| = 0, the trust ratio is 1 and the step is -lr * u
    assert torch.count_nonzero(r["p"][ZEROP]) == r["p"][ZEROP].numel()


# ---- AdamP ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 999])
@pytest.mark.parametrize("name", ["adamp_nesterov", "adamp_plain"])
def test_adamp_within_twice_the_eager_error(name, start):
    r, modes, margins = _check(name, start)
    _untouched(r, "adamp", start)
    assert min(margins) >= 0.25, margins  # a condition on the inputs: no fp32 reduction order can flip a decision
    assert r["modes"] == modes
    want = {i: {"channel": 1, "layer": 2, "zerop": 1}.get(kind, 0) for i, (shape, kind) in enumerate(SPECS) if len(shape) > 1}
    assert {i: modes[i] for i in want} == want and set(want.values()) == {0, 1, 2}
    assert all(keys == ["exp_avg", "exp_avg_sq", "step"] for i, keys in enumerate(r["state_keys"]))
    assert torch.equal(r["p"][PADROW][2], torch.zeros(5))  # the padding row stays zero


# ---- MADGRAD -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 999])
@pytest.mark.parametrize("name", ["madgrad_momentum", "madgrad_plain", "madgrad_noclip"])
def test_madgrad_within_twice_the_eager_error(name, start):
    r, _, _ = _check(name, start)
    _untouched(r, "madgrad", start)
    momentum = CONFIGS[name][1]["momentum"]
    for i, t in enumerate(_problem()):
        if momentum:
            assert torch.equal(r["x0"][i], t["x0"])  # read only
        assert r["state_keys"][i] == (["grad_sum_sq", "s", "step", "x0"] if momentum else ["grad_sum_sq", "s", "step"])


# ---- reproducibility -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lamb_clip", "adamp_nesterov", "madgrad_momentum"])
def test_two_runs_give_the_same_bits(name):
    a, b = _fused_step_cached(name, 999), _fused_step(name, 999)
    for k in ("p",) + STATE[CONFIGS[name][0]]:
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
    assert torch.equal(a["norm"], b["norm"]) and a["modes"] == b["modes"]


# ---- Lookahead -----------------------------------------------------------------------------------------------------------
LOOK = [1, 5, 8, 13, 16]  # sizes 3, 257 (its gradient one float into a buffer), CH + 1, (5, 9) (the same), (300, 130)


def _odd_views(g, odd):
    """The gradient on the device; for `odd` as a view one float into a buffer."""
    if not odd:
        return g.to(DEV).clone()
    buf = torch.zeros(g.numel() + 1, device=DEV)
    buf[1:] = g.to(DEV).reshape(-1)
    return buf[1:].view(g.shape)


@pytest.mark.parametrize("base", ["adamw", "lamb"])
def test_lookahead_k3_over_seven_steps(base):
    """Beside the wrapped optimizer runs a twin of its base on the same gradients: up to step 5 the two agree bit for bit
    (the synchronisation of step 3 creates the slow weights as copies and changes nothing, steps 4 and 5 move nothing but
    the base), at step 6 the slow weights are the restated slow + alpha (fast - slow) and the fast weights their copies."""
    prob = [_problem()[i] for i in LOOK]
    gen = torch.Generator().manual_seed(29)
    grads = [[torch.randn(t["p"].shape, generator=gen) for t in prob] for _ in range(7)]
    make = {"adamw": lambda ps: O.FusedAdamW(ps, lr=1e-2, max_grad_norm=5.0), "lamb": lambda ps: O.FusedLamb(ps, lr=1e-2)}[base]
    ps = [torch.nn.Parameter(t["p"].to(DEV).clone()) for t in prob]
    twin = [torch.nn.Parameter(t["p"].to(DEV).clone()) for t in prob]
    look, alone = O.Lookahead(make(ps), alpha=0.5, k=3), make(twin)
    slow3 = after6 = None
    for step in range(1, 8):
        for i, (p, q) in enumerate(zip(ps, twin)):
            p.grad, q.grad = _odd_views(grads[step - 1][i], i % 2), _odd_views(grads[step - 1][i], i % 2)
        look.step()
        if step <= 6:
            alone.step()
        torch.cuda.synchronize()
        slow = [look._base_optimizer.state[p].get("lookahead_slow_buff") for p in ps]
        if step < 3:
            assert all(s is None for s in slow)
        if step <= 5:
            assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(ps, twin)), step
        if step == 3:
            assert all(torch.equal(s, p.detach()) for s, p in zip(slow, ps))
            slow3 = [s.clone() for s in slow]
        if step in (4, 5):
            assert all(torch.equal(s, s3) for s, s3 in zip(slow, slow3))
        if step == 6:  # twin holds the fast weights the second synchronisation started from
            for i, (p, s, q, s3) in enumerate(zip(ps, slow, twin, slow3)):
                assert torch.equal(p.detach(), s)
                ref = FR.lookahead_sync(q.detach(), s3, 0.5)
                yard = FR.lookahead_sync(q.detach(), s3, 0.5, dtype=torch.float32)
                ok, e_got, e_yard, allowed = OR.within_yardstick(s, ref, yard, ref)
                assert ok, (base, i, e_got, e_yard, allowed)
                assert not torch.equal(s, s3) and not torch.equal(s, q.detach())
            after6 = [s.clone() for s in slow]
        if step == 7:
            assert all(torch.equal(s, a6) for s, a6 in zip(slow, after6))
            assert not any(torch.equal(p.detach(), s) for p, s in zip(ps, slow))
    assert [g["lookahead_step"] for g in look.param_groups] == [7]
    assert "lookahead_slow_buff" in look.state_dict()["state"][0]


# ---- the whole model -----------------------------------------------------------------------------------------------------
def _forward_backward(m, img, text):
    m.train()
    m.zero_grad()
    _, preds, _ = m(img, text[:, :-1])
    cost = torch.nn.functional.cross_entropy(preds.view(-1, preds.shape[-1]), text[:, 1:].contiguous().view(-1),
                                             ignore_index=0, reduction="none")
    cost.mean().backward()
    return preds.detach()


def _engine_holds_the_parameters(m):
    for name, p in m.named_parameters():
        raw = torch.empty_like(p, dtype=torch.float32).contiguous()
        m._engine.read_weight(name, raw)
        assert torch.equal(raw, p.detach()), name


def test_whole_model_lamb_step_refreshes_the_engine(cases):
    c = _case(cases, "train_step", "t2_train_step")
    _, m = engine_model(c["config"], c["max_seq_len"], c["wseed"])
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]).to(DEV)
    text = train_step_labels(c).to(DEV)
    opt = O.build_optimizer(m, opt="lamb", lr=1e-3, weight_decay=0.01, momentum=0.9, filter_bias_and_bn=True)
    assert isinstance(opt, O.FusedLamb) and opt.model is m
    _forward_backward(m, img, text)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    start = [p.detach().clone() for _, p in named]
    eng = m._engine
    uploads = eng.weight_uploads
    assert uploads >= 1
    versions = [p._version for _, p in named]
    opt.step()
    torch.cuda.synchronize()
    assert all(p._version > v for (_, p), v in zip(named, versions))
    assert sum(not torch.equal(p.detach(), s) for (_, p), s in zip(named, start)) > len(named) // 2
    _engine_holds_the_parameters(m)  # the engine's raw copies ARE the stepped parameters
    logits = _forward_backward(m, img, text)
    assert eng.weight_uploads == uploads  # neither the step nor the next training forward uploaded anything
    # a fresh model given the stepped state uploads the ordinary way and must compute the same bits
    sd = {k: v.detach().clone() for k, v in m.state_dict().items() if not k.endswith("image_positional_encoder.pe")}
    _, fresh = engine_model(c["config"], c["max_seq_len"], c["wseed"])
    fresh.load_state_dict(sd, strict=False)
    assert torch.equal(logits, _forward_backward(fresh, img, text))
    # Lookahead around it: the second synchronisation moves the weights, and the engine follows in the same launch
    look = O.Lookahead(opt, alpha=0.5, k=1)
    look.step()
    held = [p.detach().clone() for _, p in named]
    look.step()
    torch.cuda.synchronize()
    slow = [opt.state[p]["lookahead_slow_buff"] for _, p in named]
    assert all(torch.equal(p.detach(), s) for (_, p), s in zip(named, slow))
    assert any(not torch.equal(p.detach(), h) for (_, p), h in zip(named, held))
    _engine_holds_the_parameters(m)
    _forward_backward(m, img, text)
    assert eng.weight_uploads == uploads


# ---- the raw ABI ---------------------------------------------------------------------------------------------------------
def test_raw_abi_refusals():
    """Null and host pointers, negative sizes and bad scalars: D2T_EINVAL with a message, and nothing enqueued.  (A pointer of
    another device needs a second GPU: the check is d2t_optim_step's, shared.)"""
    lib = _lib.require_device()
    h = C.c_void_p()
    assert lib.d2t_optim_create(C.byref(h)) == 0
    try:
        n = 8
        p, g, a, b, c, mirror = (torch.ones(n, device=DEV) for _ in range(6))
        norm = torch.zeros((), device=DEV)
        mode = torch.zeros(1, dtype=torch.int32, device=DEV)
        host = (C.c_float * n)()
        stream = _lib.stream_of(p)
        P = lambda t: t.data_ptr()  # noqa: E731

        def lamb(grad=P(g), numel=n, lr=1e-3, bc1=0.1):
            return _lib.D2TOptimLambTensor(P(p), grad, P(a), P(b), P(mirror), numel, lr, 0.01, 0.9, 0.999, 0.1, 1e-6, bc1, 0.03, 1, 0)

        def adamp(grad=P(g), numel=n, rows=2, delta=0.1, m=P(a)):
            return _lib.D2TOptimAdampTensor(P(p), grad, m, P(b), P(mirror), P(mode), numel, rows, 1e-3, 0.01, 0.9, 0.999, 1e-8, 0.1,
                                            0.03, delta, 0.1, 1, 0)

        def madgrad(grad=P(g), numel=n, momentum=0.9, x0=P(c)):
            return _lib.D2TOptimMadgradTensor(P(p), grad, P(a), P(b), x0, P(mirror), numel, 1e-2, 0.0, momentum, 1e-6, 1e-2, 0, 0)

        def look(slow=P(a), numel=n):
            return _lib.D2TOptimLookaheadTensor(P(p), slow, P(mirror), numel)

        def call(fn, rec, count=1, mgn=1.0, norm_ptr=None):
            arr = (type(rec) * 1)(rec)
            if fn == "d2t_optim_lookahead_sync":
                rc = getattr(lib, fn)(h, arr, count, mgn, stream)
            else:
                rc = getattr(lib, fn)(h, arr, count, mgn, _lib.ptr(norm) if norm_ptr is None else norm_ptr, stream)
            return rc, lib.d2t_optim_last_error(h).decode()

        bad = [("d2t_optim_lamb_step", lamb(grad=C.addressof(host)), {}, "grad"), ("d2t_optim_lamb_step", lamb(grad=None), {}, "null"),
               ("d2t_optim_lamb_step", lamb(numel=-5), {}, "negative"), ("d2t_optim_lamb_step", lamb(bc1=0.0), {}, "scalars"),
               ("d2t_optim_lamb_step", lamb(lr=math.nan), {}, "scalars"), ("d2t_optim_lamb_step", lamb(), {"mgn": 0.0}, "max_grad_norm"),
               ("d2t_optim_lamb_step", lamb(), {"count": -1}, "-1"),
               ("d2t_optim_lamb_step", lamb(), {"norm_ptr": C.c_void_p(C.addressof(host))}, "norm"),
               ("d2t_optim_adamp_step", adamp(grad=C.addressof(host)), {}, "grad"), ("d2t_optim_adamp_step", adamp(m=None), {}, "null"),
               ("d2t_optim_adamp_step", adamp(rows=3), {}, "rows"), ("d2t_optim_adamp_step", adamp(delta=math.inf), {}, "scalars"),
               ("d2t_optim_adamp_step", adamp(), {"norm_ptr": C.c_void_p(C.addressof(host))}, "norm"),
               ("d2t_optim_madgrad_step", madgrad(grad=C.addressof(host)), {}, "grad"),
               ("d2t_optim_madgrad_step", madgrad(x0=None), {}, "null"), ("d2t_optim_madgrad_step", madgrad(momentum=1.0), {}, "scalars"),
               ("d2t_optim_madgrad_step", madgrad(numel=-1), {}, "negative"),
               ("d2t_optim_lookahead_sync", look(slow=C.addressof(host)), {}, "slow"), ("d2t_optim_lookahead_sync", look(slow=None), {}, "null"),
               ("d2t_optim_lookahead_sync", look(), {"mgn": 1.5}, "alpha"), ("d2t_optim_lookahead_sync", look(), {"count": -1}, "-1")]
        for fn, rec, kw, word in bad:
            rc, msg = call(fn, rec, **kw)
            assert rc == _lib.D2T_EINVAL and word in msg, (fn, word, rc, msg)
        torch.cuda.synchronize()
        ones = torch.ones(n, device=DEV)
        assert all(torch.equal(t, ones) for t in (p, g, a, b, c, mirror)) and float(norm) == 0.0  # nothing was launched
        # and each entry point accepts the well-formed record: parameter and mirror move together
        for fn, rec, kw in (("d2t_optim_lamb_step", lamb(), {}), ("d2t_optim_adamp_step", adamp(), {}),
                            ("d2t_optim_madgrad_step", madgrad(momentum=0.0, x0=None), {}), ("d2t_optim_lookahead_sync", look(), {"mgn": 0.5})):
            was = p.clone()
            if fn == "d2t_optim_lookahead_sync":
                a.fill_(3.0)
            rc, msg = call(fn, rec, **kw)
            assert rc == 0, (fn, msg)
            torch.cuda.synchronize()
            assert torch.equal(p, mirror) and not torch.equal(p, was), fn
            assert torch.equal(g, ones), fn
        assert torch.equal(p, a)  # Lookahead: fast, slow and mirror are equal bit for bit
        assert abs(float(norm) - n ** 0.5) <= 1e-6
    finally:
        lib.d2t_optim_destroy(h)
