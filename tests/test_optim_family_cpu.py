"""CPU: the float64 restatements of LAMB, AdamP, MADGRAD and Lookahead (tests/optim_family_refs.py) against fixtures recorded
from the reference's own classes (tests/golden/optim_family.*, tools/make_golden_optim.py), and everything of the new
classes of doc2tex_amd.optim that needs no GPU: arguments, groups, state-dict structure, the builder and the refusals.  No
kernel runs here."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import optim_family_refs as FR
from conftest import ROOT
from doc2tex_amd import Model, synth
from doc2tex_amd import optim as O

GOLDEN = os.path.join(ROOT, "tests", "golden", "optim_family")
FUSED = {"Lamb": O.FusedLamb, "AdamP": O.FusedAdamP, "MADGRAD": O.FusedMADGRAD}
SIZES = [math.prod(shape) for shape, _ in FR.FIXTURE_TENSORS]


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN + ".json") as f:
        header = json.load(f)
    return header, dict(np.load(GOLDEN + ".npz"))


def _split(vector, indices):
    """The flat vector of the tensors `indices` (in order) -> {index: float64 tensor of its shape}."""
    out, at = {}, 0
    for i in indices:
        out[i] = torch.from_numpy(vector[at:at + SIZES[i]].copy()).reshape(FR.FIXTURE_TENSORS[i][0])
        at += SIZES[i]
    assert at == len(vector)
    return out


def _restated(name):
    """The case `name` by the float64 restatements: (final parameters, final state per tensor, AdamP modes and margins per
    step)."""
    cls, args, overrides, look = FR.FIXTURE_CASES[name]
    header, _ = _golden()
    defaults = dict(header["classes"][cls]["defaults"], **args)
    ps = FR.fixture_start()
    hyper = [dict(defaults, **overrides[i >= FR.FIXTURE_SPLIT]) for i in range(len(ps))]
    state = [None] * len(ps)
    modes, margins = [], []
    for step in range(1, FR.FIXTURE_STEPS + 1):
        gs = FR.fixture_grads(ps, step)
        if cls == "Lamb":
            # the reference keeps its global norm and max_grad_norm in float32 tensors whatever the gradients' dtype, and
            # the fixtures carry that rounding: the divisor is formed from a norm accumulated the same way
            acc = torch.zeros(1)
            for g in gs:
                if g is not None:
                    acc.add_((g * g).sum())
            divisor = FR.lamb_divisor(float(acc.sqrt()), float(torch.tensor(defaults["max_grad_norm"])))
            divisor = float(torch.tensor(divisor))
        row, mrow = [], []
        for i, (p, g, h) in enumerate(zip(ps, gs, hyper)):
            if g is None:
                row.append(0)
                continue
            zeros = torch.zeros_like(p)
            if cls == "Lamb":
                st = state[i] or {"exp_avg": zeros, "exp_avg_sq": zeros.clone()}
                ps[i], st["exp_avg"], st["exp_avg_sq"] = FR.lamb_step(
                    p, g, st["exp_avg"], st["exp_avg_sq"], step, h["lr"], h["betas"], h["eps"], h["weight_decay"], divisor,
                    h["bias_correction"], h["grad_averaging"], h["trust_clip"], h["always_adapt"])
            elif cls == "AdamP":
                st = state[i] or {"exp_avg": zeros, "exp_avg_sq": zeros.clone()}
                ps[i], st["exp_avg"], st["exp_avg_sq"], mode, margin = FR.adamp_step(
                    p, g, st["exp_avg"], st["exp_avg_sq"], step, h["lr"], h["betas"], h["eps"], h["weight_decay"], h["delta"],
                    h["wd_ratio"], h["nesterov"])
                row.append(mode)
                mrow.append(margin)
            else:
                st = state[i] or dict({"grad_sum_sq": zeros, "s": zeros.clone()}, **({"x0": p.clone()} if h["momentum"] else {}))
                ps[i], st["grad_sum_sq"], st["s"] = FR.madgrad_step(
                    p, g, st["grad_sum_sq"], st["s"], st.get("x0"), step, h["lr"], h["momentum"], h["eps"], h["weight_decay"],
                    h["decoupled_decay"])
            if cls != "Lamb":
                st["step"] = step
            state[i] = st
            if look and step % look["k"] == 0:
                slow = st.get("lookahead_slow_buff", ps[i])  # created as a copy of the fast weights: the first one is a no-op
                ps[i] = st["lookahead_slow_buff"] = FR.lookahead_sync(ps[i], slow, look["alpha"])
        modes.append(row)
        margins.append(mrow)
    return ps, state, modes, margins


def _close(got, want, what):
    scale = max(float(want.abs().max()), 1e-300)
    assert float((got - want).abs().max()) <= 1e-12 * scale, what


@pytest.mark.parametrize("name", sorted(FR.FIXTURE_CASES))
def test_float64_restatements_reproduce_the_reference(name):
    """13 steps of the reference's class (float64, CPU; two groups; a tensor without a gradient, one with a zero gradient, an
    all-zero row) against the restatements: 1e-12 relative on every parameter and state tensor, scalar state and AdamP's
    decisions exactly."""
    header, arrays = _golden()
    case = header["cases"][name]
    ps, state, modes, _ = _restated(name)
    assert header["steps"] == FR.FIXTURE_STEPS
    want_p = _split(arrays[f"{name}/p"], range(len(ps)))
    for i, p in enumerate(ps):
        _close(p, want_p[i], (name, "p", i))
    assert torch.equal(ps[FR.FIXTURE_NO_GRAD], FR.fixture_start()[FR.FIXTURE_NO_GRAD])
    with_state = sorted(int(i) for i in case["state_keys"])
    assert with_state == [i for i in range(len(ps)) if i != FR.FIXTURE_NO_GRAD]
    keys = {k for i in with_state for k in case["state_keys"][str(i)]}
    for k in sorted(keys):
        have = [i for i in with_state if k in case["state_keys"][str(i)]]
        if f"{name}/{k}" in arrays:
            want = _split(arrays[f"{name}/{k}"], have)
            for i in have:
                _close(state[i][k], want[i], (name, k, i))
        else:
            for i in have:
                assert state[i][k] == case["state_scalars"][str(i)][k], (name, k, i)
    for i in with_state:
        assert sorted(state[i]) == case["state_keys"][str(i)]
    if FR.FIXTURE_CASES[name][0] == "AdamP":
        assert modes == case["modes"]
        assert {m for row in modes for m in row} == {0, 1, 2}  # every branch was taken


@pytest.mark.parametrize("name", [n for n, c in FR.FIXTURE_CASES.items() if c[0] == "AdamP"])
def test_adamp_fixture_decisions_have_margin(name):
    """A condition on the inputs: every comparison behind a decision is at least 25 % of its threshold away from it, so no
    fp32 reduction order can flip one."""
    _, _, _, margins = _restated(name)
    worst = min(m for row in margins for m in row)
    print(f"[optim] {name}: smallest AdamP decision margin {worst:.3f}")
    assert worst >= 0.25


def _params():
    return [torch.nn.Parameter(torch.zeros(shape)) for shape, _ in FR.FIXTURE_TENSORS]


@pytest.mark.parametrize("cls", sorted(FUSED))
def test_defaults_groups_and_state_dict_are_the_references(cls):
    header, arrays = _golden()
    want = header["classes"][cls]
    plain = lambda d: {k: list(v) if isinstance(v, tuple) else v for k, v in d.items()}  # noqa: E731
    opt = FUSED[cls](_params())
    assert plain(opt.defaults) == want["defaults"] and list(opt.defaults) == [k for k in want["group_keys"] if k != "params"]
    assert list(opt.param_groups[0]) == want["group_keys"]
    # the reference's state_dict after 13 steps loads, and comes out with the same structure
    name = next(n for n, c in FR.FIXTURE_CASES.items() if c[0] == cls and c[3] is None)
    case = header["cases"][name]
    sd = {"param_groups": case["param_groups"], "state": {}}
    for i, keys in case["state_keys"].items():
        have = lambda k: [int(j) for j in sorted(case["state_keys"], key=int) if k in case["state_keys"][j]]  # noqa: E731
        sd["state"][int(i)] = {k: _split(arrays[f"{name}/{k}"], have(k))[int(i)].float() if f"{name}/{k}" in arrays
                               else case["state_scalars"][i][k] for k in keys}
    ps = _params()
    opt = FUSED[cls](FR.fixture_groups(ps, ({}, {})))
    opt.load_state_dict(sd)
    got = opt.state_dict()
    assert [sorted(g) for g in got["param_groups"]] == [sorted(g) for g in case["param_groups"]]
    assert {str(i): sorted(st) for i, st in got["state"].items()} == case["state_keys"]
    for i, st in got["state"].items():
        for k, v in st.items():
            assert type(v) is type(sd["state"][i][k]) and (not isinstance(v, torch.Tensor) or torch.equal(v, sd["state"][i][k]))
    if cls == "Lamb":
        assert [g["step"] for g in opt.param_groups] == [FR.FIXTURE_STEPS] * 2


def test_lookahead_wraps_like_the_reference():
    header, _ = _golden()
    want = header["classes"]["Lookahead"]
    base = O.FusedLamb(_params())
    look = O.Lookahead(base)
    assert look.param_groups is base.param_groups and look.defaults is base.defaults
    assert list(look.param_groups[0]) == want["group_keys"]
    assert {k: list(v) if isinstance(v, tuple) else v for k, v in look.defaults.items()} == want["defaults"]
    assert look.state_dict()["param_groups"][0]["lookahead_k"] == 6
    case = header["cases"]["lookahead_lamb"]
    assert all("lookahead_slow_buff" in keys for keys in case["state_keys"].values())
    assert [g["lookahead_step"] for g in case["param_groups"]] == [FR.FIXTURE_STEPS] * 2
    with pytest.raises(ValueError, match="slow update rate"):
        O.Lookahead(base, alpha=1.5)
    with pytest.raises(ValueError, match="lookahead steps"):
        O.Lookahead(base, k=0)
    wrapped = O.Lookahead(torch.optim.SGD(_params(), lr=0.1), alpha=0.25, k=3)  # any optimizer
    assert wrapped.param_groups[0]["lookahead_alpha"] == 0.25 and wrapped.param_groups[0]["lookahead_k"] == 3


def test_build_optimizer_is_the_references_builder():
    model = Model(synth.make_config("T2"))
    build = functools.partial(O.build_optimizer, model, lr=1e-3, weight_decay=0.01, momentum=0.7, filter_bias_and_bn=True)
    want = {"adam": O.FusedAdam, "adamw": O.FusedAdamW, "adamp": O.FusedAdamP, "lamb": O.FusedLamb, "madgrad": O.FusedMADGRAD,
            "adadelta": torch.optim.Adadelta, "adagrad": torch.optim.Adagrad}
    for name, cls in want.items():
        opt = build(opt=name)
        assert type(opt) is cls, name
        no_decay, decay = opt.param_groups
        assert no_decay["weight_decay"] == 0.0 and decay["weight_decay"] == 0.01 and decay["lr"] == 1e-3
        assert opt.defaults["weight_decay"] == 0.0
        if cls.__module__ == O.__name__:
            assert opt.model is model
        look = build(opt="lookahead_" + name.upper())
        assert type(look) is O.Lookahead and type(look._base_optimizer) is cls
        assert look.param_groups[0]["lookahead_alpha"] == 0.5 and look.param_groups[0]["lookahead_k"] == 6
    adamp = build(opt="adamp", max_grad_norm=5.0)
    assert adamp.defaults["wd_ratio"] == 0.01 and adamp.defaults["nesterov"] is True and adamp.max_grad_norm == 5.0
    assert build(opt="madgrad").defaults["momentum"] == 0.7
    assert build(opt="lamb", max_grad_norm=2.0).defaults["max_grad_norm"] == 2.0  # LAMB's own clip
    assert build(opt="lamb").defaults["max_grad_norm"] == 1.0
    assert isinstance(build(opt="adagrad", max_grad_norm=5.0), torch.optim.Adagrad)  # torch's do not clip: dropped
    one = O.build_optimizer(model, "lamb", 1e-3, 0.01, 0.9, False)
    assert len(one.param_groups) == 1 and one.param_groups[0]["weight_decay"] == 0.01
    with pytest.raises(NotImplementedError, match="sgd"):
        build(opt="sgd")


def test_create_optimizer_still_refuses_and_names_the_way_out():
    model = Model(synth.make_config("T2"))
    for name in ("adamp", "lamb", "madgrad", "lookahead_adamw"):
        with pytest.raises(NotImplementedError, match="build_optimizer"):
            O.create_optimizer(model, name, 1e-3, 0.0, 0.9, True)


@pytest.mark.parametrize("cls", sorted(FUSED))
def test_step_on_cpu_parameters_raises(cls):
    p = torch.nn.Parameter(torch.randn(4, 3))
    p.grad = torch.randn(4, 3)
    before = p.detach().clone()
    opt = FUSED[cls]([p])
    with pytest.raises(RuntimeError, match="ROCm"):
        opt.step()
    with pytest.raises(RuntimeError, match="ROCm"):
        O.Lookahead(torch.optim.SGD([p], lr=0.0), k=1).step()
    assert torch.equal(p.detach(), before)
    # a refused step counts nothing: neither LAMB's group count nor a parameter's
    assert "step" not in opt.param_groups[0] and all(st.get("step", 0) == 0 for st in opt.state.values())
    assert opt.projection_modes() is None if cls == "AdamP" else True
    with pytest.raises(ValueError):
        O.FusedMADGRAD([p], momentum=1.0)
