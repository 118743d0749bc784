"""CPU: the float64 yardstick of the fused optimizer (tests/optim_refs.py) against torch.optim in float64, and everything of
doc2tex_amd.optim that needs no GPU -- the reference builder's parameter groups, state_dict interchange with torch.optim,
and the refusals.  No kernel runs here."""
import pytest
import torch

import optim_refs as OR
from doc2tex_amd import Model, synth
from doc2tex_amd import optim as O


@pytest.mark.parametrize("decoupled", [True, False])
def test_float64_reference_is_torchs_adam(decoupled):
    """Three steps of clip_grad_norm_(2.0) + torch.optim.AdamW / Adam in float64 against OR.adam_step: two groups (weight
    decay 0 and 0.01, different lr), tensors of 1 to 1000 elements; 1e-12 relative on p, m and v after every step."""
    gen = torch.Generator().manual_seed(7)
    sizes = [1, 2, 7, 64, 333, 1000]
    ps = [torch.randn(n, dtype=torch.float64, generator=gen).requires_grad_() for n in sizes]
    groups = [{"params": ps[:3], "weight_decay": 0.0, "lr": 3e-3}, {"params": ps[3:], "weight_decay": 0.01, "lr": 1e-2}]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(groups, betas=(0.9, 0.98), eps=1e-8, foreach=False)
    hyper = [(3e-3, 0.0)] * 3 + [(1e-2, 0.01)] * 3
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    clipped = 0
    for step in (1, 2, 3):
        grads = [torch.randn(n, dtype=torch.float64, generator=gen) * (0.02 if step == 2 else 1.0) for n in sizes]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        norm = OR.grad_norm(grads)
        total = torch.nn.utils.clip_grad_norm_(ps, 2.0)
        assert abs(float(total) - norm) <= 1e-12 * norm
        coef = OR.clip_coef(norm, 2.0)
        clipped += coef < 1.0
        opt.step()
        for i, (p, g) in enumerate(zip(ps, grads)):
            lr, wd = hyper[i]
            mine[i] = OR.adam_step(*mine[i][:1], g, *mine[i][1:], step, lr, (0.9, 0.98), 1e-8, wd, decoupled, coef)
            st = opt.state[p]
            for got, want in zip(mine[i], (p.detach(), st["exp_avg"], st["exp_avg_sq"])):
                assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300), (step, i)
    assert 0 < clipped < 3  # both sides of the clamp were exercised


def test_clip_coefficient_and_ulp():
    assert OR.clip_coef(10.0, 5.0) == 5.0 / (10.0 + 1e-6) and OR.clip_coef(1.0, 5.0) == 1.0
    assert OR.clip_coef(10.0, None) == 1.0 and OR.clip_coef(10.0, 0.0) == 1.0
    assert OR.ulp32(1.0) == 2.0 ** -23 and OR.ulp32(1.5) == 2.0 ** -23 and OR.ulp32(0.75) == 2.0 ** -24


def test_create_optimizer_groups_like_the_reference_builder():
    model = Model(synth.make_config("T2"))
    opt = O.create_optimizer(model, opt="adamw", lr=1e-4, weight_decay=2e-6, momentum=0.9, filter_bias_and_bn=True,
                             max_grad_norm=5.0)
    assert isinstance(opt, O.FusedAdamW) and opt.model is model and opt.max_grad_norm == 5.0
    assert opt.defaults["weight_decay"] == 0.0  # the groups carry it when filtering
    no_decay, decay = opt.param_groups
    assert no_decay["weight_decay"] == 0.0 and decay["weight_decay"] == 2e-6 and no_decay["lr"] == decay["lr"] == 1e-4
    named = dict(model.named_parameters())
    want_no = {n for n, p in named.items() if p.requires_grad and (p.dim() == 1 or n.endswith(".bias"))}
    want_dec = {n for n, p in named.items() if p.requires_grad} - want_no
    ids = {id(p): n for n, p in named.items()}
    assert {ids[id(p)] for p in no_decay["params"]} == want_no and {ids[id(p)] for p in decay["params"]} == want_dec
    assert want_no and want_dec
    frozen = [n for n, p in named.items() if not p.requires_grad]
    assert any(n.endswith("pos_embed") for n in frozen)
    assert not any(n.endswith("pos_embed") for n in want_no | want_dec)
    # no filtering: every parameter in one group that carries the decay; Adam by name, upper case and all
    opt = O.create_optimizer(model, opt="Adam", lr=1e-3, weight_decay=0.01, momentum=0.9, filter_bias_and_bn=False)
    assert isinstance(opt, O.FusedAdam) and len(opt.param_groups) == 1 and opt.param_groups[0]["weight_decay"] == 0.01
    assert len(opt.param_groups[0]["params"]) == len(named)
    kw = O.optimizer_kwargs({"opt": "adamw", "lr": 2e-4, "weight_decay": 2e-6, "momentum": 0.9, "opt_eps": 1e-6,
                             "opt_betas": (0.8, 0.9), "opt_args": None})
    assert kw == {"opt": "adamw", "lr": 2e-4, "weight_decay": 2e-6, "momentum": 0.9, "eps": 1e-6, "betas": (0.8, 0.9)}
    opt = O.create_optimizer(model, filter_bias_and_bn=True, **kw)
    assert all(g["eps"] == 1e-6 and g["betas"] == (0.8, 0.9) for g in opt.param_groups)
    assert "eps" not in O.optimizer_kwargs({"opt": "adamw", "lr": 1.0, "weight_decay": 0.0, "momentum": 0.9})
    assert isinstance(O.create_optimizer(model, "adadelta", 1.0, 0.0, 0.9, True), torch.optim.Adadelta)
    assert isinstance(O.create_optimizer(model, "adagrad", 1e-2, 0.0, 0.9, True, max_grad_norm=5.0), torch.optim.Adagrad)
    for name in ("adamp", "lamb", "madgrad", "lookahead_adamw"):
        with pytest.raises(NotImplementedError, match=name.split("_")[0]):
            O.create_optimizer(model, name, 1e-3, 0.0, 0.9, True)


def _shape_of(sd):
    return {"state": {k: {n: (type(v), v.dtype, v.device.type, tuple(v.shape)) for n, v in s.items()} for k, s in sd["state"].items()},
            "param_groups": [{k: type(v) for k, v in g.items()} for g in sd["param_groups"]]}


@pytest.mark.parametrize("pair", [(torch.optim.AdamW, O.FusedAdamW), (torch.optim.Adam, O.FusedAdam)])
def test_state_dict_moves_between_torch_and_fused(pair):
    tcls, fcls = pair
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    topt = tcls([{"params": ps[:1], "lr": 1e-2}, {"params": ps[1:], "weight_decay": 0.0}], lr=1e-3)
    for p in ps:
        p.grad = torch.randn_like(p)
    topt.step()
    topt.step()
    sd = topt.state_dict()
    fopt = fcls([{"params": ps[:1]}, {"params": ps[1:]}])
    for mine, theirs in zip(fopt.state_dict()["param_groups"], sd["param_groups"]):  # the same keys before any load, too
        assert set(mine) == set(theirs)
    fopt.load_state_dict(sd)
    got = fopt.state_dict()
    assert _shape_of(got) == _shape_of(sd)
    assert list(got["param_groups"][0]) == list(sd["param_groups"][0])
    for k, s in sd["state"].items():
        assert float(got["state"][k]["step"]) == 2.0 and got["state"][k]["step"].dtype == torch.float32
        assert torch.equal(got["state"][k]["exp_avg"], s["exp_avg"]) and torch.equal(got["state"][k]["exp_avg_sq"], s["exp_avg_sq"])
    assert fopt.param_groups[0]["lr"] == 1e-2 and fopt.param_groups[1]["weight_decay"] == 0.0
    back = tcls([{"params": ps[:1]}, {"params": ps[1:]}])
    back.load_state_dict(got)
    back.step()  # torch's own step runs on what the fused class saved
    assert float(back.state[ps[0]]["step"]) == 3.0


def test_refusals_without_a_gpu():
    p = torch.nn.Parameter(torch.randn(4))
    p.grad = torch.randn(4)
    opt = O.FusedAdamW([p])
    before = p.detach().clone()
    with pytest.raises(RuntimeError, match="ROCm"):
        opt.step()
    assert torch.equal(p.detach(), before)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        O.FusedAdamW([p], amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        O.FusedAdam([p], maximize=True)
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()
    adam = O.FusedAdam([p])
    adam.load_state_dict(torch.optim.AdamW([p]).state_dict())  # an AdamW checkpoint is not silently stepped as Adam
    with pytest.raises(NotImplementedError, match="decoupled"):
        adam.step()
