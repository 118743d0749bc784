"""CPU: the criteria of doc2tex_amd.loss beyond the plain cross-entropy -- CrossEntropyLoss(weight=, label_smoothing=) and
LabelSmoothingLoss -- as far as they go without a device: constructors, criterion_kwargs, every refusal, and a float64
restatement of both formulas (reused by tests/test_criterion_gpu.py) against the reference's own numbers in
tests/golden/loss_smooth.npz (tools/make_golden_loss.py: the reference's LabelSmoothingLoss, fp32 on the CPU).

Bounds of the restatement against the fixtures, max |restated - fixture| over max |fixture|: 1e-6 for the losses and for the
gradients at V <= 1025, 2e-5 for the gradients at V = 16384 (the reference's own fp32 result sits 7e-6 from float64 there,
about 1e-7 everywhere else).
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD
from doc2tex_amd.loss import CrossEntropyLoss, LabelSmoothingLoss, create_criterion, criterion_kwargs

with open(os.path.join(GOLD, "loss_smooth.json")) as f:
    SMOOTH_CASES = json.load(f)
SMOOTH_IDS = [c["name"] for c in SMOOTH_CASES]


def smooth_case_inputs(c):
    """Logits [rows, V] (3 * N(0, 1), as test_fused_cross_entropy draws them), targets, and the upstream gradient of the
    per-row losses, all from the case's seed.  No live row hits the padding index by chance; `pad_rows` says which rows do."""
    g = torch.Generator().manual_seed(c["seed"])
    rows, V, pad = c["rows"], c["V"], c["pad"]
    x = torch.randn(rows, V, generator=g) * 3.0
    t = torch.randint(0, V, (rows,), generator=g)
    t[t == pad] = (pad + 1) % V
    if c["pad_rows"] == "fifth":
        t[::5] = pad
    elif c["pad_rows"] == "one":
        t[rows // 2] = pad
    elif c["pad_rows"] == "all":
        t[:] = pad
    else:
        assert c["pad_rows"] == "none"
    up = torch.rand(rows, generator=g) + 0.5
    return x, t, up


def smooth_restated(x, target, classes, pad, smoothing, reduction):
    """LabelSmoothingLoss as a formula, in x's dtype and on x's device: 1 - smoothing on the target, smoothing / (classes - 2)
    on every class but the target and the padding column, nothing on a row whose target is the padding index; per row for a
    truthy `reduction`, the mean over all rows otherwise."""
    cols = torch.arange(x.shape[1], device=x.device)
    hit = cols[None, :] == target[:, None]
    mass = hit.to(x.dtype) * (1.0 - smoothing) + (~hit & (cols != pad)[None, :]).to(x.dtype) * (smoothing / (classes - 2))
    mass = mass * (target != pad)[:, None]
    loss = -(mass * torch.log_softmax(x, -1)).sum(-1)
    return loss if reduction else loss.mean()


def torch_restated(x, target, weight, ignore_index, eps, reduction):
    """nn.CrossEntropyLoss(weight, ignore_index, label_smoothing = eps) as a formula: (1 - eps) * w[t] on the target plus
    eps / V * w[v] on every class; 'mean' divides by the weights of the live rows' targets."""
    V = x.shape[1]
    w = torch.ones(V, dtype=x.dtype, device=x.device) if weight is None else weight.to(x.dtype)
    live = target != ignore_index
    t = target.clamp(0, V - 1)
    mass = F.one_hot(t, V).to(x.dtype) * ((1.0 - eps) * w[t])[:, None] + (eps / V) * w[None, :]
    loss = -(mass * torch.log_softmax(x, -1)).sum(-1) * live
    if reduction == "none":
        return loss
    return loss.sum() if reduction == "sum" else loss.sum() / (w[t] * live).sum()


def smooth_restated_grad(c, dtype=torch.float64, device="cpu"):
    """(loss, d/dx) of the case: per-row losses against the seeded upstream gradient, the scalar against 1."""
    x, t, up = smooth_case_inputs(c)
    x = x.to(device=device, dtype=dtype).requires_grad_(True)
    out = smooth_restated(x, t.to(device), c["classes"], c["pad"], c["smoothing"], c["reduction"])
    if c["reduction"]:
        (out * up.to(device=device, dtype=dtype)).sum().backward()
    else:
        out.backward()
    return out.detach(), x.grad


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "loss_smooth.npz"))


def test_case_list_covers_the_shapes():
    shapes = {(c["rows"], c["V"]) for c in SMOOTH_CASES}
    assert shapes == {(37, 93), (5, 1025), (4, 11), (24, 16384), (8, 500), (64, 1000)}
    assert {c["classes"] for c in SMOOTH_CASES if c["V"] == 11} == {11, 9}
    assert [c["reduction"] for c in SMOOTH_CASES if c["V"] == 1000] == ["none", "mean", "", None]
    assert {c["pad_rows"] for c in SMOOTH_CASES if c["V"] == 500} == {"none", "all"}
    assert any(c["smoothing"] == 0 for c in SMOOTH_CASES)
    for c in SMOOTH_CASES:
        _, t, _ = smooth_case_inputs(c)
        n = int((t == c["pad"]).sum())
        assert n == {"fifth": -(-c["rows"] // 5), "one": 1, "none": 0, "all": c["rows"]}[c["pad_rows"]], c["name"]


@pytest.mark.parametrize("c", SMOOTH_CASES, ids=SMOOTH_IDS)
def test_restatement_reproduces_the_reference_fixture(golden, c):
    want, gwant, gi = golden[c["name"] + ":loss"], golden[c["name"] + ":grad"], golden[c["name"] + ":gi"]
    _, t, _ = smooth_case_inputs(c)
    assert gwant.shape == (64,) and gi.shape == (64, 2)
    rows_in = set(gi[:, 0].tolist())
    for r in rows_in:  # every sampled row brings its target and its padding column
        cols = set(gi[gi[:, 0] == r, 1].tolist())
        assert int(t[r]) in cols and c["pad"] in cols
    loss, grad = smooth_restated_grad(c)
    assert loss.shape == (() if not c["reduction"] else (c["rows"],)) and tuple(want.shape) == tuple(loss.shape)
    err = float(np.abs(loss.numpy() - want).max())
    assert err <= 1e-6 * max(float(np.abs(want).max()), 1e-30), err
    got = grad[torch.from_numpy(gi[:, 0]).long(), torch.from_numpy(gi[:, 1]).long()].numpy()
    tol = 2e-5 if c["V"] == 16384 else 1e-6
    gerr = float(np.abs(got - gwant).max())
    print(f"[{c['name']}] loss err {err:.2e} of {float(np.abs(want).max()):.3g}; grad err {gerr:.2e} of {float(np.abs(gwant).max()):.3g}")
    assert gerr <= tol * max(float(np.abs(gwant).max()), 1e-30), gerr
    if c["pad_rows"] == "all":
        assert float(np.abs(want).max()) == 0.0 and float(np.abs(gwant).max()) == 0.0


def test_smoothing_zero_is_plain_cross_entropy():
    c = next(c for c in SMOOTH_CASES if c["smoothing"] == 0)
    x, t, _ = smooth_case_inputs(c)
    loss = smooth_restated(x.double(), t, c["classes"], c["pad"], 0.0, "none")
    ref = F.cross_entropy(x.double(), t, ignore_index=c["pad"], reduction="none")
    assert float((loss - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("weighted,eps", [(True, 0.0), (False, 0.1), (True, 0.1), (False, 0.0)])
def test_torch_mode_restatement_is_torchs_criterion(weighted, eps, reduction):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(37, 93, generator=g) * 3.0).double()
    t = torch.randint(1, 93, (37,), generator=g)
    t[::5] = 0
    w = (torch.rand(93, generator=g) + 0.5).double() if weighted else None
    ref = F.cross_entropy(x, t, weight=w, ignore_index=0, label_smoothing=eps, reduction=reduction)
    out = torch_restated(x, t, w, 0, eps, reduction)
    assert float((out - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_cross_entropy_constructor():
    crit = CrossEntropyLoss(weight=[0.5, 1.0, 2.0], ignore_index=0, reduction="none", label_smoothing=0.1)
    assert crit.ignore_index == 0 and crit.reduction == "none" and crit.label_smoothing == 0.1
    assert crit.weight.dtype == torch.float32 and crit.weight.tolist() == [0.5, 1.0, 2.0]
    assert "weight" in dict(crit.named_buffers()) and not list(crit.parameters())  # criterion.to(device) moves it
    w = torch.tensor([1.0, 2.0], dtype=torch.float64)
    crit = CrossEntropyLoss(weight=w)
    w[0] = 7.0
    assert crit.weight.tolist() == [1.0, 2.0] and crit.ignore_index == -100 and crit.reduction == "mean"
    assert CrossEntropyLoss().weight is None and CrossEntropyLoss().label_smoothing == 0.0
    for eps in (0.0, 1.0):
        assert CrossEntropyLoss(label_smoothing=eps).label_smoothing == eps
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            CrossEntropyLoss(label_smoothing=bad)
    with pytest.raises(ValueError):
        CrossEntropyLoss(reduction="average")
    with pytest.raises(ValueError):
        CrossEntropyLoss(weight=torch.ones(2, 3))
    with pytest.raises(NotImplementedError):
        CrossEntropyLoss(size_average=True)
    with pytest.raises(NotImplementedError):
        CrossEntropyLoss(reduce=False)


def test_label_smoothing_loss_constructor_mirrors_the_reference():
    crit = LabelSmoothingLoss("none", 500, 0, smoothing=0.1)
    assert (crit.confidence, crit.smoothing, crit.cls, crit.dim, crit.padding_idx, crit.reduction) == (0.9, 0.1, 500, -1, 0, "none")
    crit = LabelSmoothingLoss(reduction=None, classes=11, ignore_index=2, smoothing=0.25, dim=1)
    assert (crit.confidence, crit.smoothing, crit.cls, crit.dim, crit.padding_idx, crit.reduction) == (0.75, 0.25, 11, 1, 2, None)
    assert LabelSmoothingLoss("none", 5, 0).smoothing == 0.0 and LabelSmoothingLoss("none", 5, 0).confidence == 1.0
    assert not list(crit.parameters()) and not list(crit.buffers())


def test_label_smoothing_loss_refusals():
    x, t = torch.zeros(4, 11), torch.ones(4, dtype=torch.long)
    with pytest.raises(ZeroDivisionError):
        LabelSmoothingLoss("none", 2, 0, smoothing=0.1)(x, t)
    for pad in (11, 500, -1):
        with pytest.raises(IndexError):
            LabelSmoothingLoss("none", 11, pad, smoothing=0.1)(x, t)
    for dim in (0, 2, -2):
        with pytest.raises(NotImplementedError):
            LabelSmoothingLoss("none", 11, 0, smoothing=0.1, dim=dim)(x, t)
    with pytest.raises(RuntimeError):  # CPU logits: no eager fallback
        LabelSmoothingLoss("none", 11, 0, smoothing=0.1)(x, t)


def test_cpu_logits_are_refused_with_weight_or_smoothing():
    x, t = torch.zeros(4, 11), torch.ones(4, dtype=torch.long)
    for kw in ({"weight": torch.ones(11)}, {"label_smoothing": 0.1}, {}):
        with pytest.raises(RuntimeError):
            CrossEntropyLoss(ignore_index=0, reduction="none", **kw)(x, t)
    with pytest.raises(ValueError):  # one weight per class
        CrossEntropyLoss(weight=torch.ones(10))(x, t)
    with pytest.raises(TypeError):  # criterion.double() converts the buffer; the kernels read float32
        CrossEntropyLoss(weight=torch.ones(11)).double()(x, t)


def test_criterion_kwargs_on_the_three_configuration_forms():
    assert criterion_kwargs({"name": "entropy", "ignore_index": 0, "reduction": "none"}) == {"ignore_index": 0, "reduction": "none"}
    w = torch.ones(5)
    kw = criterion_kwargs({"name": "entropy", "ignore_index": 0, "reduction": "none", "weight": w, "loss_args": None})
    assert set(kw) == {"ignore_index", "reduction", "weight"} and kw["weight"] is w
    kw = criterion_kwargs({"name": "entropy", "ignore_index": 0, "reduction": "none", "weight": None,
                           "loss_args": {"label_smoothing": 0.1}})
    assert kw == {"ignore_index": 0, "reduction": "none", "label_smoothing": 0.1}
    crit = create_criterion("entropy", kw)
    assert isinstance(crit, CrossEntropyLoss) and crit.label_smoothing == 0.1 and crit.ignore_index == 0
    kw = criterion_kwargs({"name": "smooth", "ignore_index": 0, "reduction": "none", "loss_args": {"classes": 500, "smoothing": 0.1}})
    assert kw == {"ignore_index": 0, "reduction": "none", "classes": 500, "smoothing": 0.1}
    crit = LabelSmoothingLoss(**kw)  # the one line to change while "smooth" is not routed by name
    assert crit.cls == 500 and crit.padding_idx == 0 and crit.reduction == "none"
    kw = criterion_kwargs({"ignore_index": 0, "reduction": "mean", "loss_args": {"reduction": "sum"}})  # loss_args win
    assert kw == {"ignore_index": 0, "reduction": "sum"}
    with pytest.raises(KeyError):
        criterion_kwargs({"reduction": "none"})


def test_create_criterion_passes_weight_and_smoothing_through():
    crit = create_criterion("entropy", {"ignore_index": 0, "reduction": "sum", "weight": torch.ones(7), "label_smoothing": 0.2})
    assert isinstance(crit, CrossEntropyLoss) and crit.weight.numel() == 7 and crit.label_smoothing == 0.2 and crit.reduction == "sum"
    with pytest.raises(NotImplementedError, match=r"doc2tex_amd\.loss\.LabelSmoothingLoss"):
        create_criterion("smooth", {"reduction": "none", "classes": 500, "ignore_index": 0, "smoothing": 0.1})
    with pytest.raises(NotImplementedError):
        create_criterion("focal", {})
