"""Shared by tests/test_stacks_cpu.py and tests/test_stacks_gpu.py: the fixtures of tools/make_golden_stacks.py (the
Feat x Seq x Pred pairings beside the ones tests/golden/cases.json covers) and float64 / float32 statements of proj_feat."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLD

L = 16  # max_seq_len / batch_max_length of every fixture
TFM_GREEDY = ["vbt_greedy_b2", "vbt_greedy_b5", "rbt_greedy_b2", "rbt_greedy_b5", "vt_greedy_h32", "vt_greedy_h64",
              "vbtp_greedy", "rbtp_greedy"]
ATTN_GREEDY = ["vbap_greedy_b2", "vbap_greedy_b5", "rbap_greedy_b2", "rbap_greedy_b5"]
# the smallest top-2 logit gap a fixture may have for its tokens to be decided inside the 1e-3 logit bar: two logits that
# move by at most 1e-3 each cannot swap when they lie 2e-3 apart (tools/make_golden_stacks.py MIN_GAP)
MIN_GAP = 2e-3

_CACHE = {}


def stack_cases():
    if "cases" not in _CACHE:
        with open(os.path.join(GOLD, "stacks_cases.json")) as f:
            _CACHE["cases"] = json.load(f)
    return _CACHE["cases"]


def stack_manifests():
    if "man" not in _CACHE:
        with open(os.path.join(GOLD, "stacks_manifests.json")) as f:
            _CACHE["man"] = json.load(f)
    return _CACHE["man"]


def stack_case(kind, name):
    return next(c for c in stack_cases()[kind] if c["case"] == name)


def stack_arrays(name):
    """The arrays of one fixture, loaded once and never written to."""
    if name not in _CACHE:
        with np.load(os.path.join(GOLD, "stacks_" + name + ".npz")) as z:
            _CACHE[name] = {k: z[k] for k in z.files}
    return _CACHE[name]


# ---- proj_feat (recognizers/build_feat.py:38-40,56-61) -------------------------------------------------------------
def proj_feat_linear(feat_nchw, w, b):
    """As the reference writes it: Linear(3C -> C) over feature.permute(0, 3, 1, 2).flatten(-2), [b, w, c * h] -> [b, w, C]."""
    return F.linear(feat_nchw.permute(0, 3, 1, 2).flatten(start_dim=-2), w, b)


def proj_feat_conv(feat_nchw, w, b):
    """As the engine runs it: weight.view(C, C, 3, 1) is the OIHW filter of a (3, 1) convolution, stride 1, no padding;
    [b, C, 3, w] -> [b, C, 1, w] -> [b, w, C]."""
    C = w.shape[0]
    return F.conv2d(feat_nchw, w.view(C, C, 3, 1), b)[:, :, 0].transpose(1, 2)


def proj_feat_taps(feat_nchw, w, b):
    """A third order of the same sums: one matrix product per height, added up."""
    C = w.shape[0]
    w3 = w.view(C, C, 3)
    y = b.expand(feat_nchw.shape[0], feat_nchw.shape[3], C).clone()
    for h in range(3):
        y = y + feat_nchw[:, :, h].transpose(1, 2) @ w3[:, :, h].t()
    return y


PROJ_FORMS = (proj_feat_linear, proj_feat_conv, proj_feat_taps)


def proj_feat_case(B, Wp, C=512, seed=0):
    """Seeded float32 operands of one proj_feat call: the feature map [B, C, 3, W'], weight [C, 3C], bias [C] and an upstream
    gradient [B, W', C]."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * Wp + B)
    x = torch.randn(B, C, 3, Wp, generator=g)
    w = torch.randn(C, 3 * C, generator=g) * (2.0 / (4 * C)) ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    dy = torch.randn(B, Wp, C, generator=g)
    return x, w, b, dy


def proj_feat_refs(x, w, b, dy):
    """(y64, e32): the float64 forward, data gradient, weight gradient and bias gradient, and per output the largest
    max |y32 - y64| over the three float32 forms evaluated by autograd (the measured rule of DESIGN.md section 5.3a)."""
    def run(form, dt):
        xs, ws, bs = (t.to(dt).requires_grad_(True) for t in (x, w, b))
        y = form(xs, ws, bs)
        dx, dw, db = torch.autograd.grad(y, [xs, ws, bs], dy.to(dt))
        return {"y": y.detach(), "dx": dx, "dw": dw, "db": db}
    y64 = run(proj_feat_linear, torch.float64)
    e32 = {k: 0.0 for k in y64}
    for form in PROJ_FORMS:
        y32 = run(form, torch.float32)
        for k in y64:
            e32[k] = max(e32[k], float((y32[k].double() - y64[k]).abs().max()))
    return y64, e32
