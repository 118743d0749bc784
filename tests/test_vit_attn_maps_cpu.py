"""CPU: the ViT encoder's attn_drop modules (the reference's hook points for attention rollout,
tools/interpretation/vit_visualize.py:26-93) -- their module names against the reference's, the unchanged parameter tree,
their absence from the other encoders, and the internal consistency of the reference map fixtures
(tests/golden/vitattn_*.npz, written by tools/make_golden_vit_attn.py).  No GPU needed."""
import json
import os

import numpy as np
import pytest
import torch.nn as nn

from conftest import GOLD
from doc2tex_amd import Model, synth

with open(os.path.join(GOLD, "vitattn_cases.json")) as f:
    VA = json.load(f)
CASES = {c["case"]: c for c in VA["cases"]}
VIT_CONFIGS = sorted({c["config"] for c in VA["cases"]})
NON_VIT = ["C0", "B0", "C1", "T1"]  # VGG + BiLSTM, ResNet + None (TFM)


def _load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _model(cname):
    return Model(synth.make_config(cname, device="cpu"))


@pytest.mark.parametrize("cname", VIT_CONFIGS)
def test_attn_drop_modules_at_reference_names(cname):
    want = next(c["attn_drop_modules"] for c in VA["cases"] if c["config"] == cname)
    m = _model(cname)
    got = [n for n, _ in m.named_modules() if "attn_drop" in n]
    assert got == want
    assert want == [f"seqmodeler.SequenceModeling.blocks.{i}.attn.attn_drop" for i in range(len(want))]
    for n in got:
        mod = m.get_submodule(n)
        assert isinstance(mod, nn.Dropout) and mod.p == 0.0


@pytest.mark.parametrize("cname", VIT_CONFIGS)
def test_state_dict_unchanged(cname, manifests):
    """Dropout holds no state: the parameter tree is still the reference's (manifests.json)."""
    sd = _model(cname).state_dict()
    got = {k: list(v.shape) for k, v in sd.items() if not k.endswith("image_positional_encoder.pe")}
    want = {k: v for k, v in manifests[cname].items() if not k.endswith("image_positional_encoder.pe")}
    assert got == want


@pytest.mark.parametrize("cname", NON_VIT)
def test_non_vit_stacks_have_no_attn_drop(cname):
    m = _model(cname)
    assert m.stages["Seq"] != "ViT"
    assert not [n for n, _ in m.named_modules() if "attn_drop" in n]
    assert m._hooked_attn_drops() == []


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] == "full"])
def test_full_fixtures_are_softmax_rows(name):
    c, z = CASES[name], _load(name)
    p = z["maps"].astype(np.float64)
    assert p.shape == (c["depth"], c["B"], c["heads"], c["T"], c["T"])
    assert (p >= 0).all()
    assert np.abs(p.sum(-1) - 1).max() <= 1e-5


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["kind"] == "sampled"])
def test_sampled_fixtures_are_self_consistent(name):
    c, z = CASES[name], _load(name)
    rows, T = c["rows"], c["T"]
    assert rows == [0, T // 3, (2 * T) // 3, T - 1]
    r = z["rows"].astype(np.float64)
    assert r.shape == (c["depth"], c["B"], c["heads"], len(rows), T)
    assert np.abs(r.sum(-1) - 1).max() <= 1e-5
    assert z["argmax"].shape == z["max"].shape == (c["depth"], c["B"], c["heads"], T)
    assert np.array_equal(r.argmax(-1), z["argmax"][..., rows])
    assert np.array_equal(r.max(-1), z["max"][..., rows].astype(np.float64))
    assert ((z["max"] > 0) & (z["max"] <= 1)).all() and (z["argmax"] >= 0).all() and (z["argmax"] < T).all()
