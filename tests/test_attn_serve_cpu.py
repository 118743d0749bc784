"""CPU: the fixtures of the pipelined LSTM-attention serving path (tests/golden/attn_serve_*.npz, written from the reference
by tools/make_golden_attn_serve.py) -- their internal consistency, the oracle against them, and the Python surface of the
new mode that needs no GPU.  The rows of these batches emit [s] at different steps, which no other LSTM-head fixture does."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, oracle_state_dict
from doc2tex_amd import Model, _lib, synth
from doc2tex_amd.build_model import DecodeHandle
from oracle import restatement as R

with open(os.path.join(GOLD, "attn_serve_cases.json")) as f:
    CASES = {c["case"]: c for c in json.load(f)["cases"]}
ORACLE_TOL = 2e-6  # oracle against reference, fp32 CPU both (the generator measured 6.3e-7)
MIN_GAP = 5e-3     # 5x the 1e-3 logits bar of the GPU tests


def _load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def test_the_three_cases_are_there():
    assert sorted(CASES) == ["attn_serve_to0_stagger", "attn_serve_ts0_noend", "attn_serve_ts0_stagger"]
    assert CASES["attn_serve_ts0_stagger"]["end_steps"] == [6, 6, 14, 6] and CASES["attn_serve_ts0_stagger"]["steps"] == 15
    assert CASES["attn_serve_to0_stagger"]["end_steps"] == [5, 6, 5, 5] and CASES["attn_serve_to0_stagger"]["steps"] == 7
    assert CASES["attn_serve_ts0_noend"]["end_steps"] == [6, -1, -1, 6]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_is_consistent(name):
    c, z = CASES[name], _load(name)
    B, S = c["B"], c["max_seq_len"] + 1
    tok, probs, alpha = z["tokens"], z["probs"], z["alpha"]
    assert tok.shape == (B, S) and probs.shape == (B, S, c["vocab"]) and alpha.shape == (B, S, c["keys"])
    ends = [int(np.nonzero(tok[b] == 1)[0][0]) if (tok[b] == 1).any() else -1 for b in range(B)]
    assert ends == c["end_steps"]
    if c["kind"] == "stagger":
        assert len(set(ends)) > 1 and min(ends) >= 0 and max(ends) < S - 1  # rows end at DIFFERENT steps, before the last
        assert c["steps"] == max(ends) + 1
    else:
        assert min(ends) < 0 <= max(ends) and c["steps"] == S  # a row never ends: no exit
    live = c["steps"]
    assert not probs[:, live:].any() and not tok[:, live:].any() and not alpha[:, live:].any()
    assert np.array_equal(probs[:, :live].argmax(-1), tok[:, :live])
    top2 = np.sort(probs[:, :live], axis=-1)[..., -2:]
    assert float((top2[..., 1] - top2[..., 0]).min()) >= MIN_GAP
    np.testing.assert_allclose(alpha[:, :live].sum(-1), 1.0, atol=1e-5)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_reproduces_the_reference(name, manifests):
    c, z = CASES[name], _load(name)
    cfg, sd = oracle_state_dict(c["config"], manifests[c["config"]], c["max_seq_len"], c["wseed"], c["end_bias"])
    img = synth.staggered_images(seed=c["iseed"])
    assert tuple(img.shape) == (c["B"], 1, c["H"], c["W"])
    text = torch.full((c["B"], 1), R.GO, dtype=torch.long)
    with torch.no_grad():
        p, l, _ = R.forward(cfg, sd, img, text, is_test=True)
    assert np.array_equal(p.numpy(), z["tokens"])
    err = float(np.abs(l.numpy() - z["probs"]).max())
    print(f"{name}: oracle against reference, max |dprob| = {err:.2e}")
    assert err <= ORACLE_TOL


def test_staggered_images_are_what_the_issue_describes():
    x, base = synth.staggered_images(), synth.synth_images(4, 48, 64, seed=1300)
    assert torch.equal(x[0], base[0]) and torch.equal(x[3], base[3] * -0.7)
    assert torch.equal(x[1, :, :, :32], base[1, :, :, :32] * 0.6) and bool((x[1, :, :, 32:] == 1.0).all())
    assert torch.equal(x[2, :, :24], base[2, :, :24] * 0.25) and bool((x[2, :, 24:] == 1.0).all())


def test_python_surface_of_the_new_mode():
    assert "d2t_decode_attn_greedy_submit" in _lib.SIGNATURES
    m = Model(synth.make_config("TS0"))
    assert m.pipelined is False and m.decode_chains == 1
    # an LSTM-head handle hands back the full-size tensors, a TFM handle cuts them at the step count
    class _Eng:
        def decode_steps(self, ticket):
            return [3]
    p, l = torch.zeros(2, 5, dtype=torch.long), torch.zeros(2, 5, 7)
    full = DecodeHandle(m, _Eng(), 1, 0, (p, l), full_size=True)
    assert full.steps() == 3 and full.result()[0] is p and full.result()[1] is l
    cut = DecodeHandle(m, _Eng(), 1, 0, (p, l))
    assert tuple(cut.result()[0].shape) == (2, 3) and tuple(cut.result()[1].shape) == (2, 3, 7)
