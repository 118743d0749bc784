"""CPU: three-channel models (input_channel 3, `rgb: True`).  The rgb_* fixtures generated from the reference
(tools/make_golden_rgb.py) against oracle/restatement.py with the bounds tests/test_oracle_golden.py uses for the grey
ones -- these prove the fixtures, not the engine --, the parameter tree of the colour twins, and the C-ABI's channel check,
which needs no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, oracle_state_dict
from doc2tex_amd import Model, _lib, synth
from doc2tex_amd.engine import config_from_opt
from oracle import restatement as R
from test_oracle_golden import _grad_sample_index, train_step_labels

with open(os.path.join(GOLD, "rgb_cases.json")) as f:
    CASES = json.load(f)
with open(os.path.join(GOLD, "rgb_manifests.json")) as f:
    MANIFESTS = json.load(f)
MIN_GAP = 2e-3  # two logits that are each within the 1e-3 bar cannot change order across it


def case(kind, name):
    return next(c for c in CASES[kind] if c["case"] == name)


def names(kind):
    return [c["case"] for c in CASES[kind]]


def colour_images(c, B=None):
    return synth.synth_images(B or c["B"], c["H"], c["W"], seed=c["iseed"], channels=3)


def rgb_train_labels(c):
    """train_step_labels picks the converter layout by the grey configuration's name."""
    return train_step_labels({**c, "config": c["config"][:-1]})


def test_the_cases_the_feature_was_specified_with_are_all_there():
    assert sorted(c["config"] for c in CASES["greedy"]) == ["C0C", "T1C", "T2C", "TS0C"]
    assert sorted(c["config"] for c in CASES["beam"] + CASES["attn_beam"]) == ["T2C", "TS0C"]
    assert all(c["beam_size"] == 5 for c in CASES["beam"] + CASES["attn_beam"])
    assert sorted(c["config"] for c in CASES["train_step"]) == ["C0C", "T2C", "TS0C"]
    assert CASES["min_gap"] == MIN_GAP


@pytest.mark.parametrize("name", names("greedy"))
def test_greedy_fixture_matches_the_oracle(name):
    c = case("greedy", name)
    assert c["min_top2_gap"] >= MIN_GAP
    cfg, sd = oracle_state_dict(c["config"], MANIFESTS[c["config"]], c["max_seq_len"], c["wseed"], c["end_bias"])
    z = np.load(os.path.join(GOLD, name + ".npz"))
    assert float(z["top2_gap"].min()) >= MIN_GAP
    img = colour_images(c)
    assert img.shape[1] == 3 and not torch.equal(img[:, 0], img[:, 1])
    text = torch.full((c["B"], 1), R.GO, dtype=torch.long)
    with torch.no_grad():
        mem, shape, pad = R.forward_encoder(cfg, sd, img, faithful=False)
        preds, logits, _ = R.forward(cfg, sd, img, text, is_test=c["is_test"], faithful=False)
    assert list(mem.shape) == c["mem_shape"]
    assert (list(shape) if shape else None) == c["output_shape"]
    assert (list(pad) if pad else None) == c["feat_pad"]
    rows = z["mem_rows"].tolist()
    assert np.abs(mem[:, rows].numpy() - z["mem_sample"]).max() / max(1.0, c["mem_absmax"]) <= 2e-5
    assert preds.shape[1] == c["steps"]
    assert np.array_equal(preds.numpy(), z["tokens"])
    steps = z["logit_steps"].tolist()
    assert np.abs(logits[:, steps].numpy() - z["logits_sample"]).max() <= 1e-4


@pytest.mark.parametrize("kind,name", [(k, n) for k in ("beam", "attn_beam") for n in names(k)])
def test_beam_fixture_matches_the_oracle(kind, name):
    c = case(kind, name)
    assert c["min_top2_gap"] >= MIN_GAP and c["topk_calls"] > 0
    cfg, sd = oracle_state_dict(c["config"], MANIFESTS[c["config"]], c["max_seq_len"], c["wseed"], c["end_bias"])
    cfg["beam_size"] = c["beam_size"]
    img = colour_images(c, B=1)
    text = (torch.full((1, 1), R.GO, dtype=torch.long) if kind == "beam"
            else torch.zeros(1, c["max_seq_len"] + 1, dtype=torch.long))
    with torch.no_grad():
        seq, score, _ = R.forward(cfg, sd, img, text, is_train=False, is_test=True)
    assert seq[0].tolist() == c["seq"]
    assert abs(float(score) - c["score"]) <= 1e-3


@pytest.mark.parametrize("name", names("train_step"))
def test_train_step_fixture_matches_the_oracle(name):
    c = case("train_step", name)
    cfg, sd = oracle_state_dict(c["config"], MANIFESTS[c["config"]], c["max_seq_len"], c["wseed"])
    z = np.load(os.path.join(GOLD, name + ".npz"))
    img = colour_images(c)
    text = rgb_train_labels(c)
    assert np.array_equal(text.numpy(), z["text"])
    loss, logits, grads, bn = R.train_step_grads(cfg, sd, img, text)
    assert abs(float(loss) - c["loss"]) <= 1e-5 * max(1.0, abs(c["loss"]))
    assert np.abs(logits.numpy() - z["logits"]).max() <= 2e-4  # test_oracle_golden.py's bound for the step's logits
    assert sorted(grads) == sorted(c["grad_norms"])
    assert not any(k in grads for k in c["frozen"])
    stem = next(k for k in grads if k.endswith(("conv0_1.weight", "ConvNet.0.weight")))
    assert list(grads[stem].shape[1:]) == [3, 3, 3]
    for k, g in grads.items():
        norm, _ = c["grad_norms"][k]
        if k.endswith("attn.score.bias"):  # mathematically zero (a softmax ignores a shift of its logits): what is left is
            assert norm <= 1e-7 and float(g.abs().max()) <= 1e-7, k  # rounding noise (1e-10) that differs between CPUs
            continue
        assert abs(float(g.double().norm()) - norm) <= 1e-4 * max(norm, 1e-6) + 1e-9, k
        idx = _grad_sample_index(k, g.numel())
        ref = z["g:" + k]
        assert np.abs(g.reshape(-1)[idx].numpy() - ref).max() <= 5e-4 * max(float(np.abs(ref).max()), norm / g.numel() ** 0.5, 1e-7), k
    for k, v in bn.items():
        assert np.abs(v.numpy() - z["bn:" + k]).max() <= 1e-5 * max(1.0, float(np.abs(z["bn:" + k]).max())), k


def test_headline_size_seed_leaves_few_close_calls():
    """The GPU comparison at 128x512 skips (row, step) pairs whose top-2 gap in the restatement is below MIN_GAP; the seed was
    chosen so that this is at most 1 pair in 10 (re-derived on the GPU machine's host by that test)."""
    c = CASES["c2c_parity"]
    assert c["config"] == "C2C" and (c["B"], c["H"], c["W"], c["steps"]) == (2, 128, 512, 20)
    assert c["low_gap_pairs"] * 10 <= c["B"] * c["steps"]


@pytest.mark.parametrize("name", ["T2C", "TS0C", "C0C", "T1C", "C2C"])
def test_colour_twins_have_the_reference_parameter_tree(name):
    sd = Model(synth.make_config(name)).state_dict()
    ref = MANIFESTS[name]
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert list(v.shape) == ref[k], k
    stem = [k for k in sd if k.endswith("conv0_1.weight") or k.endswith("ConvNet.0.weight")]
    assert len(stem) == 1
    assert list(sd[stem[0]].shape) == ([64, 3, 3, 3] if name == "C0C" else [32, 3, 3, 3])
    assert synth.image_channels(synth.make_config(name)) == 3
    assert config_from_opt(synth.make_config(name)).in_channels == 3
    assert config_from_opt(synth.make_config(name[:-1])).in_channels == 1


def _create(in_channels):
    """d2t_create without a device: (status, message).  Engine(...) itself asks for a device first, so go to the library."""
    lib = _lib.load()
    cfg = config_from_opt(synth.make_config("T2C"))
    cfg.in_channels = in_channels
    ctx = C.c_void_p()
    rc = lib.d2t_create(C.byref(cfg), C.byref(ctx))
    msg = lib.d2t_last_error(ctx).decode() if ctx else ""
    if ctx:
        lib.d2t_destroy(ctx)
    return rc, msg


def test_create_accepts_one_and_three_channels_and_names_them_otherwise():
    """The config check runs before the device check, so on a machine without a GPU a 3-channel config must get as far as
    "no HIP device" (with a GPU: it is created), while 2 channels are refused with a message that names 1 and 3."""
    have_gpu = bool(_lib.load().d2t_device_available())
    for ch in (1, 3):
        rc, msg = _create(ch)
        if have_gpu:
            assert rc == _lib.D2T_OK, (ch, rc, msg)
        else:
            assert rc != _lib.D2T_OK and "no HIP device" in msg and "in_channels" not in msg, (ch, rc, msg)
    for ch in (0, 2, 4):
        rc, msg = _create(ch)
        assert rc != _lib.D2T_OK and "in_channels" in msg and "1" in msg and "3" in msg and "no HIP device" not in msg, (ch, msg)


def test_synth_images_channels_default_is_todays_bits():
    a, b = synth.synth_images(2, 8, 8, seed=5), synth.synth_images(2, 8, 8, seed=5, channels=1)
    assert a.shape == (2, 1, 8, 8) and torch.equal(a, b)
    assert synth.synth_images(2, 8, 8, seed=5, channels=3).shape == (2, 3, 8, 8)


def test_prep_plan_mirrors_minmax_size_without_is_gray():
    """`rgb: True`: minmax_size(..., is_gray=False) leaves MODE / BACKGROUND unassigned (utils/data_utils.py:75-79), so an image
    below min_dimension cannot be planned; at or above it the plan is the grey one.  Host only."""
    lib = _lib.load()
    plans = {}
    for ch in (0, 1, 3):
        cfg = _lib.D2TPrepConfig(max_h=128, max_w=512, min_h=32, min_w=32, downsample=0, variant=_lib.PREP_DEMO, mean=0.5,
                                 std=0.5, norm_mode=_lib.NORM_ALB, channels=ch)
        for hw in ((20, 100), (64, 200), (300, 900)):
            p = _lib.D2TPrepPlan()
            assert lib.d2t_prep_plan_image(C.byref(cfg), hw[0], hw[1], C.byref(p)) == _lib.D2T_OK
            plans[ch, hw] = tuple(getattr(p, f) for f, _ in _lib.D2TPrepPlan._fields_)
    for hw in ((20, 100), (64, 200), (300, 900)):
        assert plans[0, hw] == plans[1, hw]
    assert plans[3, (64, 200)] == plans[1, (64, 200)] and plans[3, (300, 900)] == plans[1, (300, 900)]
    status = [f for f, _ in _lib.D2TPrepPlan._fields_].index("status")
    assert plans[1, (20, 100)][status] == _lib.PREP_OK and plans[3, (20, 100)][status] == _lib.PREP_UNBOUND_LOCAL
