"""GPU: decoder alignment maps (viz_attn) of the LSTM-attention heads against the reference's own
(tests/golden/viz_*.npz, tools/make_golden_viz.py): greedy Prediction.alpha_stores, the beam search's decoder_attn and the
entries Model.forward adds, the training forward's alpha_stores; batched maps against per-sample maps; the maps-off path;
the history budget."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, engine_model
from doc2tex_amd import _lib, synth

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "viz_cases.json")) as f:
    VIZ = json.load(f)
CASES = {c["case"]: c for c in VIZ["cases"]}
# Engine alignments against the reference's (fp32 CPU), measured on an MI355X: max |d alpha| 7.1e-6 greedy, 8.5e-6 beam (TA0),
# 6.7e-6 training forward (fp32 backbone), 1.5e-7 on the sampled rows of the shipped geometry; the bar leaves a wide margin.
ATOL = 1e-4


def _of(kind):
    return [n for n, c in CASES.items() if c["kind"] == kind]


def _load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _viz(m, on=True):
    m.predicter.Prediction.viz_attn = on  # read at call time, as in the reference
    return m


@pytest.mark.parametrize("name", _of("greedy"))
def test_greedy_alpha_stores_match_reference(name):
    c, z = CASES[name], _load(name)
    _, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], c["end_bias"])
    _viz(m)
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]).cuda()
    text = torch.zeros(c["B"], c["max_seq_len"] + 1, dtype=torch.long, device="cuda")
    with torch.no_grad():
        preds, _, add = m(img, text, is_train=False, is_test=c["is_test"])
    assert add == {}
    assert np.array_equal(preds.cpu().numpy(), z["tokens"])
    a = m.predicter.Prediction.alpha_stores
    assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == z["alpha"].shape + (1,)
    err = float(np.abs(a[..., 0].cpu().numpy() - z["alpha"]).max())
    print(f"{name}: max |d alpha| = {err:.2e}")
    assert err <= ATOL
    if c["is_test"]:  # zeros after the early exit, exactly
        assert float(a[:, c["exit_step"] + 1:].abs().max()) == 0.0


@pytest.mark.parametrize("name", _of("beam"))
def test_beam_decoder_attn_matches_reference(name):
    c, z = CASES[name], _load(name)
    _, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], c["end_bias"], beam_size=c["beam_size"])
    _viz(m)
    img = synth.synth_images(1, c["H"], c["W"], seed=c["iseed"]).cuda()
    text = torch.zeros(1, c["max_seq_len"] + 1, dtype=torch.long, device="cuda")
    with torch.no_grad():
        mem = m.forward_encoder(img)[0]
        seq_d, _, alphas, _ = m.forward_decoder(mem, text, is_train=False, is_test=True)
        seq, score, add = m(img, text, is_train=False, is_test=True)
    assert seq[0].tolist() == seq_d[0].tolist() == c["seq"]
    assert abs(float(score) - c["score"]) <= 1e-3
    assert not hasattr(m.predicter.Prediction, "alpha_stores")
    assert alphas.is_cuda and tuple(alphas.shape) == z["alpha"].shape
    err = float(np.abs(alphas.cpu().numpy() - z["alpha"]).max())
    print(f"{name}: max |d alpha| = {err:.2e}")
    assert err <= ATOL
    assert sorted(add) == c["addition_keys"]
    if "decoder_attn" in add:
        assert list(add["decoder_attn"].shape) == c["decoder_attn_shape"]
        assert float(np.abs(add["decoder_attn"].cpu().numpy() - z["decoder_attn"]).max()) <= ATOL
        assert (add["feat_width"], add["feat_height"]) == (c["feat_width"], c["feat_height"])
        assert list(add["feat_pad"]) == c["feat_pad"]


def _train_labels(cfg, B, L, iseed):
    """tools/make_golden.py train_labels for the Attn converter: [GO] = 0 first and as padding, [s] = 1."""
    text = synth.synth_labels(B, max_len=L, seed=iseed)
    text[0, L // 2:] = 0
    text[0, L // 2 - 1] = 2
    t = text.clone()
    t[text == 1] = 0
    t[text == 2] = 1
    return t


@pytest.mark.parametrize("name", _of("train"))
def test_train_alpha_stores_match_reference(name):
    c, z = CASES[name], _load(name)
    cfg, m = engine_model(c["config"], c["max_seq_len"], c["wseed"])
    m.conv_precision = "fp32"
    _viz(m)
    m.train()
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]).cuda()
    text = _train_labels(cfg, c["B"], c["max_seq_len"], c["iseed"]).cuda()
    _, preds, _ = m(img, text[:, :-1])
    a = m.predicter.Prediction.alpha_stores
    assert not a.requires_grad and a.grad_fn is None  # detached (the reference's carries grad)
    assert tuple(a.shape) == z["alpha"].shape + (1,)
    err = float(np.abs(a[..., 0].cpu().numpy() - z["alpha"]).max())
    print(f"{name}: max |d alpha| = {err:.2e}")
    assert err <= ATOL
    preds.sum().backward()  # the step still runs its backward after the read
    torch.cuda.synchronize()


@pytest.mark.parametrize("cname,H,W,L,eb,beam", [("TS0", 48, 64, 14, 0.3, 5), ("TA0", 48, 64, 8, 0.0, 3),
                                                ("C0", 32, 320, 12, 0.17, 4)])
def test_batched_maps_equal_per_sample_maps(cname, H, W, L, eb, beam):
    _, m = engine_model(cname, L, 1234, eb, beam_size=beam)
    _viz(m)
    img = synth.synth_images(5, H, W, seed=1210).cuda()
    text = torch.zeros(1, L + 1, dtype=torch.long, device="cuda")
    with torch.no_grad():
        batch = m.beam_search_batch(img, return_attn=True)
        plain = m.beam_search_batch(img)
        for i in range(5):
            mem = m.forward_encoder(img[i:i + 1])[0]
            seq, score, alphas, _ = m.forward_decoder(mem, text, is_train=False, is_test=True)
            s2, v2, a2 = batch[i]
            assert torch.equal(seq, s2) and float(score) == float(v2)
            assert torch.equal(alphas, a2), (cname, i)
            assert torch.equal(plain[i][0], s2) and float(plain[i][1]) == float(v2)


def test_maps_off_path_is_unchanged():
    """viz_attn False: the same tensors as with the maps, no alpha_stores attribute, nothing added to addition_outputs."""
    _, m = engine_model("TS0", 12, 1234, 0.3, beam_size=1)
    img = synth.synth_images(2, 48, 64, seed=1008).cuda()
    text = torch.zeros(2, 13, dtype=torch.long, device="cuda")
    with torch.no_grad():
        p0, l0, a0 = m(img, text, is_train=False, is_test=True)
        assert not hasattr(m.predicter.Prediction, "alpha_stores") and a0 == {}
        p1, l1, _ = _viz(m)(img, text, is_train=False, is_test=True)
    assert torch.equal(p0, p1) and torch.equal(l0, l1)
    _, m = engine_model("TS0", 14, 1234, 0.3, beam_size=5)
    with torch.no_grad():
        s0, v0, a0 = m(img[:1], text[:1], is_train=False, is_test=True)
        s1, v1, a1 = _viz(m)(img[:1], text[:1], is_train=False, is_test=True)
    assert not hasattr(m.predicter.Prediction, "alpha_stores") and a0 == {}
    assert torch.equal(s0, s1) and float(v0) == float(v1) and "decoder_attn" in a1


def test_history_budget_refused_with_a_message():
    _, m = engine_model("TS0", 500, beam_size=16)
    eng = m.engine()
    T = 1695  # the shipped 448 x 960 crops: 1694 keys; 5 samples x beam 16 x 501 steps exceed the budget
    assert 5 * eng.attn_map_bytes(T, 16) > _lib.ATTN_MAP_BUDGET >= 4 * eng.attn_map_bytes(T, 16)
    mem = torch.zeros(5, T, 256, device="cuda")
    with pytest.raises(RuntimeError, match="exceeds the .*budget"):
        eng.decode_attn_beam_batch(mem, 16, return_alpha=True)


def test_beam_search_batch_splits_at_the_budget(monkeypatch):
    _, m = engine_model("TS0", 10, 1234, 0.3, beam_size=4)
    img = synth.synth_images(5, 48, 64, seed=1211).cuda()
    with torch.no_grad():
        whole = m.beam_search_batch(img, return_attn=True)
        T = m.forward_encoder(img[:1])[0].shape[1]
        monkeypatch.setattr(_lib, "ATTN_MAP_BUDGET", 2 * m.engine().attn_map_bytes(T, 4))  # parts of two samples
        parts = m.beam_search_batch(img, return_attn=True)
    for (s1, v1, a1), (s2, v2, a2) in zip(whole, parts):
        assert torch.equal(s1, s2) and float(v1) == float(v2) and torch.equal(a1, a2)


def test_shipped_test_yaml_geometry_maps():
    """config/test.yaml geometry (448 x 960 crop, 1694 keys, batch_max_length 500, beam 5) with viz_attn: the reference's
    sequence, a decoder_attn laid on the 14 x 121 grid, and its rows (argmax, sums, sampled rows) as the reference's."""
    from doc2tex_amd import Model
    c, z = CASES["viz_shipped_beam5"], _load("viz_shipped_beam5")
    cfg = synth.make_config("S0", device="cuda", max_seq_len=c["max_seq_len"], beam_size=c["beam_size"])
    cfg["max_dimension"] = [c["H"], c["W"]]
    m = Model(cfg)
    m.load_state_dict(synth.synth_state_dict({k: v for k, v in m.state_dict().items()}, end_bias=c["end_bias"]), strict=False)
    m = _viz(m.cuda().eval())
    img = synth.synth_images(1, c["H"], c["W"], seed=c["iseed"]).cuda()
    text = torch.zeros(1, c["max_seq_len"] + 1, dtype=torch.long, device="cuda")
    with torch.no_grad():
        seq, _, add = m(img, text, is_train=False)
    assert seq[0].tolist() == c["seq"]
    d = add["decoder_attn"]
    assert tuple(d.shape) == (len(c["seq"]), *c["output_shape"])
    a = d.reshape(d.shape[0], -1).cpu()
    assert np.array_equal(a.argmax(1).numpy(), z["argmax"])
    assert np.abs(a.double().sum(1).numpy() - z["rowsum"]).max() <= 1e-5
    err = float(np.abs(a[z["rows"]].numpy() - z["rows_alpha"]).max())
    print(f"viz_shipped_beam5: max |d alpha| = {err:.2e}")
    assert err <= ATOL
