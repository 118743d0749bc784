"""CPU: the parameter tree, the engine configuration and the refusals of the Feat x Seq x Pred pairings that
tools/make_golden_stacks.py covers -- BiLSTM encoders under the TFM head, VGG + PositionalEncoding2D + TFM, and
`mean_height: False` (proj_feat) -- plus the CPU anchor of their fixtures: oracle/restatement.py on the two
`mean_height: True` BiLSTM + TFM stacks, and a float64 statement of proj_feat as a (3, 1) convolution."""
import itertools

import pytest
import torch

from conftest import oracle_state_dict
from doc2tex_amd import Model, _lib, synth
from doc2tex_amd.engine import config_from_opt
from oracle import restatement as R

import stack_refs as S


@pytest.mark.parametrize("cname", ["VBT", "RBT", "VT", "VBTP", "RBTP", "VBAP", "RBAP", "VTP"])
def test_state_dict_equals_the_reference_manifest(cname):
    man = S.stack_manifests()[cname]
    m = Model(synth.make_config(cname, max_seq_len=S.L))
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == man
    has_proj = {k for k in man if k.startswith("featextractor.proj_feat.")}
    if cname in ("VBTP", "RBTP", "VBAP", "RBAP", "VTP"):
        assert has_proj == {"featextractor.proj_feat.weight", "featextractor.proj_feat.bias"}
        assert man["featextractor.proj_feat.weight"] == [512, 1536] and man["featextractor.proj_feat.bias"] == [512]
    else:
        assert not has_proj
    if cname in ("VT", "VTP"):
        assert man["seqmodeler.image_positional_encoder.pe"] == [512, 2000, 2000]


@pytest.mark.parametrize("feat", ["VGG", "ResNet"])
@pytest.mark.parametrize("mean_height", [None, True, False])
def test_proj_feat_exists_exactly_when_mean_height_is_false(feat, mean_height):
    cfg = synth.make_config("VBT" if feat == "VGG" else "RBT", max_seq_len=S.L)
    if mean_height is not None:
        cfg["FeatureExtraction"]["params"]["mean_height"] = mean_height
    m = Model(cfg)
    assert "mean_height" not in cfg["FeatureExtraction"]["params"]  # popped, as build_feat.py:16 does
    assert m.featextractor.mean_height is (mean_height is not False)
    assert hasattr(m.featextractor, "proj_feat") == (mean_height is False)
    if mean_height is False:
        lin = m.featextractor.proj_feat
        assert isinstance(lin, torch.nn.Linear) and (lin.in_features, lin.out_features) == (1536, 512)
        # a checkpoint of the reference loads strictly; one without the layer does not
        sd = m.state_dict()
        m.load_state_dict(sd, strict=True)
        sd.pop("featextractor.proj_feat.weight")
        with pytest.raises(RuntimeError, match="proj_feat.weight"):
            m.load_state_dict(sd, strict=True)


def test_config_from_opt_routes_the_new_stacks():
    want = {"VBT": (_lib.ENC_VGG_BILSTM, 0), "RBT": (_lib.ENC_RESNET_BILSTM, 0), "VT": (_lib.ENC_VGG, 0),
            "VBTP": (_lib.ENC_VGG_BILSTM, 1), "RBTP": (_lib.ENC_RESNET_BILSTM, 1), "VBAP": (_lib.ENC_VGG_BILSTM, 1),
            "RBAP": (_lib.ENC_RESNET_BILSTM, 1), "VTP": (_lib.ENC_VGG, 0), "C0": (_lib.ENC_VGG_BILSTM, 0), "T1": (_lib.ENC_RESNET, 0)}
    assert _lib.ENC_VGG == 4
    for cname, (enc, flag) in want.items():
        raw = config_from_opt(synth.make_config(cname, max_seq_len=S.L))  # the key still in the dict
        assert (raw.encoder, raw.proj_height) == (enc, flag), cname
        cfg = synth.make_config(cname, max_seq_len=S.L)
        m = Model(cfg)  # the key popped: the builder's value decides
        assert "mean_height" not in cfg["FeatureExtraction"]["params"]
        got = config_from_opt(m.engine_opt())
        assert (m.engine_opt() is cfg) == (flag == 0 and cname != "VTP")
        assert (got.encoder, got.proj_height) == (enc, flag), cname
        tfm = cfg["Prediction"]["name"] == "TFM"
        assert got.decoder == (_lib.DEC_TFM if tfm else _lib.DEC_ATTN)
        if tfm:
            assert got.dec_dim == (512 if cname in ("VT", "VTP", "T1") else 256)
    assert _lib.D2TConfig._fields_[-1][0] == "proj_height"


def test_every_triple_the_reference_can_run_is_accepted_and_the_rest_refused():
    """Feat x Seq x Pred over the convolutional feature extractors: the reference runs a forward of every BiLSTM stack and of
    Seq = None under the TFM head; Seq = None under Attn reads an attribute only FeatExtractorBuilder has (build_seq.py:78),
    under Attnv2 it leaves the result unbound."""
    heads = {"TFM256": "VBT", "TFM512": "VT", "Attn": "VBAP", "Attnv2": "RBAP"}  # a configuration with that head
    for feat, seq, head in itertools.product(("VGG", "ResNet"), ("BiLSTM", "None"), heads):
        cfg = synth.make_config("VBT", max_seq_len=S.L)
        cfg["FeatureExtraction"]["name"] = feat
        cfg["SequenceModeling"] = {"name": seq, "params": {"hidden_size": 256} if seq == "BiLSTM" else {}}
        cfg["Prediction"] = synth.make_config(heads[head], max_seq_len=S.L)["Prediction"]
        runs = (seq == "BiLSTM" and head != "TFM512") or (seq == "None" and head in ("TFM512",))
        if runs:
            Model(cfg)
            config_from_opt(cfg)
        elif seq == "None" and head == "TFM256":  # d_model 256 against 512 channels: fails in the reference's cross-attention
            continue
        else:
            with pytest.raises(NotImplementedError):
                config_from_opt(cfg)


def test_remaining_refusals_name_their_reason():
    for feat in ("VGG", "ResNet"):
        for head in ("VBAP", "RBAP"):
            cfg = synth.make_config("VT", max_seq_len=S.L)
            cfg["FeatureExtraction"]["name"] = feat
            cfg["Prediction"] = synth.make_config(head, max_seq_len=S.L)["Prediction"]
            with pytest.raises(NotImplementedError, match=r"build_seq\.py:78"):
                config_from_opt(cfg)
    cfg = synth.make_config("VBT", max_seq_len=S.L)
    cfg["SequenceModeling"]["params"]["hidden_size"] = 512
    cfg["Prediction"]["params"]["d_model"] = 512
    with pytest.raises(NotImplementedError, match="hidden_size must be 256.*512"):
        config_from_opt(cfg)
    cfg = synth.make_config("RBT", max_seq_len=S.L)
    cfg["Prediction"]["params"]["d_model"] = 512
    with pytest.raises(NotImplementedError, match="d_model = the BiLSTM hidden_size = 256.*512"):
        config_from_opt(cfg)
    cfg = synth.make_config("VBT", max_seq_len=S.L)
    cfg["SequenceModeling"]["params"]["pos_enc"] = True
    with pytest.raises(NotImplementedError, match=r"build_seq\.py:55"):
        config_from_opt(cfg)


@pytest.mark.parametrize("name", ["vbt_greedy_b2", "vbt_greedy_b5", "rbt_greedy_b2", "rbt_greedy_b5"])
def test_oracle_reproduces_the_bilstm_tfm_fixtures(name):
    """The CPU anchor that travels: oracle/restatement.py composes the BiLSTM encoders with the TFM head."""
    c = S.stack_case("greedy", name)
    z = S.stack_arrays(name)
    cfg, sd = oracle_state_dict(c["config"], S.stack_manifests()[c["config"]], S.L, c["wseed"])
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"])
    with torch.no_grad():
        mem, _, _ = R.forward_encoder(cfg, sd, img, faithful=True)
        preds, logits, _ = R.forward(cfg, sd, img, torch.full((c["B"], 1), R.GO, dtype=torch.long), is_test=False)
    assert list(mem.shape) == c["mem_shape"]
    assert float((mem - torch.from_numpy(z["mem_full"])).abs().max()) <= 1e-5 * max(1.0, c["mem_absmax"])
    assert preds.shape[1] == c["steps"] == S.L + 1
    assert (preds.numpy() == z["tokens"]).all()
    assert float((logits - torch.from_numpy(z["logits"])).abs().max()) <= 1e-5


def test_fixture_gaps_decide_the_tokens_inside_the_logit_bar():
    """Every greedy fixture records the reference's top-2 gap at every (row, step); none is below 2e-3, so no token can flip
    while both logits stay inside the 1e-3 bar.  The LSTM-attention stacks got there by walking the weight seed."""
    for name in S.TFM_GREEDY + S.ATTN_GREEDY:
        c, z = S.stack_case("greedy", name), S.stack_arrays(name)
        assert z["top2_gap"].shape == (c["B"], S.L + 1)
        assert abs(float(z["top2_gap"].min()) - c["min_top2_gap"]) <= 1e-9
        assert c["min_top2_gap"] >= S.MIN_GAP, (name, c["min_top2_gap"])
        top = torch.from_numpy(z["logits"]).topk(2, dim=-1)
        assert (top.indices[..., 0].numpy() == z["tokens"]).all()
    walked = S.stack_cases()["attn_wseed"]
    assert set(walked) == {"VBAP", "RBAP"}
    for cname, w in walked.items():
        assert w["reached"] and w["min_top2_gap"] >= S.MIN_GAP and w["seeds_tried"] <= 20
        assert all(c["wseed"] == w["wseed"] for c in S.stack_cases()["greedy"] if c["config"] == cname)


@pytest.mark.parametrize("B,Wp", [(1, 1), (2, 5), (2, 23)])
def test_proj_feat_is_a_3x1_convolution(B, Wp):
    """flatten(-2) of [b, w, c, h] orders the columns as c * 3 + h, which is how weight.view(C, C, 3, 1) lies in memory."""
    x, w, b, _ = S.proj_feat_case(B, Wp, C=64)
    ref = S.proj_feat_linear(x.double(), w.double(), b.double())
    assert ref.shape == (B, Wp, 64)
    for form in (S.proj_feat_conv, S.proj_feat_taps):
        assert float((form(x.double(), w.double(), b.double()) - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    # the order matters: the h * C + c flattening is another function
    other = torch.nn.functional.linear(x.double().permute(0, 3, 2, 1).flatten(start_dim=-2), w.double(), b.double())
    assert float((other - ref).abs().max()) > 0.1


def test_reference_failure_on_a_32_pixel_crop_is_recorded():
    c = S.stack_case("raises", "vbtp_32px")
    assert c["type"] == "RuntimeError" and "46x512 and 1536x512" in c["message"]
