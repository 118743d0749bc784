"""CPU: the LSTM-attention heads take vocabularies beyond 1024 classes (num_class = len(converter.character) comes from the
user's vocab.txt).  Construction and the reference's parameter shapes; the cap is refused with a message.  No GPU needed."""
import pytest

from doc2tex_amd import Model, synth
from doc2tex_amd._lib import ATTN_MAX_CLASSES


def _cfg(name, V):
    cfg = synth.make_config(name)
    cfg["num_class"] = V
    return cfg


def test_one_hot_head_constructs_with_3000_classes():
    m = Model(_cfg("TO0", 3000))
    sd = m.state_dict()
    p = "predicter.Prediction.attention_cell."
    assert tuple(sd[p + "generator.weight"].shape) == (3000, 256)
    assert tuple(sd[p + "generator.bias"].shape) == (3000,)
    assert tuple(sd[p + "rnn.weight_ih"].shape) == (1024, 256 + 3000)  # [4H][H + num_class]: one-hot decoder input


def test_embedded_head_constructs_with_the_cap():
    m = Model(_cfg("TS0", ATTN_MAX_CLASSES))
    sd = m.state_dict()
    assert tuple(sd["predicter.Prediction.embedding.weight"].shape) == (ATTN_MAX_CLASSES, 256)
    assert tuple(sd["predicter.Prediction.attention_cell.generator.weight"].shape) == (ATTN_MAX_CLASSES, 256)


def test_one_hot_head_at_the_cap_constructs():
    Model(_cfg("TO0", ATTN_MAX_CLASSES))


def test_one_hot_head_beyond_the_cap_is_refused():
    assert ATTN_MAX_CLASSES >= 16384
    with pytest.raises(NotImplementedError, match=str(ATTN_MAX_CLASSES)):
        Model(_cfg("TO0", ATTN_MAX_CLASSES + 1))


def test_cap_matches_the_c_header():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "d2t.h")) as f:
        assert f"#define D2T_ATTN_MAX_CLASSES {ATTN_MAX_CLASSES}\n" in f.read()
