"""GPU: LSTM-attention heads with vocabularies beyond 1024 classes.  The decode kernel's wide build (V > 1024) computes every
class's logit with the arithmetic of the one-class-per-thread build and takes the same first maximum; these tests pin that
(a model padded with classes that never win gives bitwise the same logits and tokens as the unpadded one), compare greedy,
beam and training against the oracle at large V, and check the limits."""
import random

import pytest
import torch

from doc2tex_amd import Model, synth
from doc2tex_amd._lib import ATTN_MAX_CLASSES
from doc2tex_amd.engine import Engine
from oracle import restatement as R
from test_train_gpu import _check_instance, _step

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3  # the LSTM-head parity tests' bar
P = "predicter.Prediction."
AC = P + "attention_cell."


def _cfg(cname, V, L, beam_size=None, **pred):
    cfg = synth.make_config(cname, device="cuda", max_seq_len=L, beam_size=beam_size)
    cfg["num_class"] = V
    cfg["Prediction"]["params"].update(pred)
    return cfg


def _model(cfg, sd):
    m = Model(cfg)
    m.load_state_dict(sd)
    m.eval()
    return m.cuda()


def _seeded(cfg, wseed=1234, end_bias=0.0):
    """Seeded weights with the model's own keys and shapes (the committed manifests hold num_class = 500)."""
    tmpl = Model(cfg).state_dict()
    return synth.synth_state_dict(tmpl, seed=wseed, end_bias=end_bias, learned_pos=synth.learned_pos_embed(cfg))


def _pad(sd, V0, extra, seed=77):
    """The same model with `extra` classes appended that can never win: random generator rows, bias -1e4, random
    embedding rows / one-hot W_ih columns."""
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    gw = sd[AC + "generator.weight"]
    out[AC + "generator.weight"] = torch.cat([gw, torch.randn(extra, gw.shape[1], generator=g) * 0.05])
    out[AC + "generator.bias"] = torch.cat([sd[AC + "generator.bias"], torch.full((extra,), -1e4)])
    if P + "embedding.weight" in sd:
        e = sd[P + "embedding.weight"]
        out[P + "embedding.weight"] = torch.cat([e, torch.randn(extra, e.shape[1], generator=g)])
    w = sd[AC + "rnn.weight_ih"]
    if w.shape[1] == 256 + V0:  # one-hot targets: one W_ih column per class
        out[AC + "rnn.weight_ih"] = torch.cat([w, torch.randn(w.shape[0], extra, generator=g) * 0.05], 1)
    return out


def _labels(B, L, V, seed):
    """Teacher-forcing labels in the Attn converter's layout: [GO] = 0 first and as padding, [s] = 1, symbols in [2, V)."""
    g = torch.Generator().manual_seed(seed)
    text = torch.zeros(B, L + 2, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(L // 2, L + 1, (1,), generator=g))
        text[b, 1:1 + n] = torch.randint(2, V, (n,), generator=g)
        text[b, 1 + n] = 1
    return text


def _greedy(m, img, L, is_test):
    text = torch.zeros(img.shape[0], L + 1, dtype=torch.long, device="cuda")
    with torch.no_grad():
        preds, logits, _ = m(img.cuda(), text, is_train=False, is_test=is_test)
    torch.cuda.synchronize()
    return preds.cpu(), logits.cpu()


@pytest.mark.parametrize("cname", ["TS0", "TO0"])
def test_padded_vocabulary_gives_the_same_decode(cname):
    """V0 = 1000 runs the one-class-per-thread build, V0 + 2000 the wide build: tokens, logits [..., :V0] (bitwise),
    the is_test early exit, viz_attn maps and the beam search agree."""
    V0, V1, L = 1000, 3000, 12
    H, W = synth.crop_shape(cname)
    cfg0, cfg1 = _cfg(cname, V0, L), _cfg(cname, V1, L)
    sd0 = _seeded(cfg0, end_bias=0.3)
    sd1 = _pad(sd0, V0, V1 - V0)
    m0, m1 = _model(cfg0, sd0), _model(cfg1, sd1)
    img = synth.synth_images(3, H, W, seed=701)
    for is_test in (False, True):
        for m in (m0, m1):
            m.predicter.Prediction.viz_attn = True
        p0, l0 = _greedy(m0, img, L, is_test)
        a0 = m0.predicter.Prediction.alpha_stores.cpu()
        p1, l1 = _greedy(m1, img, L, is_test)
        a1 = m1.predicter.Prediction.alpha_stores.cpu()
        assert l1.shape[-1] == V1
        assert torch.equal(p0, p1), (is_test, p0, p1)
        assert torch.equal(l0, l1[..., :V0]), float((l0 - l1[..., :V0]).abs().max())
        assert torch.equal(a0, a1)
        live = l1[..., V0:]
        assert bool((live[live != 0] < -1e3).all())  # padding classes: bias -1e4 (zeros after an early exit)
    assert int((p0 == 1).any(1).sum()) >= 1  # [s] is emitted: the early exit is exercised
    for m in (m0, m1):
        m.predicter.Prediction.viz_attn = False
    beam = 4
    b0 = _model(_cfg(cname, V0, L, beam_size=beam), sd0)
    b1 = _model(_cfg(cname, V1, L, beam_size=beam), sd1)
    text = torch.zeros(1, L + 1, dtype=torch.long, device="cuda")
    for iseed in (702, 703):
        im = synth.synth_images(1, H, W, seed=iseed).cuda()
        with torch.no_grad():
            s0, v0, _ = b0(im, text, is_train=False, is_test=True)
            s1, v1, _ = b1(im, text, is_train=False, is_test=True)
        assert s0[0].tolist() == s1[0].tolist() and float(v0) == float(v1), (iseed, s0, s1, float(v0), float(v1))


@pytest.mark.parametrize("cname", ["TS0", "TO0"])
def test_padded_vocabulary_gives_the_same_training_step(cname):
    V0, V1, L, B = 1000, 3000, 10, 2
    H, W = synth.crop_shape(cname)
    kw = dict(droprate=0.0, teacher_forcing=1.0)
    cfg0, cfg1 = _cfg(cname, V0, L, **kw), _cfg(cname, V1, L, **kw)
    sd0 = _seeded(cfg0)
    sd1 = _pad(sd0, V0, V1 - V0)
    m0, m1 = _model(cfg0, sd0), _model(cfg1, sd1)
    m0.conv_precision = m1.conv_precision = "fp32"
    img = synth.synth_images(B, H, W, seed=711)
    text = _labels(B, L, V0, 712)
    loss0, pr0 = _step(m0, img, text)
    loss1, pr1 = _step(m1, img, text)
    assert abs(float(loss0) - float(loss1)) <= 1e-6 * max(1.0, abs(float(loss0)))
    assert torch.equal(pr0, pr1[..., :V0])
    g0 = {k: q.grad for k, q in m0.named_parameters() if q.grad is not None}
    g1 = {k: q.grad for k, q in m1.named_parameters() if q.grad is not None}
    assert sorted(g0) == sorted(g1)
    # The padding classes' softmax terms are exact zeros, but the cross-entropy and the dlogits . generator GEMM reduce over
    # a longer row, so gradients move by rounding: the decoder's within 1e-6 of each tensor's largest entry, the encoder's
    # (sums over every pixel, downstream of the memory gradient) within 1e-5.
    worst = {"head": 0.0, "encoder": 0.0}
    for k, a in g0.items():
        b = g1[k]
        assert bool(torch.isfinite(b).all()), k
        if k == AC + "rnn.weight_ih" and b.shape[1] != a.shape[1]:
            b = b[:, :a.shape[1]]
        elif b.shape != a.shape:
            b = b[:a.shape[0]]
        err = float((a - b).abs().max()) / max(float(a.abs().max()), 1e-30)
        part = "head" if k.startswith("predicter.") else "encoder"
        worst[part] = max(worst[part], err)
        assert err <= (1e-6 if part == "head" else 1e-5), (k, err)
    print(f"{cname}: padded training step, worst shared-gradient error of the tensor's largest entry: "
          f"head {worst['head']:.2e}, encoder {worst['encoder']:.2e}")


def _oracle_sd(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@pytest.mark.parametrize("cname,V", [("TS0", 1025), ("TO0", 4096), ("TS0", 16384), ("TB0", 5000)])
def test_greedy_vs_oracle_at_large_vocabularies(cname, V):
    L, B = 10, 2
    H, W = synth.crop_shape(cname)
    cfg = _cfg(cname, V, L)
    sd = _seeded(cfg, wseed=1240 + V % 97)
    m = _model(cfg, sd)
    img = synth.synth_images(B, H, W, seed=720 + V % 13)
    p, l = _greedy(m, img, L, False)
    text = torch.zeros(B, L + 1, dtype=torch.long)
    with torch.no_grad():
        op, ol, _ = R.forward(cfg, _oracle_sd(sd), img.double(), text, is_train=False, is_test=False)
    err = float((l.double() - ol).abs().max())
    print(f"{cname} V={V}: greedy tokens {'equal' if torch.equal(p, op) else 'DIFFER'}, max |dlogit| {err:.2e}, "
          f"{int((p >= 1024).sum())} of {p.numel()} tokens >= 1024")
    assert torch.equal(p, op)
    assert err <= LOGIT_TOL
    if V >= 4096:
        assert int((p >= 1024).sum()) >= 1  # the classes beyond the first 1024 win somewhere


@pytest.mark.parametrize("cname,V,beam", [("TS0", 1500, 4), ("TO0", 3000, 3)])
def test_beam_vs_oracle_at_large_vocabularies(cname, V, beam):
    L = 10
    H, W = synth.crop_shape(cname)
    cfg = _cfg(cname, V, L, beam_size=beam)
    sd = _seeded(cfg, end_bias=0.3)
    m = _model(cfg, sd)
    big = 0
    for iseed in (731, 732):
        img = synth.synth_images(1, H, W, seed=iseed)
        text = torch.zeros(1, L + 1, dtype=torch.long)
        with torch.no_grad():
            seq, score, _ = m(img.cuda(), text.cuda(), is_train=False, is_test=True)
            oseq, oscore, _ = R.forward(cfg, _oracle_sd(sd), img.double(), text, is_train=False, is_test=True)
        print(f"{cname} V={V} beam {beam}: |dscore| {abs(float(score) - float(oscore)):.2e}")
        assert seq[0].tolist() == oseq[0].tolist(), (iseed, seq, oseq)
        assert abs(float(score) - float(oscore)) <= 1e-3
        big += sum(t >= 1024 for t in seq[0].tolist())
    assert big >= 1


def test_training_with_output_dropout_and_scheduled_sampling_at_3000_classes():
    """TS0D (droprate 0.25, teacher_forcing 0.7) at num_class 3000: the engine's Philox mask read back, the oracle on the
    same mask and `random` flags (as test_train_gpu.test_lstm_head_training_with_output_dropout_and_scheduled_sampling)."""
    V, L, B, p = 3000, 10, 2, 0.25
    H, W = synth.crop_shape("TS0D")
    cfg = _cfg("TS0D", V, L)
    sd = _seeded(cfg, wseed=1250)
    m = _model(cfg, sd)
    m.conv_precision = "fp32"
    img = synth.synth_images(B, H, W, seed=741)
    text = _labels(B, L, V, 742)
    random.seed(743)
    flags = [1] + [0 if 0.7 < random.random() else 1 for _ in range(L)]  # doc2tex_amd/train.py, same stream
    assert 0 in flags[1:] and 1 in flags[1:]
    random.seed(743)  # the engine draws the same numbers
    torch.manual_seed(99)
    loss, preds = _step(m, img, text)
    eng = m._engine
    assert eng.mask_count() == 1
    S = L + 1
    mask = eng.read_mask(0, B * S * V).cpu().float().reshape(B, S, V)
    assert abs(float(mask.mean()) - (1.0 - p)) < 0.02
    step = [0]

    def drop(shape, kind):
        mk = mask[:, step[0], :] / (1.0 - p)
        step[0] += 1
        return mk

    oloss, ologits, ograds, _ = R.train_step_grads(cfg, sd, img, text, drop=drop, flags=flags)
    # the sampled steps feed the argmax of the previous step back: some of those tokens lie beyond the first 1024
    fed = [int(t) for j in range(1, S) if not flags[j] for t in ologits[:, j - 1].argmax(-1)]
    print(f"TS0D V={V}: |dloss| {abs(float(loss) - float(oloss)):.2e}, max |dlogit| "
          f"{float((preds.cpu() - ologits).abs().max()):.2e}, sampled tokens fed back {fed}")
    assert any(t >= 1024 for t in fed), fed
    assert abs(float(loss) - float(oloss)) <= 1e-4 * max(1.0, abs(float(oloss)))
    assert float((preds.cpu() - ologits).abs().max()) <= 1e-3
    assert _check_instance(m, ograds) <= 3e-2


def test_training_step_vs_oracle_at_2500_classes():
    V, L, B = 2500, 10, 2
    H, W = synth.crop_shape("TS0")
    cfg = _cfg("TS0", V, L, droprate=0.0, teacher_forcing=1.0)
    sd = _seeded(cfg, wseed=1260)
    m = _model(cfg, sd)
    m.conv_precision = "fp32"
    img = synth.synth_images(B, H, W, seed=751)
    text = _labels(B, L, V, 752)
    assert int((text >= 1024).sum()) >= 1
    loss, preds = _step(m, img, text)
    oloss, ologits, ograds, _ = R.train_step_grads(cfg, sd, img, text)
    print(f"TS0 V={V} training: |dloss| {abs(float(loss) - float(oloss)):.2e}, max |dlogit| "
          f"{float((preds.cpu() - ologits).abs().max()):.2e}")
    assert abs(float(loss) - float(oloss)) <= 1e-4 * max(1.0, abs(float(oloss)))
    assert float((preds.cpu() - ologits).abs().max()) <= 1e-3
    _check_instance(m, ograds)


def test_context_limits():
    Engine(_cfg("TS0", ATTN_MAX_CLASSES, 10))
    with pytest.raises(RuntimeError, match=f"num_class <= {ATTN_MAX_CLASSES}"):
        Engine(_cfg("TS0", ATTN_MAX_CLASSES + 1, 10))
    with pytest.raises(NotImplementedError, match=str(ATTN_MAX_CLASSES)):
        Model(_cfg("TO0", ATTN_MAX_CLASSES + 1, 10))
