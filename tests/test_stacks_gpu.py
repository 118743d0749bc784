"""GPU: the Feat x Seq x Pred pairings of tools/make_golden_stacks.py against the reference's fixtures -- BiLSTM encoders
under the TFM head (d_model 256), VGG + PositionalEncoding2D + TFM (d_model 512), and `mean_height: False` (proj_feat =
Linear(3C -> C) over the flattened height, run as a (3, 1) convolution) under the TFM, Attn and Attnv2 heads.

Bars: greedy tokens exact and logits within 1e-3 (every fixture's top-2 gap is >= 2e-3, tests/test_stacks_cpu.py); beam
sequences exact, scores at the tolerance of tests/test_parity_gpu.py; training steps held to what tests/test_train_gpu.py asks
of c0_train_step / t1_train_step against their fixtures; the proj_feat operator against float64 under the measured rule of
DESIGN.md section 5.3a (err <= 8 e32 + 1e-6 max |y64|) in fp32 arithmetic."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from conftest import engine_model
from doc2tex_amd import _lib, synth
from oracle import restatement as R

import stack_refs as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-3
MEM_TOL = {"fp32": 1e-4, "bf16x3": 5e-4, "fp16x2": 2e-3, "mixed": 1e-3}  # encoder memory, as tests/test_parity_gpu.py


def _go(B):
    return torch.full((B, 1), R.GO, dtype=torch.long, device=DEV)


# ---- greedy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.TFM_GREEDY + S.ATTN_GREEDY)
def test_greedy_vs_reference_fixture(name):
    c, z = S.stack_case("greedy", name), S.stack_arrays(name)
    assert c["min_top2_gap"] >= S.MIN_GAP
    cfg, m = engine_model(c["config"], S.L, c["wseed"])
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]).to(DEV)
    with torch.no_grad():
        mem, shape, pad = m.forward_encoder(img)
        preds, logits, _ = m(img, _go(c["B"]), is_train=False, is_test=False)
    torch.cuda.synchronize()
    assert list(mem.shape) == c["mem_shape"] and shape is None and pad is None
    dmem = float(np.abs(mem.cpu().numpy() - z["mem_full"]).max()) / max(1.0, c["mem_absmax"])
    dl = float(np.abs(logits.cpu().numpy() - z["logits"]).max())
    print(f"{name}: memory rel err {dmem:.3e}, max |dlogit| {dl:.3e}, fixture gap {c['min_top2_gap']:.3e}")
    assert dmem <= MEM_TOL[m.effective_conv_precision()], f"encoder memory rel err {dmem}"
    assert preds.shape[1] == c["steps"] == S.L + 1
    assert np.array_equal(preds.cpu().numpy(), z["tokens"]), "greedy token ids differ from the reference"
    assert dl <= LOGIT_TOL, f"logits differ by {dl}"


# ---- beam --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vbt_beam3", "vbt_beam3_end"])
def test_tfm_beam_vs_reference_fixture(name):
    c = S.stack_case("beam", name)
    cfg, m = engine_model(c["config"], S.L, c["wseed"], c["end_bias"], beam_size=c["beam_size"])
    img = synth.synth_images(1, c["H"], c["W"], seed=c["iseed"]).to(DEV)
    with torch.no_grad():
        seq, score, _ = m(img, _go(1), is_train=False, is_test=True)
        batch = m.beam_search_batch(img)
    assert seq.shape[0] == 1 and seq[0].tolist() == c["seq"], (seq, c["seq"])
    # tests/test_parity_gpu.py _score_tol: a sum of n log-probabilities, each held to ~1e-5
    tol = 5e-3 if m.effective_conv_precision() == "fp16x2" else max(1e-3, 2e-5 * len(c["seq"]))
    assert abs(score - c["score"]) <= tol, (score, c["score"])
    assert len(batch) == 1 and torch.equal(batch[0][0], seq) and batch[0][1] == score


@pytest.mark.parametrize("name", ["vbap_beam3", "vbap_beam3_end"])
def test_attn_beam_vs_reference_fixture(name):
    c = S.stack_case("attn_beam", name)
    cfg, m = engine_model(c["config"], S.L, c["wseed"], c["end_bias"], beam_size=c["beam_size"])
    img = synth.synth_images(1, c["H"], c["W"], seed=c["iseed"]).to(DEV)
    text = torch.zeros(1, S.L + 1, dtype=torch.long, device=DEV)
    with torch.no_grad():
        seq, score, _ = m(img, text, is_train=False, is_test=True)
    assert seq.shape[0] == 1 and seq[0].tolist() == c["seq"], (seq, c["seq"])
    assert abs(float(score) - c["score"]) <= 1e-3, (score, c["score"])
    assert (int(seq[0][-1]) == 1) == c["ended"]


# ---- serving modes of the TFM head on a BiLSTM memory ----------------------------------------------------------------------
@pytest.mark.parametrize("cname", ["VBT", "RBTP"])
def test_pipelined_and_grouped_decodes_equal_the_synchronous_call(cname):
    H = synth.crop_shape(cname)[0]
    cfg, m = engine_model(cname, S.L)
    imgs = [synth.synth_images(B, H, W, seed=900 + i).to(DEV) for i, (B, W) in enumerate([(3, 96), (3, 96), (5, 64), (2, 128), (3, 96)])]
    with torch.no_grad():
        ref = [tuple(t.clone() for t in m(x, _go(x.shape[0]), is_train=False)[:2]) for x in imgs]
        for chains, group, mixed in [(1, 1, False), (2, 1, False), (2, 2, False), (2, 3, True)]:
            m.pipelined, m.decode_chains, m.decode_group, m.decode_group_mixed = True, chains, group, mixed
            got = [m(x, _go(x.shape[0]), is_train=False)[:2] for x in imgs]
            m.synchronize()
            torch.cuda.synchronize()
            for i, ((p, l), (rp, rl)) in enumerate(zip(got, ref)):
                assert torch.equal(p, rp) and torch.equal(l, rl), (chains, group, mixed, i)
        m.pipelined, m.decode_group, m.decode_group_mixed = False, 1, False
        p, l, _ = m(imgs[0], _go(3), is_train=False)
    assert torch.equal(p, ref[0][0]) and torch.equal(l, ref[0][1])
    assert m.engine().supports_ragged_groups()  # d_model 256: the mixed group above really was one step loop


def test_beam_search_over_two_crop_widths_equals_single_calls():
    cfg, m = engine_model("VBT", S.L, 1234, 1.0, beam_size=3)
    a = synth.synth_images(2, 32, 96, seed=920).to(DEV)
    b = synth.synth_images(3, 32, 64, seed=921).to(DEV)
    with torch.no_grad():
        single = [m(x[i:i + 1], _go(1), is_train=False, is_test=True)[:2] for x in (a, b) for i in range(x.shape[0])]
        tensor = m.beam_search_batch(a) + m.beam_search_batch(b)
        m.pipelined = True
        mixed = m.beam_search_batch([a, b])
        m.pipelined = False
    assert m.engine().supports_ragged_beam()
    assert len(single) == len(tensor) == len(mixed) == 5
    for i, (s, t, x) in enumerate(zip(single, tensor, mixed)):
        assert torch.equal(s[0], t[0]) and torch.equal(s[0], x[0]), i
        assert s[1] == t[1] == x[1], i


def test_vgg_flat_memory_keeps_serving_tensor_by_tensor():
    """d_model 512: no ragged groups / ragged beam; pipelined forwards and the list form of beam_search_batch still return
    what the synchronous single calls return."""
    cfg, m = engine_model("VT", S.L, 1234, 4.0, beam_size=3)
    a = synth.synth_images(2, 32, 96, seed=930).to(DEV)
    b = synth.synth_images(1, 64, 64, seed=931).to(DEV)
    with torch.no_grad():
        single = [m(x[i:i + 1], _go(1), is_train=False, is_test=True)[:2] for x in (a, b) for i in range(x.shape[0])]
        mixed = m.beam_search_batch([a, b])
        m.opt["beam_size"] = 1
        ref = [tuple(t.clone() for t in m(x, _go(x.shape[0]), is_train=False)[:2]) for x in (a, b)]
        m.pipelined, m.decode_group, m.decode_group_mixed = True, 2, True
        got = [m(x, _go(x.shape[0]), is_train=False)[:2] for x in (a, b)]
        m.synchronize()
        torch.cuda.synchronize()
    assert not m.engine().supports_ragged_groups() and not m.engine().supports_ragged_beam()
    for s, x in zip(single, mixed):
        assert torch.equal(s[0], x[0]) and s[1] == x[1]
    for (p, l), (rp, rl) in zip(got, ref):
        assert torch.equal(p, rp) and torch.equal(l, rl)


# ---- the crop proj_feat cannot take -------------------------------------------------------------------------------------------
def test_32_pixel_crop_under_mean_height_false_raises_and_writes_nothing():
    c = S.stack_case("raises", "vbtp_32px")
    assert c["type"] == "RuntimeError"
    cfg, m = engine_model("VBTP", S.L)
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=1000).to(DEV)
    with pytest.raises(RuntimeError, match=r"height 3 .*height 1"):
        with torch.no_grad():
            m(img, _go(c["B"]), is_train=False)
    eng = m.engine()
    T, d = eng.encoder_shape(c["H"], c["W"])[:2]
    memory = torch.full((c["B"], T, d), -7.25, device=DEV)
    rc = eng.lib.d2t_encode(eng.ctx, _lib.ptr(img), c["B"], c["H"], c["W"], _lib.ptr(memory), _lib.stream_of(img))
    torch.cuda.synchronize()
    assert rc == _lib.D2T_EINVAL
    msg = eng.lib.d2t_last_error(eng.ctx).decode()
    assert "height 3" in msg and "height 1" in msg
    assert bool((memory == -7.25).all())
    m.train()
    with pytest.raises(RuntimeError, match=r"height 3 .*height 1"):
        m(img, torch.ones(c["B"], 5, dtype=torch.long, device=DEV))
    m.eval()
    ok = synth.synth_images(2, 64, 96, seed=1000).to(DEV)  # the context still serves
    with torch.no_grad():
        preds, _, _ = m(ok, _go(2), is_train=False)
    assert np.array_equal(preds.cpu().numpy(), S.stack_arrays("vbtp_greedy")["tokens"])


# ---- training ------------------------------------------------------------------------------------------------------------
def _step(m, img, text):
    m.train()
    m.zero_grad()
    _, preds, _ = m(img.to(DEV), text[:, :-1].to(DEV))  # forward_step, engine/training.py:88
    cost = torch.nn.functional.cross_entropy(preds.view(-1, preds.shape[-1]), text[:, 1:].to(DEV).contiguous().view(-1),
                                             ignore_index=0, reduction="none")
    loss = cost.mean()
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), preds.detach()


def _grad_sample_index(key, numel):  # tools/make_golden.py grad_sample_index
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    return torch.randint(0, numel, (min(48, numel),), generator=g)


def _check_train_step(m, c, z, loss, preds):
    """What tests/test_train_gpu.py asks of c0_train_step / t1_train_step against their fixtures, in fp32 arithmetic; the
    tensors downstream of every ReLU / max-pool decision also value by value on the fixture's samples."""
    assert abs(float(loss) - c["loss"]) <= 1e-4 * max(1.0, abs(c["loss"]))
    assert np.abs(preds.cpu().numpy() - z["logits"]).max() <= 1e-3
    bufs = dict(m.named_buffers())
    stats = [k[3:] for k in z if k.startswith("bn:")]
    assert stats
    for k in stats:
        assert np.abs(bufs[k].cpu().numpy() - z["bn:" + k]).max() <= 1e-4 * max(1.0, float(np.abs(z["bn:" + k]).max())), k
    assert int(bufs[next(k for k in bufs if k.endswith("num_batches_tracked"))]) == 1
    params = dict(m.named_parameters())
    assert sorted(k for k, p in params.items() if p.grad is not None) == sorted(c["grad_norms"])
    for k, (norm, _) in c["grad_norms"].items():
        assert params[k].grad.shape == params[k].shape
        assert abs(float(params[k].grad.double().norm()) - norm) <= 3e-2 * max(norm, 1e-6), k
    if c["config"] in ("VBAP",):
        strict = [k for k in params if ".generator." in k]
        assert len(strict) == 2
    else:
        last = max(int(k.split("layers.")[1].split(".")[0]) for k in params if "model.layers." in k)
        strict = [k for k in params if k.startswith("predicter.Prediction.proj.")
                  or (f"model.layers.{last}." in k and ("linear2" in k or "norm3" in k))]
        assert len(strict) == 6
    for k in strict:
        want = torch.from_numpy(z["g:" + k]).double()
        got = params[k].grad.reshape(-1)[_grad_sample_index(k, params[k].numel()).to(DEV)].double().cpu()
        assert float((got - want).abs().max()) <= 1e-4 * max(float(want.abs().max()), 1e-12), k


@pytest.mark.parametrize("name", ["vbt_train_step", "vt_train_step", "vbtp_train_step", "vbap_train_step"])
def test_train_step_matches_reference_fixture(name):
    c, z = S.stack_case("train_step", name), S.stack_arrays(name)
    cfg, m = engine_model(c["config"], S.L, c["wseed"])
    m.conv_precision = "fp32"
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"])
    loss, preds = _step(m, img, torch.from_numpy(z["text"]))
    _check_train_step(m, c, z, loss, preds)
    if name in ("vbtp_train_step", "vbap_train_step"):
        g = m.featextractor.proj_feat.weight.grad
        assert tuple(g.shape) == (512, 1536) and tuple(m.featextractor.proj_feat.bias.grad.shape) == (512,)
        assert c["proj_feat_grad_shapes"]["featextractor.proj_feat.weight"] == [512, 1536]
        # every entry by the fixture's samples: the (3, 1) filter's gradient comes back in the Linear's own [C, 3C] order
        k = "featextractor.proj_feat.weight"
        want = torch.from_numpy(z["g:" + k]).double()
        got = g.reshape(-1)[_grad_sample_index(k, g.numel()).to(DEV)].double().cpu()
        assert float((got - want).norm()) <= 3e-2 * float(want.norm())
    m.eval()  # the model still serves inference, with the updated running statistics
    with torch.no_grad():
        out = m(img.to(DEV), _go(c["B"]), is_train=False)
    assert out[0].shape == (c["B"], S.L + 1)


def test_unused_proj_feat_gets_no_gradient():
    """mean_height False with Seq = None: the reference builds proj_feat and never reads it.  The same step as vt_train_step
    (the extra layer changes nothing), and the layer's .grad stays None."""
    c, z = S.stack_case("train_step", "vt_train_step"), S.stack_arrays("vt_train_step")
    cfg, m = engine_model("VTP", S.L, c["wseed"])
    m.conv_precision = "fp32"
    assert "featextractor.proj_feat.weight" in m.state_dict()
    loss, preds = _step(m, synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]), torch.from_numpy(z["text"]))
    _check_train_step(m, c, z, loss, preds)
    assert m.featextractor.proj_feat.weight.grad is None and m.featextractor.proj_feat.bias.grad is None


@pytest.mark.parametrize("cname", ["VBTD", "VBAD"])
def test_dropout_and_scheduled_sampling_on_the_new_stacks(cname):
    """Decoder-layer dropout (TFM) and droprate + teacher_forcing (Attn) behind proj_feat + BiLSTM: masks are drawn, the step is
    reproducible under the same seeds and differs under others, every gradient is finite.  (The engine's Philox stream
    advances with every forward under one seed, as torch's generator does, and starts over when the seed changes.)"""
    base = "vbtp_train_step" if cname == "VBTD" else "vbap_train_step"
    c, z = S.stack_case("train_step", base), S.stack_arrays(base)
    cfg, m = engine_model(cname, S.L, c["wseed"])
    img, text = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]), torch.from_numpy(z["text"])
    runs = []
    for seed in (5, 6, 5):
        torch.manual_seed(seed)
        random.seed(seed)
        loss, preds = _step(m, img, text)
        if cname == "VBTD":
            assert m._engine.mask_count() > 0
        grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert "featextractor.proj_feat.weight" in grads
        runs.append((float(loss), preds.clone()))
    assert runs[0][0] == runs[2][0] and torch.equal(runs[0][1], runs[2][1])
    assert not torch.equal(runs[0][1], runs[1][1])
    assert abs(runs[0][0] - c["loss"]) > 1e-3  # not the step without dropout


def test_fused_adamw_refreshes_proj_feat_in_the_engine():
    from doc2tex_amd import optim as O
    c, z = S.stack_case("train_step", "vbtp_train_step"), S.stack_arrays("vbtp_train_step")
    cfg, m = engine_model(c["config"], S.L, c["wseed"])
    img, text = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]), torch.from_numpy(z["text"])
    opt = O.create_optimizer(m, opt="adamw", lr=1e-3, weight_decay=0.01, momentum=0.9, filter_bias_and_bn=True, max_grad_norm=5.0)
    assert isinstance(opt, O.FusedAdamW)
    _, before = _step(m, img, text)
    eng, uploads = m._engine, m._engine.weight_uploads
    old = m.featextractor.proj_feat.weight.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    for name in ("featextractor.proj_feat.weight", "featextractor.proj_feat.bias"):
        p = dict(m.named_parameters())[name]
        raw = torch.empty_like(p, dtype=torch.float32).contiguous()
        eng.read_weight(name, raw)
        assert torch.equal(raw, p.detach()), name
    assert not torch.equal(old, m.featextractor.proj_feat.weight.detach())
    _, after = _step(m, img, text)
    assert eng.weight_uploads == uploads and not torch.equal(before, after)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.eval()
    cfg2, fresh = engine_model(c["config"], S.L, c["wseed"])
    fresh.load_state_dict(sd)
    with torch.no_grad():  # the packed (3, 1) filter follows the stepped weight
        a = m.forward_encoder(img.to(DEV))[0]
        b = fresh.forward_encoder(img.to(DEV))[0]
    assert torch.equal(a, b)


# ---- the proj_feat layer alone ----------------------------------------------------------------------------------------------
def _rule(name, y, y64, e32):
    err, mx = float((y.double().cpu() - y64).abs().max()), float(y64.abs().max())
    print(f"{name}: e32 {e32:.3e} err {err:.3e} ratio {err / e32 if e32 > 0 else 0.0:.2f} max {mx:.3e}")
    assert err <= 8.0 * e32 + 1e-6 * mx, f"{name}: |y - y64| = {err:.3e}, e32 = {e32:.3e}, max |y64| = {mx:.3e}"


@pytest.mark.parametrize("B,Wp", [(1, 1), (2, 1), (1, 5), (2, 5), (1, 23), (2, 23)])
def test_proj_feat_operator_against_float64(B, Wp):
    """proj_feat as the engine runs it -- a convolution with window (3, 1), stride 1, no padding over the NHWC map [B, 3, W',
    512] -- through d2t_op_conv2d (forward, as tests/test_ops_gpu.py calls it) and d2t_op_train_conv (the training node: forward,
    data gradient, weight gradient in the Linear's [C, 3C] layout, bias gradient), fp32 arithmetic, against float64 of the
    reference's flatten(-2) + F.linear.  W' = 1 is a GEMM of B rows; no width here fills a tile."""
    lib = _lib.require_device()
    Cc = 512
    x, w, b, dy = S.proj_feat_case(B, Wp, C=Cc)
    y64, e32 = S.proj_feat_refs(x, w, b, dy)
    xg = x.permute(0, 2, 3, 1).contiguous().to(DEV)                       # NHWC [B, 3, W', C]
    w_oihw = w.view(Cc, Cc, 3, 1)
    w_ohwi = w_oihw.permute(0, 2, 3, 1).contiguous().to(DEV)              # d2t_op_conv2d takes OHWI
    wg, bg, dyg = w.contiguous().to(DEV), b.to(DEV), dy.contiguous().to(DEV)  # dy [B, W', C] = NHWC [B, 1, W', C]
    y = torch.full((B, 1, Wp, Cc), float("nan"), device=DEV)
    rc = lib.d2t_op_conv2d(_lib.ptr(xg), _lib.ptr(w_ohwi), _lib.ptr(bg), None, _lib.ptr(y), B, 3, Wp, Cc, Cc, 3, 1, 1, 1, 0, 0,
                           _lib.ACT_NONE, _lib.stream_of(xg))
    assert rc == 0
    torch.cuda.synchronize()
    _rule("proj_fwd", y.view(B, Wp, Cc), y64["y"], e32["y"])
    y2 = torch.full_like(y, float("nan"))
    dx = torch.full((B, 3, Wp, Cc), float("nan"), device=DEV)
    dw = torch.full_like(wg, float("nan"))
    db = torch.full((Cc,), float("nan"), device=DEV)
    rc = lib.d2t_op_train_conv(_lib.ptr(xg), _lib.ptr(wg), _lib.ptr(bg), None, None, None, _lib.ptr(dyg), _lib.ptr(y2),
                               _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), None, None, None, B, 3, Wp, Cc, Cc, 3, 1, 1, 1, 0, 0, 0, 0,
                               _lib.stream_of(xg))
    assert rc == 0
    torch.cuda.synchronize()
    _rule("proj_train_fwd", y2.view(B, Wp, Cc), y64["y"], e32["y"])
    _rule("proj_dx", dx.permute(0, 3, 1, 2), y64["dx"], e32["dx"])
    assert tuple(dw.shape) == (Cc, 3 * Cc)
    _rule("proj_dw", dw, y64["dw"], e32["dw"])
    _rule("proj_db", db, y64["db"], e32["db"])


@pytest.mark.parametrize("B,Wp", [(1, 1), (2, 5), (2, 23)])
def test_proj_feat_operator_in_split_bf16(B, Wp):
    """The arithmetic the engine runs proj_feat in by default (d2t_op_conv2d_bf16x3: fp32 rows split on the fly; the training
    node with bf16x3 = 1).  Bound from the formats, element by element: an operand is hi + lo + a residue below 2^-16 of it
    (two 8-bit significands), and the kernel drops lo * lo, so a product is off by at most (2 * 2^-16 + 2^-16 + 2^-32) < 4 *
    2^-16 of |x| |w|; the fp32 accumulation of K terms adds (K + 4) * 2^-24 of the same sum -- both times the sum of the
    absolute products, which float64 evaluates on the absolute operands."""
    lib = _lib.require_device()
    Cc = 512
    x, w, b, dy = S.proj_feat_case(B, Wp, C=Cc, seed=1)
    y64, _ = S.proj_feat_refs(x, w, b, dy)
    a64, _ = S.proj_feat_refs(x.abs(), w.abs(), b.abs(), dy.abs())
    K = max(3 * Cc, B * Wp)
    factor = 4 * 2.0 ** -16 + (K + 4) * 2.0 ** -24
    xg = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    w_ohwi = w.view(Cc, Cc, 3, 1).permute(0, 2, 3, 1).contiguous().to(DEV)
    wg, bg, dyg = w.contiguous().to(DEV), b.to(DEV), dy.contiguous().to(DEV)
    y = torch.full((B, 1, Wp, Cc), float("nan"), device=DEV)
    rc = lib.d2t_op_conv2d_bf16x3(_lib.ptr(xg), _lib.ptr(w_ohwi), _lib.ptr(bg), None, _lib.ptr(y), B, 3, Wp, Cc, Cc, 3, 1, 1, 1, 0,
                                  0, _lib.ACT_NONE, _lib.stream_of(xg))
    assert rc == 0
    y2, dx = torch.full_like(y, float("nan")), torch.full((B, 3, Wp, Cc), float("nan"), device=DEV)
    dw, db = torch.full_like(wg, float("nan")), torch.full((Cc,), float("nan"), device=DEV)
    rc = lib.d2t_op_train_conv(_lib.ptr(xg), _lib.ptr(wg), _lib.ptr(bg), None, None, None, _lib.ptr(dyg), _lib.ptr(y2),
                               _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), None, None, None, B, 3, Wp, Cc, Cc, 3, 1, 1, 1, 0, 0, 0, 1,
                               _lib.stream_of(xg))
    assert rc == 0
    torch.cuda.synchronize()
    for nm, got, key in (("fwd", y.view(B, Wp, Cc), "y"), ("train_fwd", y2.view(B, Wp, Cc), "y"), ("dx", dx.permute(0, 3, 1, 2), "dx"),
                         ("dw", dw, "dw")):
        excess = (got.double().cpu() - y64[key]).abs() - factor * a64[key]
        print(f"proj_bf16x3_{nm}: max err {float((got.double().cpu() - y64[key]).abs().max()):.3e}, "
              f"largest err / bound {float(((got.double().cpu() - y64[key]).abs() / (factor * a64[key])).max()):.3f}")
        assert float(excess.max()) <= 0.0, nm
    _rule("proj_bf16x3_db", db, y64["db"], S.proj_feat_refs(x, w, b, dy)[1]["db"])  # a column sum: plain fp32 in both modes
