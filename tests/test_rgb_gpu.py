"""GPU: three-channel models (input_channel 3, `rgb: True`) through every layer that sees the channels -- the stem kernels
at op level, the colour fixtures generated from the reference (tools/make_golden_rgb.py) through doc2tex_amd.Model in both
arithmetic modes, the training step, the headline size against the restatement, pre-processing -- and the grey path, which
must still produce the bits it produced before the stem kernels were templated on the channel count."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD, engine_model, oracle_state_dict
from doc2tex_amd import _lib, synth
from doc2tex_amd import dist as ddist
from oracle import preprocess as P
from oracle import restatement as R
from test_parity_gpu import LOGIT_TOL, MEM_TOL, _score_tol
from test_rgb_cpu import CASES, MANIFESTS, MIN_GAP, case, colour_images, names, rgb_train_labels
from test_train_gpu import _check_instance, _l2_errors, _rel, _ReplayDecisions, _step, _train_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4  # test_train_ops_gpu.py's bound: max |engine - fp64| relative to max |fp64|, fp32 arithmetic


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _set_precision(m, precision):
    if precision != "default":
        m.conv_precision = precision
    return m


# ---- 5. op level ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cout", [(2, 20, 36, 32), (2, 37, 53, 32), (2, 37, 53, 64), (1, 128, 512, 32), (1, 128, 512, 64),
                                        (3, 1, 1, 32), (1, 5, 3, 64)])
def test_stem_conv_cin3(B, H, W, Cout):
    """stem_kernel<3> through d2t_op_conv2d against float64 conv + bias + ReLU; inputs scaled as in
    test_ops_gpu.py::test_stem_conv_cin1, whose bound (1e-5) this is.  A 27-tap fp32 multiply-add chain in the kernel's order
    (Cout 64, 37x53, five seeds) is at most 2.1e-6 from float64 on the CPU, so the bound leaves 5x room.  The image goes in
    as the encoder takes it, NCHW planar; the weights OHWI like every d2t_op_conv2d call."""
    lib = _lib.require_device()
    x = _rand(B, 3, H, W, seed=8)
    w = _rand(Cout, 3, 3, 3, seed=9, scale=0.3)
    b = _rand(Cout, seed=10, scale=0.1)
    xd, wd, bd = x.contiguous().to(DEV), w.permute(0, 2, 3, 1).contiguous().to(DEV), b.to(DEV)
    y = torch.full((B, H, W, Cout), float("nan"), device=DEV)
    rc = lib.d2t_op_conv2d(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), None, _lib.ptr(y), B, H, W, 3, Cout, 3, 3, 1, 1, 1, 1,
                           _lib.ACT_RELU, _lib.stream_of(xd))
    assert rc == 0
    torch.cuda.synchronize()
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), 1, 1)).float()
    err = float((y.cpu().permute(0, 3, 1, 2) - ref).abs().max())
    print(f"[stem cin3 {B}x{H}x{W} -> {Cout}] max |d| = {err:.3e}")
    assert err <= 1e-5, err


def test_stem_conv_refuses_other_channel_counts():
    lib = _lib.require_device()
    x, w, y = torch.zeros(1, 2, 8, 8, device=DEV), torch.zeros(32, 3, 3, 2, device=DEV), torch.zeros(1, 8, 8, 32, device=DEV)
    assert lib.d2t_op_conv2d(_lib.ptr(x), _lib.ptr(w), None, None, _lib.ptr(y), 1, 8, 8, 2, 32, 3, 3, 1, 1, 1, 1, 0,
                             _lib.stream_of(x)) != 0


@pytest.mark.parametrize("B,H,W", [(2, 20, 36), (2, 37, 53), (3, 48, 64)])
def test_stem_conv_cin3_backward(B, H, W):
    """conv0_1 (3 -> 32 channels, 3x3) + BatchNorm + ReLU: stem_raw_kernel<3> and stem_wgrad_kernel<32, 3> through
    d2t_op_train_conv, built like test_train_ops_gpu.py::test_stem_conv_backward, its TOL for y, dW, dgamma, dbeta."""
    lib = _lib.require_device()
    Cout = 32
    x = _rand(B, 3, H, W, seed=8)
    w = _rand(Cout, 3, 3, 3, seed=9, scale=0.3)
    gamma = torch.rand(Cout, generator=torch.Generator().manual_seed(10)) + 0.5
    beta = _rand(Cout, seed=11, scale=0.1)
    dy = _rand(B, Cout, H, W, seed=12)
    wd, gd, bd = (t.double().requires_grad_(True) for t in (w, gamma, beta))
    z = F.batch_norm(F.conv2d(x.double(), wd, None, 1, 1), None, None, gd, bd, training=True, eps=1e-5)
    dy = dy.masked_fill(z.detach().abs() < 1e-3, 0.0)
    grads = torch.autograd.grad(F.relu(z), [wd, gd, bd], dy.double())
    xg, wg, dyg = x.contiguous().to(DEV), w.to(DEV), dy.permute(0, 2, 3, 1).contiguous().to(DEV)
    gg, bg = gamma.to(DEV), beta.to(DEV)
    y = torch.empty((B, H, W, Cout), device=DEV)
    dw, dgam, dbet = torch.full_like(wg, float("nan")), torch.empty(Cout, device=DEV), torch.empty(Cout, device=DEV)
    rc = lib.d2t_op_train_conv(_lib.ptr(xg), _lib.ptr(wg), None, _lib.ptr(gg), _lib.ptr(bg), None,
                               _lib.ptr(dyg), _lib.ptr(y), None, _lib.ptr(dw), None, _lib.ptr(dgam), _lib.ptr(dbet), None,
                               B, H, W, 3, Cout, 3, 3, 1, 1, 1, 1, 1, 0, _lib.stream_of(xg))
    assert rc == 0
    torch.cuda.synchronize()
    errs = {"y": _rel(y.cpu().permute(0, 3, 1, 2), F.relu(z).detach()), "dw": _rel(dw, grads[0]),
            "dgamma": _rel(dgam, grads[1]), "dbeta": _rel(dbet, grads[2])}
    print(f"[stem cin3 backward {B}x{H}x{W}] {errs}")
    assert max(errs.values()) <= TOL, errs
    for ci in range(3):  # every input plane reaches its own slice of the weight gradient
        assert _rel(dw[:, ci], grads[0][:, ci]) <= TOL and float(dw[:, ci].abs().max()) > 0.0


# ---- 6. fixtures through Model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["default", "fp32"])
@pytest.mark.parametrize("name", names("greedy"))
def test_greedy_vs_reference_fixture(name, precision):
    c = case("greedy", name)
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], c["end_bias"])
    _set_precision(m, precision)
    img = colour_images(c).cuda()
    text = torch.full((c["B"], 1), R.GO, dtype=torch.long, device=DEV)
    with torch.no_grad():
        mem, shape, pad = m.forward_encoder(img)
        preds, logits, _ = m(img, text, is_train=False, is_test=c["is_test"])
    torch.cuda.synchronize()
    assert list(mem.shape) == c["mem_shape"]
    assert (list(shape) if shape else None) == c["output_shape"]
    assert (list(pad) if pad else None) == c["feat_pad"]
    rows = z["mem_rows"].tolist()
    dmem = float(np.abs(mem.cpu()[:, rows].numpy() - z["mem_sample"]).max()) / max(1.0, c["mem_absmax"])
    dl = float(np.abs(logits.cpu()[:, z["logit_steps"].tolist()].numpy() - z["logits_sample"]).max())
    print(f"[{name}, {m.effective_conv_precision()}] memory rel err {dmem:.3e}, max |dlogit| {dl:.3e}")
    assert dmem <= MEM_TOL[m.effective_conv_precision()], dmem
    assert preds.shape[1] == c["steps"]
    assert np.array_equal(preds.cpu().numpy(), z["tokens"]), "greedy token ids differ from the reference"
    assert dl <= LOGIT_TOL, dl


@pytest.mark.parametrize("precision", ["default", "fp32"])
@pytest.mark.parametrize("kind,name", [(k, n) for k in ("beam", "attn_beam") for n in names(k)])
def test_beam_vs_reference_fixture(kind, name, precision):
    c = case(kind, name)
    cfg, m = engine_model(c["config"], c["max_seq_len"], c["wseed"], c["end_bias"], beam_size=c["beam_size"])
    _set_precision(m, precision)
    img = colour_images(c, B=1).cuda()
    text = (torch.full((1, 1), R.GO, dtype=torch.long, device=DEV) if kind == "beam"
            else torch.zeros(1, c["max_seq_len"] + 1, dtype=torch.long, device=DEV))
    with torch.no_grad():
        seq, score, _ = m(img, text, is_train=False, is_test=True)
        seq2, score2, _ = m(img, text, is_train=False, is_test=True)
    print(f"[{name}, {m.effective_conv_precision()}] score {float(score)} vs {c['score']}")
    assert seq.shape[0] == 1 and seq[0].tolist() == c["seq"], (seq, c["seq"])
    tol = _score_tol(m, len(c["seq"])) if kind == "beam" else 1e-3  # as test_parity_gpu.py bounds the two searches
    assert abs(float(score) - c["score"]) <= tol, (score, c["score"])
    assert torch.equal(seq, seq2) and float(score) == float(score2)


# ---- 7. training step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("train_step"))
def test_train_step_matches_reference_fixture(name):
    """The assertions of test_train_gpu.py::test_train_step_matches_reference_fixture on the colour fixtures, plus the stem's
    weight gradient: [*, 3, 3, 3] with every channel slice filled."""
    c = case("train_step", name)
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, sd = oracle_state_dict(c["config"], MANIFESTS[c["config"]], c["max_seq_len"], c["wseed"])
    img = colour_images(c)
    text = rgb_train_labels(c)
    oloss, ologits, ograds, obn = R.train_step_grads(cfg, sd, img, text)
    _, m = _train_model(c["config"], c["max_seq_len"], c["wseed"])
    loss, preds = _step(m, img, text)
    print(f"[{name}] loss {float(loss)} vs {c['loss']}, max |dlogit| {np.abs(preds.cpu().numpy() - z['logits']).max():.3e}")
    assert abs(float(loss) - c["loss"]) <= 1e-4 * max(1.0, abs(c["loss"]))
    assert np.abs(preds.cpu().numpy() - z["logits"]).max() <= 1e-3
    bufs = dict(m.named_buffers())
    for k, v in obn.items():
        assert _rel(bufs[k], v) <= 1e-4, k
        assert np.abs(bufs[k].cpu().numpy() - z["bn:" + k]).max() <= 1e-4 * max(1.0, float(np.abs(z["bn:" + k]).max())), k
    assert int(bufs[next(k for k in bufs if k.endswith("num_batches_tracked"))]) == 1
    _check_instance(m, ograds)
    params = dict(m.named_parameters())
    for k, (norm, _) in c["grad_norms"].items():
        assert abs(float(params[k].grad.double().norm()) - norm) <= 3e-2 * max(norm, 1e-6), k
    stem = next(k for k in params if k.endswith(("conv0_1.weight", "ConvNet.0.weight")))
    g = params[stem].grad
    assert list(g.shape[1:]) == [3, 3, 3]
    for ci in range(3):
        assert float(g[:, ci].abs().max()) > 0.0, ci
    m.eval()  # the model still serves inference, now with the updated running statistics
    with torch.no_grad():
        omem, _, _ = R.forward_encoder(cfg, {**sd, **obn}, img, faithful=True)
        mem, _, _ = m.forward_encoder(img.cuda())
    assert float((mem.cpu() - omem).abs().max()) / max(1.0, float(omem.abs().max())) <= 1e-4


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_gradients_with_the_engines_own_decisions_replayed(precision):
    """T2C with the float64 oracle replaying the engine's ReLU / max-pool decisions: every gradient tensor, the three-channel
    stem's included, within the bounds test_train_gpu.py states (2e-4 fp32 / 1e-3 split-bf16 relative L2)."""
    c = case("train_step", "rgb_t2c_train_step")
    cfg, sd = oracle_state_dict(c["config"], MANIFESTS[c["config"]], c["max_seq_len"], c["wseed"])
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    _, m = _train_model(c["config"], c["max_seq_len"], c["wseed"], precision=precision)
    img = colour_images(c)
    text = rgb_train_labels(c)
    loss, preds = _step(m, img, text)
    with _ReplayDecisions(m._engine) as rep:
        oloss, ologits, ograds, _ = R.train_step_grads(cfg, sd64, img.double(), text)
    assert rep.n >= 30
    assert abs(float(loss) - float(oloss)) <= 1e-4 * max(1.0, abs(float(oloss)))
    assert float((preds.cpu().double() - ologits).abs().max()) <= 1e-3
    l2 = _l2_errors(m, ograds)
    k, v = max(l2.items(), key=lambda kv: kv[1])
    stem = next(n for n in l2 if n.endswith("conv0_1.weight"))
    print(f"[replayed decisions, T2C, {precision}] worst tensor {k}: {v:.3e}; stem {l2[stem]:.3e}")
    assert v <= (2e-4 if precision == "fp32" else 1e-3), (k, v)


# ---- 8. headline size -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["default", "fp32"])
def test_headline_size_vs_the_restatement(precision):
    """C2C at 128x512, B = 2, against the restatement run here on the host, first 20 steps: logits within 1e-3, memory within
    1e-4 of its scale, tokens exact at every step where the restatement's own top-2 gap is >= 2e-3.  At most 1 in 10 of the
    40 (row, step) pairs may fall below that gap (the image seed was chosen on the CPU so that the restatement meets it)."""
    c = CASES["c2c_parity"]
    n = c["steps"]
    cfg, m = engine_model(c["config"], c["max_seq_len"], c["wseed"])
    _set_precision(m, precision)
    ocfg, sd = oracle_state_dict(c["config"], MANIFESTS[c["config"]], c["max_seq_len"], c["wseed"])
    img = colour_images(c)
    text = torch.full((c["B"], 1), R.GO, dtype=torch.long)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    with torch.no_grad():
        omem, _, _ = R.forward_encoder(ocfg, sd, img, faithful=False)
        op, ol, _ = R.forward(ocfg, sd, img, text, is_test=False, faithful=False)
        mem, _, _ = m.forward_encoder(img.cuda())
        p, l, _ = m(img.cuda(), text.cuda(), is_train=False)
    torch.cuda.synchronize()
    p, l, mem = p.cpu()[:, :n], l.cpu()[:, :n], mem.cpu()
    op, ol = op[:, :n], ol[:, :n]
    top2 = ol.topk(2, dim=-1).values
    sure = (top2[..., 0] - top2[..., 1]) >= MIN_GAP
    dmem = float((mem - omem).abs().max()) / max(1.0, float(omem.abs().max()))
    dl = float((l - ol).abs().max())
    print(f"[C2C 128x512, {m.effective_conv_precision()}] memory rel err {dmem:.3e}, max |dlogit| {dl:.3e}, "
          f"pairs compared {int(sure.sum())} of {sure.numel()}")
    assert op.tolist() == c["tokens"]  # the restatement here is the one the seed was chosen with
    assert int((~sure).sum()) * 10 <= sure.numel()
    assert dl <= LOGIT_TOL, dl
    assert dmem <= 1e-4, dmem
    assert torch.equal(p[sure], op[sure])


# ---- 9. the grey path is untouched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["default", "fp32"])
def test_grey_path_bits_are_those_of_the_build_before_the_channel_template(precision):
    """T2 memory, logits and tokens equal, bitwise, the arrays dumped on an MI355X from the build of the commit before the
    stem kernels took the channel count as a template parameter (tests/golden/rgb_grey_baseline.npz; DESIGN.md names the
    commit).  The 1-channel instantiation is meant to be the same code and the inference path is deterministic."""
    z = np.load(os.path.join(GOLD, "rgb_grey_baseline.npz"))
    cfg, m = engine_model("T2", 12)
    _set_precision(m, precision)
    img = synth.synth_images(2, 48, 64, seed=1000).cuda()
    text = torch.full((2, 1), R.GO, dtype=torch.long, device=DEV)
    with torch.no_grad():
        mem, _, _ = m.forward_encoder(img)
        preds, logits, _ = m(img, text, is_train=False)
    torch.cuda.synchronize()
    assert m.effective_conv_precision() == ("fp32" if precision == "fp32" else "bf16x3")
    assert np.array_equal(mem.cpu().numpy(), z[precision + "_memory"])
    assert np.array_equal(logits.cpu().numpy(), z[precision + "_logits"])
    assert np.array_equal(preds.cpu().numpy(), z[precision + "_tokens"])


# ---- 10. shape errors -------------------------------------------------------------------------------------------------
def test_channel_count_of_the_image_must_be_the_models():
    text = torch.full((2, 1), R.GO, dtype=torch.long, device=DEV)
    grey, colour = synth.synth_images(2, 48, 64, seed=7).cuda(), synth.synth_images(2, 48, 64, seed=7, channels=3).cuda()
    for cname, good, bad in (("T2", grey, colour), ("T2C", colour, grey)):
        cfg, m = engine_model(cname, 12)
        with torch.no_grad():
            want = m(good, text, is_train=False)
            with pytest.raises(ValueError):
                m(bad, text, is_train=False)
            with pytest.raises(ValueError):
                m.forward_encoder(bad[:, :1].expand(-1, 2, -1, -1))
            got = m(good, text, is_train=False)  # the model serves a correct call afterwards
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        m.train()
        with pytest.raises(ValueError):
            m(bad, synth.synth_labels(2, max_len=12).cuda()[:, :-1])
        m.eval()


def test_weights_whose_stem_disagrees_with_the_config_are_refused():
    """d2t_finalize_weights: a 1-channel conv0_1 under in_channels = 3 (and the reverse) is an error, not a wrong answer."""
    from doc2tex_amd import Model
    for cname, other in (("T2C", "T2"), ("T2", "T2C")):
        m = Model(synth.make_config(cname, device="cuda")).cuda().eval()
        k = "seqmodeler.SequenceModeling.patch_embed.backbone.ConvNet.conv0_1"
        stem = getattr(Model(synth.make_config(other)).seqmodeler.SequenceModeling.patch_embed.backbone.ConvNet, "conv0_1")
        m.seqmodeler.SequenceModeling.patch_embed.backbone.ConvNet.conv0_1 = stem.cuda()
        ch = 3 if cname == "T2C" else 1
        with pytest.raises(RuntimeError, match="conv0_1"):
            m.forward_encoder(synth.synth_images(1, 48, 64, seed=1, channels=ch).cuda())
        assert k + ".weight" in m.state_dict()


# ---- 11. pre-processing -----------------------------------------------------------------------------------------------
def _opt(rgb, **kw):
    o = {"imgH": None, "imgW": None, "max_dimension": [48, 64], "min_dimension": [32, 32], "mean": 0.5, "std": 0.5,
         "rgb": rgb, "pad": False, "use_resizer": False, "device": "cuda"}
    o.update(kw)
    return o


@pytest.mark.parametrize("variant", ["demo", "api"])
def test_preprocessor_rgb(variant):
    """`rgb: True` as the reference's resize() has it: the image is opened as "L", resized, converted to "RGB" and normalised
    with one scalar mean / std, so the three planes are equal and each is bitwise the plane `rgb: False` returns -- which is
    itself still bitwise the oracle's.  The result feeds T2C.forward_encoder as it is, on the device."""
    from doc2tex_amd.preprocess import Preprocessor, resize
    grey, colour = Preprocessor(_opt(False), variant), Preprocessor(_opt(True), variant)
    cfg, m = engine_model("T2C", 12)
    ocfg, sd = oracle_state_dict("T2C", MANIFESTS["T2C"], 12)
    done = 0
    # at min_dimension, inside the range, and above max_dimension in one / both directions (the LANCZOS path)
    for i, (h, w) in enumerate([(32, 32), (32, 64), (40, 60), (48, 64), (40, 48), (100, 150), (48, 200), (301, 77), (96, 128)]):
        img = synth.synth_formula_image(h, w, 7000 + i)
        try:
            want = P.resize(img, _opt(False), variant=variant)
        except UnboundLocalError:  # the api copy's get_divisible_size: raised whatever `rgb` says
            with pytest.raises(UnboundLocalError):
                grey(img)
            with pytest.raises(UnboundLocalError):
                colour(img)
            continue
        g, c3 = grey(img), colour(img)
        assert g.shape == (1, 1) + want.shape[2:] and np.array_equal(g.cpu().numpy(), want)  # rgb: False is what it was
        assert c3.shape == (1, 3) + want.shape[2:] and c3.is_cuda and c3.dtype == torch.float32 and c3.is_contiguous()
        for ch in range(3):
            assert torch.equal(c3[:, ch], g[:, 0]), (h, w, ch)
        assert torch.equal(resize(None, img, _opt(True), variant=variant), c3)
        with torch.no_grad():
            mem, _, _ = m.forward_encoder(c3)  # no copy on the host
            omem, _, _ = R.forward_encoder(ocfg, sd, c3.cpu(), faithful=False)
        assert float((mem.cpu() - omem).abs().max()) / max(1.0, float(omem.abs().max())) <= MEM_TOL[m.effective_conv_precision()]
        done += 1
        if h > 48 or w > 64:
            assert c3.shape[2] <= 48 and c3.shape[3] <= 64
    assert done >= (5 if variant == "api" else 9)
    # below min_dimension: minmax_size(..., is_gray=False) leaves MODE / BACKGROUND unassigned (data_utils.py:75-79,
    # helper.py:124-126) -- not a ValueError, so resize() lets it through; with rgb: False the image is pasted on a canvas
    small = synth.synth_formula_image(20, 50, 7100)
    with pytest.raises(UnboundLocalError):
        colour(small)
    if variant == "demo":
        assert grey(small).shape[1] == 1
    # a batch: colour images of one output size share one [n, 3, H, W] bucket; the small one is reported, not raised
    imgs = [synth.synth_formula_image(40, 60, 7200 + i) for i in range(3)] + [small]
    tensors, errors = colour.batch(imgs)
    assert [e is None for e in errors] == [True, True, True, False] and isinstance(errors[3], UnboundLocalError)
    assert tensors[0]._base is not None and tensors[0]._base.shape[:2] == (3, 3)
    for t, im in zip(tensors[:3], imgs):
        assert torch.equal(t, colour(im))


def test_preprocessor_rgb_fixed_height():
    """`imgH` set (predict_utils.py:98-114): the grey pixels repeated to three planes, torchvision Normalize with 3-tuples of
    the same scalars, planes dropped only when `rgb` is false."""
    from doc2tex_amd.preprocess import Preprocessor
    img = synth.synth_formula_image(48, 64, 7300)
    g = Preprocessor(_opt(False, imgH=48), "api")(img)
    c3 = Preprocessor(_opt(True, imgH=48), "api")(img)
    assert c3.shape == (1, 3, 48, 64)
    for ch in range(3):
        assert torch.equal(c3[:, ch], g[:, 0])


# ---- 12. batch sharding -----------------------------------------------------------------------------------------------
def test_shards_of_a_colour_batch_decode_like_the_whole_batch():
    """doc2tex_amd.dist.decode_sharded slices [B,3,H,W] along the batch: every shard's tokens and logits are those of the
    whole batch (one process, the ranks one after the other)."""
    cfg, m = engine_model("T2C", 12)
    img = synth.synth_images(5, 48, 64, seed=77, channels=3).cuda()
    go = lambda n: torch.full((n, 1), R.GO, dtype=torch.long, device=DEV)
    with torch.no_grad():
        p_all, l_all, _ = m(img, go(5), is_train=False)
        for world in (2, 3):
            parts = [ddist.decode_sharded(lambda x: m(x, go(x.shape[0]), is_train=False)[0], img, rank=r, world=world, gather=False)
                     for r in range(world)]
            assert torch.equal(torch.cat(parts), p_all)
            lo, hi = ddist.shard_bounds(5, 1, world)
            assert torch.equal(m(img[lo:hi], go(hi - lo), is_train=False)[1], l_all[lo:hi])


def _colour_rank_program():
    import test_dist_rccl_gpu as D
    prog = D.RANK_PROGRAM.replace('engine_model("T2", 24', 'engine_model("T2C", 24')
    prog = prog.replace("seed=1001)", "seed=1001, channels=3)").replace("seed=1040)", "seed=1040, channels=3)", 1)
    assert prog.count('"T2C"') == 2 and prog.count("channels=3") == 2
    return D, prog


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
@pytest.mark.parametrize("mode", ["decode", "train"])
def test_colour_model_over_rccl_two_ranks(tmp_path, monkeypatch, mode):
    D, prog = _colour_rank_program()
    monkeypatch.setattr(D, "RANK_PROGRAM", prog)
    D._run_ranks(mode, tmp_path)


def test_colour_rank_program_with_one_rank(tmp_path, monkeypatch):
    """The two-rank program above as a one-rank RCCL world, so that it is known to work before a two-GPU machine sees it."""
    D, prog = _colour_rank_program()
    monkeypatch.setattr(D, "RANK_PROGRAM", prog)
    D._run_ranks("decode", tmp_path, world=1)
