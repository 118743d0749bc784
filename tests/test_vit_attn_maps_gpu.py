"""GPU: ViT self-attention maps through forward hooks on attn_drop (the reference's attention-rollout hook points,
tools/interpretation/vit_visualize.py:26-93): parity with the reference's maps (tests/golden/vitattn_*.npz,
tools/make_golden_vit_attn.py), long memories against the oracle's block inputs, the op-level kernel against float64
softmax, outputs unchanged with maps on, and the hook semantics."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD, engine_model, oracle_state_dict
from doc2tex_amd import Model, _lib, synth
from oracle import restatement as R

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "vitattn_cases.json")) as f:
    VA = json.load(f)
CASES = {c["case"]: c for c in VA["cases"]}
SP = "seqmodeler.SequenceModeling."
# Engine maps against the reference's (fp32 CPU), measured on an MI355X: max |dp| 1.0e-5 (default bf16x3 backbone) / 1.5e-6
# (fp32) on the full fixtures, 1.1e-6 / 1.0e-7 on the sampled C2 rows and row maxima; the bar leaves a wide margin.
ATOL = 1e-4


def _load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _drops(m):
    return [blk.attn.attn_drop for blk in m.seqmodeler.SequenceModeling.blocks]


def _collect(mods):
    """Forward hooks that record (block index, output); returns (records, handles)."""
    got, handles = [], []
    for i, mod in mods:
        handles.append(mod.register_forward_hook(lambda _m, _inp, out, i=i: got.append((i, out))))
    return got, handles


@pytest.mark.parametrize("precision", ["default", "fp32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_maps_match_reference(name, precision):
    c, z = CASES[name], _load(name)
    _, m = engine_model(c["config"], c["max_seq_len"], c["wseed"])
    if precision == "fp32":
        m.conv_precision = "fp32"
    got, handles = _collect(list(enumerate(_drops(m))))
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]).cuda()
    with torch.no_grad():
        m.forward_encoder(img)
    torch.cuda.synchronize()
    for h in handles:
        h.remove()
    assert [i for i, _ in got] == list(range(c["depth"]))
    maps = torch.stack([p for _, p in got]).cpu().numpy()
    assert maps.shape == (c["depth"], c["B"], c["heads"], c["T"], c["T"])
    if c["kind"] == "full":
        err = float(np.abs(maps - z["maps"]).max())
    else:
        rows = c["rows"]
        err = max(float(np.abs(maps[:, :, :, rows] - z["rows"]).max()), float(np.abs(maps.max(-1) - z["max"]).max()))
        # the argmax may differ only where two keys are within rounding of each other
        am = maps.argmax(-1)
        diff = am != z["argmax"]
        if diff.any():
            picked = np.take_along_axis(maps, z["argmax"][..., None].astype(np.int64), -1)[..., 0]
            assert float(np.abs(picked - maps.max(-1))[diff].max()) <= ATOL
    print(f"{name} ({precision}): max |dp| = {err:.2e}")
    assert err <= ATOL


def _oracle_maps(sd, x, i, heads):
    """float64 softmax(q k^T / sqrt(32)) of block i from its input x [B, T, C] (vision_transformer.py:61-76)."""
    p = f"{SP}blocks.{i}."
    x = x.double()
    h = F.layer_norm(x, (x.shape[-1],), sd[p + "norm1.weight"].double(), sd[p + "norm1.bias"].double(), 1e-6)
    qkv = F.linear(h, sd[p + "attn.qkv.weight"].double(), sd[p + "attn.qkv.bias"].double())
    B, T, C3 = qkv.shape
    q, k, _ = qkv.reshape(B, T, 3, heads, C3 // 3 // heads).permute(2, 0, 3, 1, 4)
    return ((q @ k.transpose(-2, -1)) * (q.shape[-1] ** -0.5)).softmax(-1)


def _block_input(sd, taps, i):
    if i > 0:
        return taps[f"block{i - 1}"]
    x = taps["patch"]
    x = torch.cat((sd[SP + "cls_token"].expand(x.shape[0], -1, -1), x), dim=1)
    return x + sd[SP + "pos_embed"][:, : x.shape[1]]  # ViTEncoderV3: flat prefix slice (vit_encoder.py:260)


def _c2_at(manifests, H, W, L=4):
    """The C2 stack built for max_dimension [H, W], engine (fp32 arithmetic) and oracle on the same seeded weights."""
    cfg = synth.make_config("C2", device="cuda", max_seq_len=L)
    cfg["max_dimension"] = [H, W]
    m = Model(cfg)
    m.load_state_dict(synth.synth_state_dict({k: v for k, v in m.state_dict().items()}), strict=False)
    m = m.cuda().eval()
    m.conv_precision = "fp32"
    ocfg, sd = oracle_state_dict("C2", manifests["C2"], L)
    ocfg["max_dimension"] = [H, W]
    gh, gw = R.vit_max_grid([H, W], (2, 2))
    sd = dict(sd)
    sd[SP + "pos_embed"] = R.sincos_2d_table(256, gh, gw)
    return m, ocfg, sd


@pytest.mark.parametrize("H,W,layers", [(448, 960, (0, 3)), (800, 800, (1, 5))])
def test_long_memories_against_oracle(manifests, H, W, layers):
    """The shipped 448 x 960 geometry (1695 tokens: 256-key chunks staged again for the maps, four query blocks per head) and
    800 x 800 (2526 tokens) -- two hooked layers each, against float64 maps recomputed from the oracle's block inputs."""
    m, ocfg, sd = _c2_at(manifests, H, W)
    img = synth.synth_images(1, H, W, seed=910 + H)
    drops = _drops(m)
    got, handles = _collect([(i, drops[i]) for i in layers])
    with torch.no_grad():
        mem = m.forward_encoder(img.cuda())[0]
        taps = {}
        R.forward_encoder(ocfg, sd, img, faithful=False, taps=taps)
    for h in handles:
        h.remove()
    T = mem.shape[1]
    assert T == {448: 1695, 800: 2526}[H]
    assert [i for i, _ in got] == list(layers)
    worst = 0.0
    for i, p in got:
        assert tuple(p.shape) == (1, 8, T, T) and p.is_contiguous()
        ref = _oracle_maps(sd, _block_input(sd, taps, i), i, 8)
        err = float((p.cpu().double() - ref).abs().max())
        worst = max(worst, err)
        assert float((p.double().sum(-1) - 1).abs().max()) <= 1e-5
    # measured on an MI355X: 448 x 960 1.7e-8, 800 x 800 1.6e-8
    print(f"{H}x{W}: T = {T}, max |dp| = {worst:.2e}")
    assert worst <= ATOL


@pytest.mark.parametrize("N", [1, 10, 31, 32, 33, 261, 512, 513, 1695, 4096])
def test_op_probs_against_float64(N):
    lib = _lib.require_device()
    B, heads = 2, 8
    C = heads * 32
    g = torch.Generator().manual_seed(31 + N)
    qkv = torch.randn(B, N, 3, heads, 32, generator=g).cuda()
    y0 = torch.empty((B, N, C), device="cuda")
    y1 = torch.empty((B, N, C), device="cuda")
    n, guard = B * heads * N * N, 4096
    buf = torch.full((n + guard,), -7.0, device="cuda")
    probs = buf[:n].view(B, heads, N, N)
    s = _lib.stream_of(qkv)
    assert lib.d2t_op_vit_attention(_lib.ptr(qkv), _lib.ptr(y0), B, N, heads, s) == 0
    assert lib.d2t_op_vit_attention_probs(_lib.ptr(qkv), _lib.ptr(y1), _lib.ptr(buf), B, N, heads, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)  # the attention output is bitwise the maps-off kernel's
    assert bool((buf[n:] == -7.0).all())  # nothing past [B, heads, N, N]
    q, k, _ = [t.double() for t in qkv.permute(2, 0, 3, 1, 4)]
    ref = ((q @ k.transpose(-2, -1)) * 32 ** -0.5).softmax(-1)
    err = float((probs.double() - ref).abs().max())
    rows = float((probs.double().sum(-1) - 1).abs().max())
    # measured on an MI355X: max |dp| <= 1.9e-7 and row sums within 5.9e-7 over all N
    print(f"N = {N}: max |dp| = {err:.2e}, max |row sum - 1| = {rows:.2e}")
    assert err <= 1e-5 and rows <= 1e-5


def test_op_probs_rejects_null():
    lib = _lib.require_device()
    qkv = torch.zeros(1, 4, 3, 8, 32, device="cuda")
    y = torch.empty(1, 4, 256, device="cuda")
    assert lib.d2t_op_vit_attention_probs(_lib.ptr(qkv), _lib.ptr(y), None, 1, 4, 8, _lib.stream_of(qkv)) != 0


@pytest.mark.parametrize("cname,H,W,L", [("C2", 128, 512, 20), ("TS0", 48, 64, 12)])
def test_maps_leave_results_unchanged(cname, H, W, L):
    """TFM (C2) and Attnv2 (TS0): memory, tokens and logits are bitwise the same with every block hooked, and after the
    hooks are removed."""
    _, m = engine_model(cname, L)
    img = synth.synth_images(2, H, W, seed=1300).cuda()
    text = (torch.full((2, 1), R.GO, dtype=torch.long) if cname == "C2" else torch.zeros(2, L + 1, dtype=torch.long)).cuda()

    def run():
        with torch.no_grad():
            mem = m.forward_encoder(img)[0].clone()
            preds, logits, _ = m(img, text, is_train=False)
        torch.cuda.synchronize()
        return mem, preds.clone(), logits.clone()

    base = run()
    got, handles = _collect(list(enumerate(_drops(m))))
    on = run()
    assert len(got) == 2 * len(handles)  # forward_encoder + forward
    for h in handles:
        h.remove()
    got.clear()
    off = run()
    assert not got
    for a, b, c in zip(base, on, off):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_hook_semantics(monkeypatch):
    c = CASES["vitattn_c2"]
    _, m = engine_model("C2", c["max_seq_len"], c["wseed"])
    img = synth.synth_images(2, 96, 384, seed=1301).cuda()
    drops = _drops(m)
    eng = m.engine()
    seen_maps = []
    real_encode = eng.encode

    def spy(image, attn_maps=None):
        seen_maps.append(attn_maps)
        return real_encode(image, attn_maps=attn_maps)

    monkeypatch.setattr(eng, "encode", spy)
    order, pre = [], []
    handles = [drops[4].register_forward_hook(lambda _m, _i, out: order.append((4, out))),
               drops[1].register_forward_hook(lambda _m, _i, out: order.append((1, out))),
               drops[1].register_forward_pre_hook(lambda _m, inp: pre.append(inp[0])),
               drops[4].register_forward_hook(lambda _m, args, kwargs, out: order.append(("kw", out)), with_kwargs=True)]
    with torch.no_grad():
        mem = m.forward_encoder(img)[0]
    T = mem.shape[1]
    # fired once per hooked block, in block order, with contiguous fp32 [B, heads, T, T]
    assert [o[0] for o in order] == [1, 4, "kw"]
    for _, p in order:
        assert p.dtype == torch.float32 and p.is_cuda and p.is_contiguous() and tuple(p.shape) == (2, 8, T, T)
    assert order[1][1] is order[2][1]
    assert len(pre) == 1 and pre[0] is order[0][1]  # the pre-hook sees the same tensor
    # only the hooked layers were allocated
    assert len(seen_maps) == 1 and [a is not None for a in seen_maps[0]] == [i in (1, 4) for i in range(6)]
    for h in handles:
        h.remove()
    # a hook that replaces the output, or a pre-hook that replaces the input, is refused
    h = drops[2].register_forward_hook(lambda _m, _i, out: out * 1.0)
    with pytest.raises(RuntimeError, match="replacement"), torch.no_grad():
        m.forward_encoder(img)
    h.remove()
    h = drops[0].register_forward_pre_hook(lambda _m, inp: (inp[0].clone(),))
    with pytest.raises(RuntimeError, match="replacement"), torch.no_grad():
        m.forward_encoder(img)
    h.remove()
    # training mode: no maps from the training kernels
    h = drops[0].register_forward_hook(lambda _m, _i, out: None)
    m.train()
    text = torch.zeros(2, c["max_seq_len"] + 1, dtype=torch.long, device="cuda")
    with pytest.raises(NotImplementedError, match="attn_train_fwd_kernel"):
        m(img, text)
    with pytest.raises(NotImplementedError, match="attn_train_fwd_kernel"):
        m.forward_encoder(img)
    m.eval()
    h.remove()


def _rollout(attentions):
    """VITAttentionRollout.rollout (head_fusion "max") written out.  discard_ratio 0: with the reference's 0.9 the discarded
    set is decided by a threshold among ~T^2 near-equal small values, which rounding-level differences reorder."""
    result = torch.eye(attentions[0].size(-1), dtype=torch.float64)
    for attention in attentions:
        fused = attention.max(axis=1)[0]
        eye = torch.eye(fused.size(-1), dtype=torch.float64)
        a = (fused + 1.0 * eye) / 2
        a = a / a.sum(dim=-1)
        result = torch.matmul(a, result)
    mask = result[0, 0, 1:]
    return mask / mask.max()


def test_rollout_matches_oracle_on_c2(manifests):
    c = CASES["vitattn_c2"]
    _, m = engine_model("C2", c["max_seq_len"], c["wseed"])
    m.conv_precision = "fp32"
    img = synth.synth_images(1, c["H"], c["W"], seed=c["iseed"])
    got, handles = _collect(list(enumerate(_drops(m))))
    with torch.no_grad():
        m.forward_encoder(img.cuda())
    for h in handles:
        h.remove()
    ocfg, sd = oracle_state_dict("C2", manifests["C2"], c["max_seq_len"], c["wseed"])
    taps = {}
    with torch.no_grad():
        R.forward_encoder(ocfg, sd, img, faithful=False, taps=taps)
    ours = _rollout([p.cpu().double() for _, p in got])
    ref = _rollout([_oracle_maps(sd, _block_input(sd, taps, i), i, c["heads"]) for i in range(c["depth"])])
    err = float((ours - ref).abs().max())
    print(f"C2 rollout: max |d mask| = {err:.2e}")  # measured on an MI355X: 1.9e-6
    assert err <= 1e-4
