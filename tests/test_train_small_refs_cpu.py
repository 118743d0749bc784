"""CPU: the kernel-layout references of tests/train_small_refs.py (what tests/test_train_small_ops_gpu.py compares the small
kernels of the training step with) agree in float64 with oracle.restatement -- the restatement tests/test_oracle_golden.py
ties to the reference project's recorded outputs -- and with F.interpolate; the Philox restatement reproduces the
known-answer vectors of Philox4x32-10 and passes two statistical checks; the three reduction orders agree in float64."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_small_refs as TR
from oracle import restatement as R

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _r(*s, seed=0, sc=1.0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed), dtype=F64) * sc


@pytest.mark.parametrize("B,H,W,C", [(2, 3, 5, 68), (1, 1, 1, 128), (2, 19, 27, 64)])
def test_global_context_is_the_restatement(B, H, W, C):
    P = {k: v.double() for k, v in TR.gc_params(C, seed=C + H).items()}
    x = _r(B, H * W, C, seed=1)
    p = "enc.layer1.1."
    m = p + "bottleneck_add."
    sd = {p + "global_cxt.weight": P["wg"].reshape(1, C, 1, 1), p + "global_cxt.bias": P["bg"],
          m + "fc1.weight": P["w1"].reshape(C, C, 1, 1), m + "fc1.bias": P["b1"], m + "norm.weight": P["ln_g"],
          m + "norm.bias": P["ln_b"], m + "fc2.weight": P["w2"].reshape(C, C, 1, 1), m + "fc2.bias": P["b2"]}
    want = R._global_context(x.reshape(B, H, W, C).permute(0, 3, 1, 2), sd, p, drop=None).permute(0, 2, 3, 1).reshape(B, H * W, C)
    assert float((want - x).abs().max()) > 0.1  # fc2.weight is not zero: the ConvMLP contributes
    for mode in TR.MODES:
        assert _rel(TR.global_context_ref(x, P, mode)["out"], want) <= 1e-12
    # the pool node alone, forward and autograd, in the three orders
    dctx = _r(B, C, seed=2)
    ref = TR.gc_pool_bwd_ref(x, P["wg"], P["bg"], dctx)
    for mode in TR.MODES[1:]:
        got = TR.gc_pool_bwd_ref(x, P["wg"], P["bg"], dctx, mode)
        for k in ("ctx", "dx", "dwg"):
            assert float((got[k] - ref[k]).abs().max()) <= 1e-12 * max(1.0, float(ref[k].abs().max())), (mode, k)
    assert abs(float(ref["dbg"])) <= 1e-12 * float(ref["dl"].abs().sum()) + 1e-300  # a softmax ignores a shift


def test_bcast_add_orders_agree():
    x, y, dout = _r(2, 37, 8, seed=3), _r(2, 8, seed=4), _r(2, 37, 8, seed=5)
    ref = TR.bcast_add_ref(x, y, dout)
    assert torch.equal(ref["out"], x + y[:, None]) and torch.equal(ref["dx"], dout)
    for mode in TR.MODES[1:]:
        got = TR.bcast_add_ref(x, y, dout, mode)
        assert torch.equal(got["out"], ref["out"]) and torch.equal(got["dx"], dout)
        assert _rel(got["dy"], ref["dy"]) <= 1e-12


@pytest.mark.parametrize("GH,GW,gh,gw,D", [(6, 40, 3, 17, 16), (6, 40, 6, 33, 16), (6, 40, 5, 40, 16), (6, 40, 1, 1, 8),
                                           (1, 9, 1, 5, 8), (4, 4, 7, 9, 8), (2, 3, 2, 2, 8)])
def test_table_resize_is_the_restatement_and_aten(GH, GW, gh, gw, D):
    src = _r(GH * GW, D, seed=GH * GW + gh)
    sh, sw = 1.0 / ((gh + 0.1) / GH), 1.0 / ((gw + 0.1) / GW)  # ATen's scales for a float64 input
    want = TR.bicubic_table_aten(src, GH, GW, gh, gw)
    for order in ("x_first", "y_first"):
        assert _rel(TR.bicubic_table_ref(src, GH, GW, gh, gw, sh, sw, order), want) <= 1e-12
    pos = torch.cat([_r(1, D, seed=9), src])[None]
    if not (gh * gw == GH * GW and gh == gw):
        got = R.interpolated_pos_embed(pos, (GH, GW), {"height": gh, "width": gw}, (1, 1))
        assert torch.equal(got[0, 0], pos[0, 0])
        assert _rel(TR.bicubic_table_ref(src, GH, GW, gh, gw, sh, sw), got[0, 1:]) <= 1e-12
    # the float scales of the kernels move the result by a rounding of the scale only
    fh, fw = TR.pos_scales(GH, GW, gh, gw)
    assert abs(fh - sh) <= 2.0 ** -24 * sh and abs(fw - sw) <= 2.0 ** -24 * sw
    assert _rel(TR.bicubic_table_ref(src, GH, GW, gh, gw, fh, fw), want) <= 1e-5


def test_tap_matrix_rows_sum_to_one_and_clamp():
    for scale, n_out, n_in in ((6 / 3.1, 3, 6), (1 / 1.1, 1, 1), (9 / 5.1, 5, 9), (4 / 7.1, 7, 4)):
        M = TR.tap_matrix(scale, n_out, n_in, F64)
        assert float((M.sum(1) - 1).abs().max()) <= 1e-14
    M = TR.tap_matrix(1 / 1.1, 1, 1, F64)  # a one-row table: every tap is the row
    assert M.shape == (1, 1) and abs(float(M) - 1.0) <= 1e-14


@pytest.mark.parametrize("B,L,V,D", [(3, 7, 11, 16), (1, 1, 5, 8)])
def test_embedding_is_the_restatement(B, L, V, D):
    g = torch.Generator().manual_seed(B + L)
    tgt = torch.randint(0, V, (B, L), generator=g)
    sd = {"p.word_embed.weight": _r(V, D, seed=1), "p.pos_enc.pe": _r(L + 3, D, seed=2)}
    want = R._embed(tgt, sd, "p.").reshape(B * L, D)
    got = TR.embed_ref(sd["p.word_embed.weight"], sd["p.pos_enc.pe"], tgt.reshape(-1), L, math.sqrt(D))
    assert _rel(got, want) <= 1e-12


def test_embedding_backward_ordered_sum_is_the_gradient():
    g = torch.Generator().manual_seed(7)
    rows, V, D, pad = 300, 9, 12, 0
    tok = torch.randint(0, V - 1, (rows,), generator=g)  # token V - 1 is absent
    dx = torch.randn(rows, D, generator=g)
    want = TR.embed_bwd_autograd(dx.double(), tok, V, 4.0, pad)
    got = TR.embed_bwd_ordered_fp32(dx, tok, V, 4.0, pad)
    assert float(got[pad].abs().max()) == 0.0 and float(got[V - 1].abs().max()) == 0.0
    assert float(want[pad].abs().max()) == 0.0 and float(want[V - 1].abs().max()) == 0.0
    assert _rel(got.double(), want) <= rows * 2.0 ** -24


# Known-answer vectors of Philox4x32-10 (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(w[0]) for w in TR.philox4x32_10(*ctr, *key)) == out


def test_philox_draw_layout():
    """counter = (group lo, group hi, stream lo, stream hi), key = (seed lo, seed hi); low half of a word first"""
    seed, stream = 0x0123456789ABCDEF, (1 << 40) + 1
    d = TR.dropout_draws(29, seed, stream)
    for grp in (0, 3):
        r = [int(w[0]) for w in TR.philox4x32_10(grp, 0, stream & 0xFFFFFFFF, stream >> 32, seed & 0xFFFFFFFF, seed >> 32)]
        want = [h for w in r for h in (w & 0xFFFF, w >> 16)]
        assert list(d[grp * 8:grp * 8 + 8]) == want[:len(d[grp * 8:grp * 8 + 8])]
    assert [TR.dropout_threshold(p) for p in (0.1, 0.25, 0.5, 0.0)] == [6554, 16384, 32768, 0]
    m = TR.dropout_mask_ref(29, 0.25, seed, stream)
    assert m.dtype == torch.uint8 and m.tolist() == [int(v >= 16384) for v in d]


def test_philox_keep_rate_and_stream_independence():
    n, p = 10 ** 6, 0.25
    a = TR.dropout_mask_ref(n, p, 1234, 5).numpy().astype(np.float64)
    b = TR.dropout_mask_ref(n, p, 1234, (3 << 16) | 5).numpy().astype(np.float64)
    keep = 1.0 - TR.dropout_threshold(p) / 65536.0
    assert keep == 0.75
    s = math.sqrt(keep * (1 - keep) / n)
    assert abs(a.mean() - keep) <= 5 * s and abs(b.mean() - keep) <= 5 * s
    agree = keep * keep + (1 - keep) ** 2  # independent masks agree where both keep or both drop
    assert agree == 0.625
    assert abs((a == b).mean() - agree) <= 5 * math.sqrt(agree * (1 - agree) / n)


def test_small_refs_orders_agree():
    x = _r(3, 6, 17, 8, seed=11)
    for mode in TR.MODES:
        assert _rel(TR.mean_h_ref(x, mode), x.mean(1)) <= 1e-12
        assert _rel(TR.sum_over_batch_ref(x.reshape(-1), 6 * 17 * 8, 100, mode), x.reshape(3, -1)[:, :100].sum(0)) <= 1e-12
        assert _rel(TR.sum_rows_strided_ref(x.reshape(-1, 8), 6 * 17, 4, mode), x.reshape(3, 6 * 17, 8)[:, 4].sum(0)) <= 1e-12
    src = _r(2 * 5, 4, seed=12)
    sc = TR.token_rows_ref(src, 2, 5, 1, scatter=True)
    assert sc.shape == (12, 4) and float(sc.reshape(2, 6, 4)[:, 0].abs().max()) == 0.0
    assert torch.equal(TR.token_rows_ref(sc, 2, 5, 1, scatter=False), src)
    xg = torch.linspace(-8, 8, 101, dtype=F64)
    y, dx = TR.ew_ref(xg, torch.ones_like(xg), 0)
    cdf = 0.5 * (1 + torch.erf(xg / math.sqrt(2)))
    assert _rel(y, xg * cdf) <= 1e-12
    assert _rel(dx, cdf + xg * torch.exp(-0.5 * xg * xg) / math.sqrt(2 * math.pi)) <= 1e-12
