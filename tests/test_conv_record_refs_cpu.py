"""CPU: the restatements of tests/conv_record_refs.py against independent torch operations -- `.to(torch.bfloat16)` and
`.half()` where the rule is round-to-nearest-even, integer shifts for the truncation, permutes for the layouts, F.max_pool2d /
F.conv2d / F.batch_norm for the operators -- at the edge values the record formats are documented for (conv_common.h)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_record_refs as R


def rand_values(n, seed):
    g = torch.Generator().manual_seed(seed)
    return np.concatenate([(torch.randn(n, generator=g) * s).numpy() for s in (1e-3, 1.0, 300.0)])


ALL = np.concatenate([R.edge_values(), rand_values(4000, 1)])


def t_bits16(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def test_bf16_rne_is_torch_bfloat16():
    x = ALL
    want = t_bits16(torch.from_numpy(x).to(torch.bfloat16))
    assert R.same_bits(R.bf16_rne_bits(x), want, "bf16")
    # the ties went to the even neighbour, the value beside a tie to the nearer one
    tie = np.array([0x3F808000, 0x3F818000, 0x3F808001], dtype=np.uint32).view(np.float32)
    assert list(R.bf16_rne_bits(tie)) == [0x3F80, 0x3F82, 0x3F81]


def test_f16_saturates_finite_values_and_passes_the_others():
    x = ALL
    t = torch.from_numpy(x)
    want = torch.where(torch.isfinite(t), t.clamp(-65504.0, 65504.0), t).half()
    assert R.same_bits(R.f16_sat_bits(x), t_bits16(want), "f16")
    got = R.f16_bits_to_f32(R.f16_sat_bits(np.array([65504, 65519, 65520, 1e5, -1e5, 3e38, np.inf, -np.inf], dtype=np.float32)))
    assert list(got) == [65504, 65504, 65504, 65504, -65504, 65504, np.inf, -np.inf]
    assert np.isnan(R.f16_bits_to_f32(R.f16_sat_bits(np.array([np.nan], dtype=np.float32))))[0]
    sub = np.array([2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24], dtype=np.float32)
    assert list(R.f16_sat_bits(sub)) == [1, 3, 1023, 0, 2]  # subnormals are kept; ties to even
    assert list(R.f16_sat_bits(np.array([0.0, -0.0], dtype=np.float32))) == [0, 0x8000]


def test_bf16_records_truncate_hi_and_round_lo():
    x = ALL
    hi, lo = R.split_act(x, 0)
    t = torch.from_numpy(x)
    want_hi = ((t.view(torch.int32) >> 16) & 0xFFFF).numpy().astype(np.uint16)  # truncation, not rounding
    assert np.array_equal(hi, want_hi)
    hi_f = (t.view(torch.int32) & -65536).view(torch.float32)
    want_lo = t_bits16((t - hi_f).to(torch.bfloat16))
    assert R.same_bits(lo, want_lo, "bf16")
    fin = np.isfinite(x)
    j = R.join_act(hi, lo, 0)
    assert np.all(np.abs(j[fin].astype(np.float64) - x[fin]) <= np.abs(x[fin]) * 2.0 ** -16)
    assert np.all(np.isnan(j[~fin]))  # Inf - Inf: a non-finite value reads back as NaN, never as a finite number
    # a remainder within 2^-9 of a whole step rounds UP to the step: lo is then a power of two of hi's last place
    near = np.float32(1.0 + 2.0 ** -7 * (1 - 2.0 ** -10))
    h, l = R.split_act(np.array([near]), 0)
    assert h[0] == 0x3F80 and R.bf16_bits_to_f32(l)[0] == np.float32(2.0 ** -7)


def test_f16_records():
    x = ALL
    t = torch.from_numpy(x)
    sat = torch.where(torch.isfinite(t), t.clamp(-65504.0, 65504.0), t)
    hi1, lo1 = R.split_act(x, 1)
    assert R.same_bits(hi1, t_bits16(sat.half()), "f16") and not lo1.any()
    hi2, lo2 = R.split_act(x, 2)
    assert np.array_equal(hi2, hi1)
    rem = t - sat.half().float()
    want_lo = torch.where(torch.isfinite(rem), rem.clamp(-65504.0, 65504.0), rem).half()
    assert R.same_bits(lo2, t_bits16(want_lo), "f16")
    assert np.array_equal(R.join_act(hi1, lo1, 1), R.f16_bits_to_f32(hi1), equal_nan=True)
    j = R.join_act(hi2, lo2, 2).astype(np.float64)
    ok = np.isfinite(x) & (np.abs(x) <= 65504.0) & (np.abs(x) >= 2.0 ** -3)  # (below, lo runs into fp16's subnormals)
    assert np.all(np.abs(j[ok] - x[ok]) <= np.abs(x[ok]) * 2.0 ** -21)
    # the MFMAs of the two-MFMA arithmetic read the hi half alone
    assert np.array_equal(R.mma_operand(hi2, lo2, 2), R.f16_bits_to_f32(hi2).astype(np.float64), equal_nan=True)


def test_weight_planes_round_hi_to_nearest():
    w = ALL
    t = torch.from_numpy(w)
    hi, lo = R.split_weight_bf16(w)
    th = t.to(torch.bfloat16)
    assert R.same_bits(hi, t_bits16(th), "bf16")
    assert R.same_bits(lo, t_bits16((t - th.float()).to(torch.bfloat16)), "bf16")
    tie = np.array([0x3F808000, 0x3F818000], dtype=np.uint32).view(np.float32)
    assert list(R.split_weight_bf16(tie)[0]) == [0x3F80, 0x3F82] and list(R.split_act(tie, 0)[0]) == [0x3F80, 0x3F81]
    h16, l16 = R.split_weight_f16(w)
    assert np.array_equal(h16, R.split_act(w, 2)[0]) and np.array_equal(l16, R.split_act(w, 2)[1])


@pytest.mark.parametrize("rows,C", [(1, 32), (3, 64), (257, 96)])
def test_plane_layout_is_one_record_per_row_and_group(rows, C):
    hi = np.arange(rows * C, dtype=np.uint32).reshape(rows, C).astype(np.uint16)
    lo = (hi ^ 0xFFFF).astype(np.uint16)
    p = R.to_planes(hi, lo)
    v = torch.from_numpy(p.astype(np.int32)).view(rows, C // 32, 2, 32)
    assert np.array_equal(v[:, :, 0].reshape(rows, C).numpy(), hi.astype(np.int32))
    assert np.array_equal(v[:, :, 1].reshape(rows, C).numpy(), lo.astype(np.int32))
    h2, l2 = R.from_planes(p, rows, C)
    assert np.array_equal(h2, hi) and np.array_equal(l2, lo)
    x = rand_values(rows * C // 3 + 1, 2)[:rows * C].reshape(rows, C)
    for fmt in (0, 1, 2):
        assert np.array_equal(R.values_of(R.records_of(x, fmt), rows, C, fmt), R.join_act(*R.split_act(x, fmt), fmt))


@pytest.mark.parametrize("B,OH,OW", [(1, 2, 2), (2, 4, 6), (3, 5, 7)])
def test_pooled_row_order(B, OH, OW):
    pix = torch.arange(B * OH * OW).view(B, OH, OW)[:, :OH // 2 * 2, :OW // 2 * 2]
    want = pix.reshape(B, OH // 2, 2, OW // 2, 2).permute(0, 1, 3, 2, 4).reshape(-1)
    assert np.array_equal(R.pooled_row_pixel(B, OH, OW), want.numpy())
    # rows 4 q .. 4 q + 3 are one window: their maximum is max_pool2d
    x = torch.randn(B, 1, OH, OW, generator=torch.Generator().manual_seed(3))
    rows = x.reshape(-1)[torch.from_numpy(R.pooled_row_pixel(B, OH, OW))]
    assert torch.equal(rows.view(-1, 4).max(1).values, F.max_pool2d(x, 2, 2).reshape(-1))


def test_row_remap_and_table_rows():
    B, rpi, stride, off = 3, 15, 16, 1
    rows = torch.arange(B * rpi)
    out = torch.full((B, stride), -1)
    out[:, off:off + rpi] = rows.view(B, rpi)
    idx = R.remap_rows(B * rpi, rpi, stride, off)
    got = torch.full((B * stride,), -1)
    got[torch.from_numpy(idx)] = rows
    assert torch.equal(got.view(B, stride), out)
    assert np.array_equal(R.remap_rows(7, 0, 0, 0), np.arange(7))
    assert np.array_equal(R.row_add_rows(B * rpi, rpi, 1), (torch.arange(rpi) + 1).repeat(B).numpy())
    assert np.array_equal(R.row_add_rows(5, 0, 2), np.full(5, 2))


@pytest.mark.parametrize("B,T,heads,hd,slabs", [(3, 37, 8, 32, 2), (1, 129, 3, 20, 6), (2, 5, 4, 64, 2)])
def test_head_split_index_is_a_permute(B, T, heads, hd, slabs):
    N = slabs * heads * hd
    plain = torch.arange(B * T * N).view(B, T, slabs, heads, hd)
    want = plain.permute(2, 0, 3, 1, 4).reshape(-1)
    out = torch.empty(B * T * N, dtype=torch.long)
    out[torch.from_numpy(R.kv_index(B, T, heads, hd, N)).reshape(-1)] = plain.reshape(-1)
    assert torch.equal(out, want)


@pytest.mark.parametrize("Cout,Cin,k", [(8, 64, 3), (4, 32, 1), (5, 3, 3), (6, 160, 2)])
def test_k_order_is_chunk_tap_channel(Cout, Cin, k):
    w = torch.randn(Cout, Cin, k, k, generator=torch.Generator().manual_seed(4))
    got = R.pack_rows(w.numpy())
    if Cin % 32:
        want = w.permute(0, 2, 3, 1).reshape(Cout, -1)
    else:
        want = w.view(Cout, Cin // 32, 32, k, k).permute(0, 1, 3, 4, 2).reshape(Cout, -1)
    assert np.array_equal(got, want.numpy())


def test_packed_rows_times_gathered_taps_is_conv2d():
    """the GEMM view: A[m][k] gathered in the same K order (second input's channels behind) times pack_rows is F.conv2d"""
    g = torch.Generator().manual_seed(5)
    B, H, W, Cin, Cout, Cin2 = 2, 5, 6, 64, 7, 32
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    x2 = torch.randn(B, Cin2, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    w2 = torch.randn(Cout, Cin2, 1, 1, generator=g, dtype=torch.float64)
    cols = F.unfold(x, 3, padding=1).view(B, Cin, 9, H * W)  # [b][c][tap][pixel]
    A = cols.view(B, Cin // 32, 32, 9, H * W).permute(0, 4, 1, 3, 2).reshape(B * H * W, -1)
    A = torch.cat([A, x2.permute(0, 2, 3, 1).reshape(B * H * W, Cin2)], 1)
    Wp = np.concatenate([R.pack_rows(w.numpy()), R.pack_rows(w2.numpy())], 1)
    got = A @ torch.from_numpy(Wp).T
    want = (F.conv2d(x, w, None, 1, 1) + F.conv2d(x2, w2)).permute(0, 2, 3, 1).reshape(B * H * W, Cout)
    assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("with_bias,with_bn", [(True, True), (False, True), (True, False), (False, False)])
def test_batchnorm_fold_is_batch_norm_of_conv2d(with_bias, with_bn):
    g = torch.Generator().manual_seed(6)
    Cout, Cin = 6, 4
    x = torch.randn(2, Cin, 5, 5, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    cb = torch.randn(Cout, generator=g, dtype=torch.float64) if with_bias else None
    gamma = torch.tensor([1.0, -0.5, 0.0, 2.0, 0.3, -1.0], dtype=torch.float64)
    beta, mean = torch.randn(Cout, generator=g, dtype=torch.float64), torch.randn(Cout, generator=g, dtype=torch.float64) * 3
    var = torch.rand(Cout, generator=g, dtype=torch.float64) * 10 + 1e-2
    eps = 1e-5
    y = F.conv2d(x, w, cb, 1, 1)
    if with_bn:
        y = F.batch_norm(y, mean, var, gamma, beta, False, 0.0, float(np.float32(eps)))
    wf, bf = R.bn_fold(w.numpy(), None if cb is None else cb.numpy(),
                       (gamma.numpy(), beta.numpy(), mean.numpy(), var.numpy()) if with_bn else None, eps)
    got = F.conv2d(x, torch.from_numpy(wf), torch.from_numpy(bf), 1, 1)
    assert float((got - y).abs().max()) <= 1e-12


def test_conv_ref_grid_override_reads_zeros_beyond_the_map():
    g = torch.Generator().manual_seed(7)
    B, H, W, Cin, Cout = 2, 5, 9, 8, 4
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 2, 2, generator=g, dtype=torch.float64)
    got = R.conv_ref(x.reshape(-1, Cin).numpy(), B, H, W, w.numpy(), None, (2, 2), (0, 0), 3, 5)
    xp = torch.zeros(B, 6, 10, Cin, dtype=torch.float64)
    xp[:, :H, :W] = x
    want = F.conv2d(xp.permute(0, 3, 1, 2), w, None, 2).permute(0, 2, 3, 1).reshape(-1, Cout)
    assert got.shape == (B * 15, Cout) and float(np.abs(got - want.numpy()).max()) <= 1e-12
    plain = R.conv_ref(x.reshape(-1, Cin).numpy(), B, H, W, w.numpy(), None, (2, 2), (0, 0))
    assert plain.shape == (B * 2 * 4, Cout)
    assert np.array_equal(R.finish_ref(np.array([-1.0, 2.0]), 1, np.array([0.5, 0.5])), np.array([0.0, 2.5]))
