"""CPU: pins the references of tests/train_gemm_refs.py (what tests/test_train_gemm_ops_gpu.py holds the weight-gradient,
BatchNorm, LayerNorm, stem and data-movement kernels against) to torch.autograd on the float64 ops -- F.conv2d, F.linear,
F.batch_norm(training=True), F.layer_norm -- at 1e-12 relative, summed over the chunks where a reference is chunked; the two
operand splits to each other and to their defining properties; the two fp32 summation orders to a plain restatement; and the
S / chunk choice of Tr::wgrad (d2t_op_wgrad_plan, host only) to its contract."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_record_refs as CR
import train_gemm_refs as G
from doc2tex_amd import _lib

F64 = torch.float64
REL = 1e-12


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b):
    err, mx = float((a - b).abs().max()), float(b.abs().max())
    assert a.shape == b.shape and err <= REL * max(mx, 1e-300), f"{err:.3e} against max {mx:.3e}"


def _nchw(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("name", list(G.GEOMS))
@pytest.mark.parametrize("S, chunk", [(1, 96), (3, 32), (6, 16)])
def test_wgrad_ref_is_conv2d_weight_gradient(name, S, chunk):
    geom = G.GEOMS[name]
    KH, KW, SH, SW, PH, PW = geom
    B, H, W, Cin, Cout = 2, 6, 8, 8, 12
    OH, OW = G.out_size(H, W, geom)
    P = B * OH * OW
    S = (P + chunk - 1) // chunk
    g = _gen(7)
    x = torch.randn(B * H * W, Cin + 4, generator=g, dtype=F64)    # ldb > N
    dz = torch.randn(P, Cout + 4, generator=g, dtype=F64)          # lda > M
    w = torch.zeros(Cout, Cin, KH, KW, dtype=F64, requires_grad=True)
    y = F.conv2d(_nchw(x[:, :Cin], B, H, W), w, stride=(SH, SW), padding=(PH, PW))
    (y * _nchw(dz[:, :Cout], B, OH, OW)).sum().backward()
    for mode in G.MODES:
        part = G.wgrad_ref(dz, x, Cout, Cin, S, chunk, G.src_rows(B, H, W, geom), mode)
        assert part.shape == (S, KH * KW, Cout, Cin)
        _close(G.reduce_ref(part, 1, mode=mode), w.grad.reshape(Cout, Cin, KH * KW))  # OIHW: dst[m][n][tap]
    dst = torch.randn(Cout, Cin, KH * KW, generator=g, dtype=F64)
    _close(G.reduce_ref(part, 1, dst=dst), dst + w.grad.reshape(Cout, Cin, KH * KW))


def test_wgrad_ref_is_linear_weight_gradient():
    g = _gen(8)
    P, K, N = 45, 20, 12
    x, dy = torch.randn(P, K, generator=g, dtype=F64), torch.randn(P, N, generator=g, dtype=F64)
    w = torch.zeros(N, K, dtype=F64, requires_grad=True)
    (F.linear(x, w) * dy).sum().backward()
    part = G.wgrad_ref(dy, x, N, K, 2, 32)
    _close(G.reduce_ref(part, 0), w.grad)
    _close(G.abs_product(dy, x, N, K, 1, 64)[0, 0], dy.abs().t() @ x.abs())


def test_splits_agree_and_reconstruct():
    """the records' split and wgrad_bf16x3_kernel's split are the same function of an fp32 value; hi has 8 significant bits,
    |x - hi| < 2^-7 |x|, |x - hi - lo| <= 2^-8 |x - hi|: the two roundings of the derived bound"""
    g = _gen(9)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g).float(),
                   torch.tensor(CR.edge_values()[np.isfinite(CR.edge_values())])]).numpy()
    h1, l1 = G.split4_bf16(x)
    h2, l2 = G.split_records(x)
    assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(l1.view(np.uint32), l2.view(np.uint32))
    assert not (h1.view(np.uint32) & 0xFFFF).any() and not (l1.view(np.uint32) & 0xFFFF).any()
    x64, h64, l64 = x.astype(np.float64), h1.astype(np.float64), l1.astype(np.float64)
    nz = (x64 != 0) & (np.abs(x64) >= 2.0 ** -100)  # (normal values; the bound is for the normal range)
    assert (np.abs(x64 - h64)[nz] < 2.0 ** -7 * np.abs(x64)[nz]).all()
    assert (np.abs(x64 - h64 - l64)[nz] <= 2.0 ** -8 * np.abs(x64 - h64)[nz]).all()
    assert (np.abs(x64 - h64 - l64)[nz] <= 2.0 ** -15 * np.abs(x64)[nz]).all()


@pytest.mark.parametrize("S", [1, 2, 255, 256, 257, 600])
def test_fp32_summation_orders(S):
    rng = np.random.default_rng(S)
    part = rng.standard_normal((S, 4, 3, 2)).astype(np.float32)
    dst = rng.standard_normal((3, 2, 4)).astype(np.float32)
    seq = np.zeros((4, 3, 2), np.float32)
    for z in range(S):
        seq = seq + part[z]
    assert np.array_equal(G.reduce_ordered_fp32(part, 1), seq.transpose(1, 2, 0))
    assert np.array_equal(G.reduce_ordered_fp32(part, 1, dst), dst + seq.transpose(1, 2, 0))
    # the tree, one output at a time in scalar arithmetic
    flat = part.reshape(S, -1)
    want = np.zeros(flat.shape[1], np.float32)
    for i in range(flat.shape[1]):
        red = [np.float32(0)] * 256
        for z in range(S):
            red[z % 256] = np.float32(red[z % 256] + flat[z, i])
        o = 128
        while o:
            for t in range(o):
                red[t] = np.float32(red[t] + red[t + o])
            o //= 2
        want[i] = red[0]
    assert np.array_equal(G.reduce_tree_fp32(part, 1), want.reshape(4, 3, 2).transpose(1, 2, 0))
    err = np.abs(G.reduce_tree_fp32(part, 1).astype(np.float64) - part.astype(np.float64).sum(0).transpose(1, 2, 0)).max()
    assert err <= S * 2.0 ** -24 * np.abs(part).sum(0).max()


@pytest.mark.parametrize("R, relu, with_res", [(37, False, False), (37, True, True), (1, False, False), (2, True, False)])
def test_batchnorm_refs_are_batch_norm_autograd(R, relu, with_res):
    g = _gen(10 + R)
    Cc, eps, mom = 8, 1e-5, 0.1
    z = (torch.randn(R, Cc, generator=g, dtype=F64) + 3.0).requires_grad_(True)
    gamma = torch.randn(Cc, generator=g, dtype=F64).requires_grad_(True)
    beta = torch.randn(Cc, generator=g, dtype=F64).requires_grad_(True)
    res = torch.randn(R, Cc, generator=g, dtype=F64).requires_grad_(True) if with_res else None
    dy = torch.randn(R, Cc, generator=g, dtype=F64)
    rm, rv = torch.randn(Cc, generator=g, dtype=F64), torch.rand(Cc, generator=g, dtype=F64) + 0.5
    k = G.bn_chain_ref(z.detach(), gamma.detach(), beta.detach(), None if res is None else res.detach(), relu, dy, eps, mom, rm, rv)
    if R == 1:  # F.batch_norm refuses one value per channel in training mode: the definition alone
        assert float(k["var"].abs().max()) == 0.0
        _close(k["run_var"], 0.9 * rv)
        _close(k["y"], torch.clamp(beta.detach()[None, :], min=0) if relu else beta.detach()[None, :].expand(1, Cc))
        return
    trm, trv = rm.clone(), rv.clone()
    t = F.batch_norm(z.t()[None], trm, trv, gamma, beta, training=True, momentum=mom, eps=eps)[0].t()
    if res is not None:
        t = t + res
    y = torch.relu(t) if relu else t
    (y * dy).sum().backward()
    _close(k["y"], y.detach())
    _close(k["run_mean"], trm)
    _close(k["run_var"], trv)
    _close(k["dz"], z.grad)
    _close(k["s0"], beta.grad)
    _close(k["s1"], gamma.grad)
    if res is not None:
        _close(k["g"], res.grad)
    # the column-sum pairs
    m, q = k["mean"], k["rstd"]
    s0, s1 = G.colsums_ref(G.CR_SUM_SQ, z.detach())
    _close(z.detach()[0] + s0 / R, m)
    assert float((s1 / R - (s0 / R) ** 2 - k["var"]).abs().max()) <= 1e-12 * float((s1 / R).max())
    b0, b1 = G.colsums_ref(G.CR_BN_BWD, dy, k["y"] if relu else None, z.detach(), m, q)
    _close(b0, beta.grad)
    _close(b1, gamma.grad)
    _close(G.colsums_ref(G.CR_SUM, dy)[0], dy.sum(0))


@pytest.mark.parametrize("rows, D, with_add", [(5, 128, False), (3, 256, True), (1, 512, True)])
def test_layernorm_refs_are_layer_norm_autograd(rows, D, with_add):
    g = _gen(20 + D)
    eps = 1e-5
    x = (torch.randn(rows, D, generator=g, dtype=F64) + 2.0).requires_grad_(True)
    gamma = torch.randn(D, generator=g, dtype=F64).requires_grad_(True)
    beta = torch.randn(D, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(rows, D, generator=g, dtype=F64)
    add = torch.randn(rows, D, generator=g, dtype=F64) if with_add else None
    y = F.layer_norm(x, (D,), gamma, beta, eps)
    (y * dy).sum().backward()
    for mode in G.MODES:
        k = G.ln_ref(x.detach(), gamma.detach(), beta.detach(), eps, mode)
        _close(k["y"], y.detach())
        dx = G.ln_bwd_ref(dy, x.detach(), k["mean"], k["rstd"], gamma.detach(), add, mode)
        _close(dx, x.grad if add is None else x.grad + add)
        s0, s1 = G.colsums_ref(G.CR_LN_BWD, dy, None, x.detach(), k["mean"], k["rstd"], mode)
        _close(s0, beta.grad)
        _close(s1, gamma.grad)


@pytest.mark.parametrize("Cin, Cout, chunk", [(1, 32, 7), (3, 64, 1), (3, 32, 1000)])
def test_stem_refs_are_conv2d(Cin, Cout, chunk):
    g = _gen(30 + Cin)
    B, H, W = 2, 5, 7
    img = torch.randn(B, Cin, H, W, generator=g, dtype=F64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=F64).requires_grad_(True)
    dz = torch.randn(B * H * W, Cout, generator=g, dtype=F64)
    y = F.conv2d(img, w, padding=1)
    (y * _nchw(dz, B, H, W)).sum().backward()
    for mode in G.MODES:
        _close(G.stem_ref(img, w.detach(), mode), y.detach().permute(0, 2, 3, 1).reshape(-1, Cout))
        part = G.stem_wgrad_ref(img, dz, chunk, mode)
        n = part.shape[0]
        assert part.shape == ((B * H * W + chunk - 1) // chunk, 9 * Cin, Cout)
        # reduced as the step does: wgrad partials with M = Cout, N = 1, layout 1 -> [Cout][1][9 Cin] = OIHW
        _close(G.reduce_ref(part.reshape(n, 9 * Cin, Cout, 1), 1, mode=mode).reshape(Cout, Cin, 3, 3), w.grad)


@pytest.mark.parametrize("name", ["3x3p1", "2x2s21p01", "2x2s2"])
def test_dilate_and_flip_give_the_data_gradient(name):
    """dx of a (strided) convolution = the stride-1 valid convolution of the zero-dilated dz, placed KH-1-PH / KW-1-PW in, with
    the flipped IOHW filter: pins dilate_ref and flip_oihw_ref together"""
    geom = G.GEOMS[name]
    KH, KW, SH, SW, PH, PW = geom
    g = _gen(40)
    B, H, W, Cin, Cout = 2, 6, 7, 3, 5
    OH, OW = G.out_size(H, W, geom)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(Cout, Cin, KH, KW, generator=g, dtype=F64)
    dy = torch.randn(B, OH, OW, Cout, generator=g, dtype=F64)
    (F.conv2d(x, w, stride=(SH, SW), padding=(PH, PW)) * dy.permute(0, 3, 1, 2)).sum().backward()
    d = G.dilate_ref(dy, H + KH - 1, W + KW - 1, SH, SW, KH - 1 - PH, KW - 1 - PW)
    _close(F.conv2d(d.permute(0, 3, 1, 2), G.flip_oihw_ref(w)), x.grad)


def test_row_movers():
    g = _gen(50)
    src = torch.randn(5, 6, generator=g)
    assert torch.equal(G.pad_cols_ref(src, 8), F.pad(src, (0, 2)))
    assert torch.equal(G.pad_cols_ref(src, 6), src)
    dst = torch.randn(5, 9, generator=g)
    out = G.copy2d_ref(src, dst, 4)
    assert torch.equal(out[:, :4], src[:, :4]) and torch.equal(out[:, 4:], dst[:, 4:])


# ---------------------------------------------------------------------------------------------------------------------
# Tr::wgrad's choice of S and chunk (host only: needs the library, no device)
# ---------------------------------------------------------------------------------------------------------------------
PLAN_SHAPES = [  # (M, N, taps, records, tile)
    (512, 512, 9, 1, (256, 256)), (256, 128, 9, 1, (256, 128)), (128, 128, 9, 1, (128, 128)), (384, 128, 1, 1, (128, 128)),
    (128, 64, 9, 1, (128, 64)), (64, 32, 9, 1, (64, 32)),
    (512, 512, 9, 0, (128, 128)), (500, 512, 1, 0, (128, 128)), (64, 32, 9, 0, (64, 64)), (4, 512, 1, 0, (64, 64)),
    (2048, 512, 1, 0, (128, 128))]
PLAN_P = sorted(set(list(range(1, 70)) + [127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 32767, 32768, 32769,
                                           65535, 65537, 99999, 131072, 200001, 262144, 299999, 300000] +
                    list(range(1, 300000, 1777))))


@pytest.mark.parametrize("M, N, taps, records, tile", PLAN_SHAPES)
def test_wgrad_plan_contract(M, N, taps, records, tile):
    lib = _lib.load()
    out = (C.c_int64 * 4)()
    seen = set()
    for P in PLAN_P:
        assert lib.d2t_op_wgrad_plan(P, M, N, taps, records, out) == 0
        S, chunk = out[0], out[1]
        assert (out[2], out[3]) == tile
        assert S >= 1 and chunk >= 32 and chunk % 32 == 0, (P, S, chunk)
        assert S * chunk >= P > (S - 1) * chunk, (P, S, chunk)  # every row in a chunk, no chunk empty
        if not records:
            assert S <= 64, (P, S)
        seen.add(S)
    assert len(seen) > 1  # the sweep reaches a split


def test_wgrad_plan_refusals():
    lib = _lib.load()
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    for args in [(0, 64, 64, 1, 0), (10, 0, 64, 1, 0), (10, 64, 64, 0, 0), (10, 96, 96, 9, 1), (10, 64, 64, 9, 1)]:
        assert lib.d2t_op_wgrad_plan(*args, out) == 1
    assert list(out) == [-1] * 4
