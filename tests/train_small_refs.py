"""References of the small kernels of the training step (csrc/train_kernels.hip, posembed.hip, and the GlobalContext kernels
of ops.hip) written from each operation's definition, at the KERNELS' layouts (maps [B][H*W][C], tables [cell][D]).  Plain
torch on the CPU, any dtype: float64 is the reference, and the same functions at float32 give e32 (reduction orders "plain",
"rev", "chunk" as in tests/recurrent_refs.py).  Backward references are torch.autograd on the forward, never a formula.
Shared by tests/test_train_small_ops_gpu.py and tests/test_train_small_refs_cpu.py, which pins them to oracle.restatement,
to F.interpolate and to the known-answer vectors of Philox4x32-10.
"""
import numpy as np
import torch
import torch.nn.functional as F

from recurrent_refs import MODES, e32_of, mm, rsum  # noqa: F401  (re-exported)


# ---------------------------------------------------------------------------------------------------------------------
# GlobalContext (addon_module/visual_attention.py:147-165)
# ---------------------------------------------------------------------------------------------------------------------
def gc_pool_ref(x, wg, bg, mode="plain"):
    """x [B][HW][C], wg [C], bg [1] -> (ctx [B][C], logits [B][HW]): ctx[b] = sum_p softmax_p(x[b] . wg + bg)[p] x[b][p]"""
    logits = mm(mode, x, wg[:, None])[..., 0] + bg
    e = torch.exp(logits - logits.max(-1, keepdim=True).values)
    a = e / rsum(mode, e, -1)[:, None]
    return mm(mode, a[:, None, :], x)[:, 0], logits


def gc_pool_bwd_ref(x, wg, bg, dctx, mode="plain"):
    """forward and autograd of gc_pool_ref; dl = the gradient of the logits (its sum is dbg)"""
    x, wg, bg = (t.detach().clone().requires_grad_(True) for t in (x, wg, bg))
    ctx, logits = gc_pool_ref(x, wg, bg, mode)
    logits.retain_grad()
    ctx.backward(dctx)
    return dict(ctx=ctx.detach(), dx=x.grad, dwg=wg.grad, dbg=bg.grad, dl=logits.grad)


def bcast_add_ref(x, y, dout, mode="plain"):
    """out[b][p] = x[b][p] + y[b]; the sum over the positions that autograd forms for dy runs forwards ("plain"), backwards
    ("rev") or in 16 chunks ("chunk")"""
    x, y = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    if mode == "plain":
        out = x + y[:, None]
    elif mode == "rev":
        out = (x.flip(1) + y[:, None]).flip(1)
    else:
        out = torch.cat([c + y[:, None] for c in x.chunk(16, dim=1)], 1)
    out.backward(dout)
    return dict(out=out.detach(), dx=x.grad, dy=y.grad)


def global_context_ref(x, P, mode="plain"):
    """The whole block on x [B][HW][C]: x + fc2(relu(LayerNorm(fc1(ctx)))), eps 1e-5.  P: wg [C], bg [1], w1 / w2 [C][C],
    b1 / ln_g / ln_b / b2 [C] (any dtype; cast to x's)."""
    P = {k: v.to(x.dtype) for k, v in P.items()}
    C = x.shape[-1]
    ctx, _ = gc_pool_ref(x, P["wg"], P["bg"], mode)
    h = mm(mode, ctx, P["w1"].t()) + P["b1"]
    d = h - rsum(mode, h, -1)[:, None] / C
    var = rsum(mode, d * d, -1)[:, None] / C
    h = torch.relu(d / torch.sqrt(var + 1e-5) * P["ln_g"] + P["ln_b"])
    y = mm(mode, h, P["w2"].t()) + P["b2"]
    return dict(out=x + y[:, None], ctx=ctx)


def gc_params(C, seed, bg=0.1):
    """random block weights: wg ~ N(0, 2 / C) (the reference's kaiming scale), fc2.weight NOT zero"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(wg=r(C) * (2.0 / C) ** 0.5, bg=torch.tensor([bg]), w1=r(C, C) * C ** -0.5, b1=r(C) * 0.1,
                ln_g=1.0 + 0.2 * r(C), ln_b=r(C) * 0.1, w2=r(C, C) * C ** -0.5, b2=r(C) * 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# embedding rows (prediction_head/tfm.py:86-94)
# ---------------------------------------------------------------------------------------------------------------------
def embed_ref(E, pe, tok, L, scale):
    """x[r] = E[tok[r]] * scale + pe[r % L]"""
    return E[tok] * scale + pe[torch.arange(tok.numel()) % L]


def embed_bwd_autograd(dx, tok, V, scale, pad_id):
    """float64 autograd of E -> E[tok] * scale with the padding row masked (nn.Embedding padding_idx)"""
    E = torch.zeros(V, dx.shape[1], dtype=dx.dtype, requires_grad=True)
    (E[tok] * scale * (tok != pad_id)[:, None].to(dx.dtype)).backward(dx)
    return E.grad


def embed_bwd_ordered_fp32(dx, tok, V, scale, pad_id):
    """What the kernel's comment promises, evaluated on the host in fp32: per vocabulary row the hit rows added one after the
    other in ascending row order from 0.0f, then one multiply by scale; zero for pad_id and for absent tokens."""
    d = dx.numpy().astype(np.float32)
    t = tok.numpy()
    out = np.zeros((V, d.shape[1]), np.float32)
    sc = np.float32(scale)
    for v in range(V):
        if v == pad_id:
            continue
        acc = np.zeros(d.shape[1], np.float32)
        for r in np.nonzero(t == v)[0]:
            acc = acc + d[r]
        out[v] = acc * sc
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------------------------------------------------
# dropout masks: Philox4x32-10 restated from csrc/train_kernels.hip in integer arithmetic
# ---------------------------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1, _LO = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counter words c0..c3 (arrays or ints), key words k0, k1 -> the four output words, uint32 values held in uint64 arrays"""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _LO for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & _LO, np.uint64(k1) & _LO
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def dropout_threshold(p):
    """(unsigned)(p * 65536.0f + 0.5f) in float arithmetic"""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def dropout_draws(n, seed, stream_id):
    """the 16-bit draw of every element: counter = (group lo, group hi, stream lo, stream hi), key = (seed lo, seed hi), group =
    element / 8; eight draws per call in the order r[0] low, r[0] high, r[1] low, ..."""
    g = np.arange((n + 7) // 8, dtype=np.uint64)
    r = philox4x32_10(g & _LO, g >> _S32, stream_id & 0xFFFFFFFF, stream_id >> 32, seed & 0xFFFFFFFF, seed >> 32)
    d = np.empty((g.size, 8), np.uint64)
    for k in range(8):
        d[:, k] = (r[k >> 1] >> np.uint64(16 * (k & 1))) & np.uint64(0xFFFF)
    return d.reshape(-1)[:n].astype(np.int64)


def dropout_mask_ref(n, p, seed, stream_id):
    """keep mask as uint8: element i is kept when its draw >= the threshold"""
    return torch.from_numpy((dropout_draws(n, seed, stream_id) >= dropout_threshold(p)).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# the learned position table resized to a crop's patch grid (seq_modeling/vit_encoder.py:58-95): ATen's upsample_bicubic2d
# ---------------------------------------------------------------------------------------------------------------------
def pos_scales(GH, GW, gh, gw):
    """scale_h, scale_w as csrc/ctx.h pos_grid hands them to the kernels: the float of 1 / ((g + 0.1) / G) in double"""
    return float(np.float32(1.0 / ((gh + 0.1) / GH))), float(np.float32(1.0 / ((gw + 0.1) / GW)))


def source_coords(scale, n_out):
    """float64 source coordinate of every destination cell: scale * (dst + 0.5) - 0.5"""
    return scale * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5


def tap_matrix(scale, n_out, n_in, dtype):
    """[n_out][n_in]: the cubic-convolution weights (A = -0.75) of every destination cell on the source cells, taps clamped to
    the table (clamped taps add up on the edge cell), evaluated in `dtype`"""
    A = -0.75
    real = (torch.tensor(scale, dtype=dtype) * (torch.arange(n_out, dtype=dtype) + 0.5) - 0.5)
    i0 = torch.clamp(torch.floor(real).long(), max=n_in - 1)
    t = torch.clamp(real - i0.to(dtype), 0.0, 1.0)
    x0, x1, x2 = t + 1.0, t, 1.0 - t
    x3 = x2 + 1.0
    w = torch.stack([((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A, ((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0,
                     ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0, ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A], 1)
    M = torch.zeros(n_out, n_in, dtype=dtype)
    for k in range(4):
        M.scatter_add_(1, torch.clamp(i0 - 1 + k, 0, n_in - 1)[:, None], w[:, k:k + 1])
    return M


def bicubic_table_ref(src, GH, GW, gh, gw, sh, sw, order="x_first"):
    """src [GH*GW][D] -> [gh*gw][D] as a dense tap-matrix product in src's dtype; order: which axis is contracted first"""
    D = src.shape[1]
    Wy, Wx = tap_matrix(sh, gh, GH, src.dtype), tap_matrix(sw, gw, GW, src.dtype)
    s = src.reshape(GH, GW, D)
    if order == "x_first":
        out = torch.einsum("oy,ypd->opd", Wy, torch.einsum("px,yxd->ypd", Wx, s))
    else:
        out = torch.einsum("px,oxd->opd", Wx, torch.einsum("oy,yxd->oxd", Wy, s))
    return out.reshape(gh * gw, D)


def bicubic_table_aten(src, GH, GW, gh, gw, scale_factor=None):
    """the same through F.interpolate, the call of the reference (scale factors (gh + 0.1) / GH, (gw + 0.1) / GW)"""
    D = src.shape[1]
    sf = scale_factor or ((gh + 0.1) / GH, (gw + 0.1) / GW)
    out = F.interpolate(src.reshape(1, GH, GW, D).permute(0, 3, 1, 2), scale_factor=sf, mode="bicubic", align_corners=False)
    assert out.shape[-2:] == (gh, gw)
    return out.permute(0, 2, 3, 1).reshape(gh * gw, D)


def bicubic_e32(src, g, GH, GW, gh, gw, sh, sw):
    """(y64, e32 forward, d64, e32 transpose): float64 = the dense product with the kernels' float scales; fp32 evaluations =
    F.interpolate and the dense product in both association orders; the transpose is autograd of each forward on g"""
    def run(fn, dt):
        s = src.to(dt).clone().requires_grad_(True)
        y = fn(s)
        y.backward(g.to(dt))
        return y.detach(), s.grad
    y64, d64 = run(lambda s: bicubic_table_ref(s, GH, GW, gh, gw, sh, sw), torch.float64)
    ey = ed = 0.0
    for fn in (lambda s: bicubic_table_aten(s, GH, GW, gh, gw),
               lambda s: bicubic_table_ref(s, GH, GW, gh, gw, sh, sw, "x_first"),
               lambda s: bicubic_table_ref(s, GH, GW, gh, gw, sh, sw, "y_first")):
        y, d = run(fn, torch.float32)
        ey, ed = max(ey, float((y.double() - y64).abs().max())), max(ed, float((d.double() - d64).abs().max()))
    return y64, ey, d64, ed


# ---------------------------------------------------------------------------------------------------------------------
# the rest
# ---------------------------------------------------------------------------------------------------------------------
def mean_h_ref(x, mode="plain"):
    """x [B][H][W][C] -> [B][W][C]"""
    return rsum(mode, x, 1) / x.shape[1]


def sum_over_batch_ref(x, stride, n, mode="plain"):
    """x [B * stride] -> out[i] = sum_b x[b * stride + i], i < n"""
    return rsum(mode, x.reshape(-1, stride)[:, :n], 0)


def sum_rows_strided_ref(x, stride_rows, row, mode="plain"):
    """x [B * stride_rows][D] -> sum_b x[b * stride_rows + row]"""
    return rsum(mode, x.reshape(-1, stride_rows, x.shape[-1])[:, row], 0)


def token_rows_ref(src, B, n, skip, scatter):
    """gather: [B][n + skip][D] -> [B][n][D] (rows skip ...); scatter: the inverse with zero skip rows"""
    D = src.shape[-1]
    if not scatter:
        return src.reshape(B, n + skip, D)[:, skip:].reshape(B * n, D).clone()
    out = torch.zeros(B, n + skip, D, dtype=src.dtype)
    out[:, skip:] = src.reshape(B, n, D)
    return out.reshape(B * (n + skip), D)


def ew_ref(x, dy, op):
    """GELU (op 0, the exact erf form of nn.GELU) or ReLU (op 1): (y, dx) by autograd in x's dtype"""
    x = x.detach().clone().requires_grad_(True)
    y = F.gelu(x) if op == 0 else F.relu(x)
    y.backward(dy.to(x.dtype))
    return y.detach(), x.grad
