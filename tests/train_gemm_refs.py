"""References of the weight-gradient, BatchNorm, LayerNorm, stem and data-movement kernels of the training step
(csrc/train_wgrad.hip, train_kernels.hip), written from each operation's definition at the KERNELS' layouts: row-major
[rows][channels] matrices, NHWC maps, per-chunk partials part[z][tap][m][n].  Plain torch on the CPU at any dtype: float64 is
the reference and the same functions at float32 give e32 (`mode` as in tests/recurrent_refs.py: torch's own reductions, every
reduction reversed, every reduction in 16 chunks).  Shared by tests/test_train_gemm_ops_gpu.py and
tests/test_train_gemm_refs_cpu.py, which pins every function here to torch.autograd on F.conv2d / F.batch_norm /
F.layer_norm / F.linear.

The bit-exact references (the two orders of the sum over chunks, the operand split of wgrad_bf16x3_kernel) are numpy.
"""
import numpy as np
import torch

import conv_record_refs as CR
from recurrent_refs import MODES, e32_of, mm, rsum  # noqa: F401  (re-exported)

# the four convolution geometries of the network: (KH, KW, SH, SW, PH, PW)
GEOMS = {"3x3p1": (3, 3, 1, 1, 1, 1), "2x2s21p01": (2, 2, 2, 1, 0, 1), "2x2s2": (2, 2, 2, 2, 0, 0), "1x1": (1, 1, 1, 1, 0, 0)}


def out_size(H, W, geom):
    KH, KW, SH, SW, PH, PW = geom
    return (H + 2 * PH - KH) // SH + 1, (W + 2 * PW - KW) // SW + 1


# ---------------------------------------------------------------------------------------------------------------------
# operand splits
# ---------------------------------------------------------------------------------------------------------------------
def split4_bf16(x):
    """wgrad_bf16x3_kernel's split of an fp32 operand, in integer arithmetic: hi = the upper 16 bits (truncation), lo = bf16
    round-to-nearest-even of x - hi (that difference is exact in fp32).  Returns (hi, lo) as fp32 VALUES (numpy)."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    u = x.view(np.uint32)
    hi = (u & np.uint32(0xFFFF0000)).view(np.float32)
    r = (x - hi).astype(np.float32).view(np.uint32).astype(np.uint64)
    lo = (((r + 0x7FFF + ((r >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return hi, lo


def split_records(x):
    """the record split (tests/conv_record_refs.py split_act, format 0) as fp32 values"""
    hi, lo = CR.split_act(np.asarray(x, dtype=np.float32), CR.REC_BF16)
    return CR.bf16_bits_to_f32(hi), CR.bf16_bits_to_f32(lo)


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def src_rows(B, H, W, geom):
    """[taps][P] int64: the row of the NHWC input that output pixel p reads under tap kh * KW + kw; -1 = padding"""
    KH, KW, SH, SW, PH, PW = geom
    OH, OW = out_size(H, W, geom)
    b, oh, ow = torch.meshgrid(torch.arange(B), torch.arange(OH), torch.arange(OW), indexing="ij")
    out = []
    for kh in range(KH):
        for kw in range(KW):
            ih, iw = oh * SH - PH + kh, ow * SW - PW + kw
            ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
            out.append(torch.where(ok, (b * H + ih) * W + iw, torch.full_like(ih, -1)).reshape(-1))
    return torch.stack(out)


def wgrad_ref(a, b, M, N, S, chunk, src=None, mode="plain"):
    """part[z][tap][m][n] = sum_{p in chunk z} a[p][m] * b[src[tap][p]][n];  a [P][lda], b [rows][ldb] (the first M / N columns
    count), src None = one tap reading row p"""
    P = a.shape[0]
    a, b = a[:, :M], b[:, :N]
    taps = 1 if src is None else src.shape[0]
    part = torch.zeros(S, taps, M, N, dtype=a.dtype)
    for t in range(taps):
        if src is None:
            bt = b
        else:
            bt = b[src[t].clamp(min=0)] * (src[t] >= 0).to(a.dtype)[:, None]
        for z in range(S):
            lo, hi = z * chunk, min((z + 1) * chunk, P)
            if hi > lo:
                part[z, t] = mm(mode, a[lo:hi].t().contiguous(), bt[lo:hi].contiguous())
    return part


def wgrad_split_ref(a_hl, b_hl, M, N, S, chunk, src=None, mode="plain"):
    """the three products of split-bf16 arithmetic, lo*hi + hi*lo + hi*hi, each as wgrad_ref and summed in that order"""
    (ah, al), (bh, bl) = a_hl, b_hl
    f = lambda x, y: wgrad_ref(x, y, M, N, S, chunk, src, mode)
    return f(al, bh) + f(ah, bl) + f(ah, bh)


def abs_product(a, b, M, N, S, chunk, src=None):
    """sum |a||b| per element of part, float64: the scale of the derived bounds"""
    return wgrad_ref(a.double().abs(), b.double().abs(), M, N, S, chunk, src)


def reduce_ref(part, layout, dst=None, mode="plain"):
    """sum over the chunks of part [S][taps][M][N] (+ dst);  layout 0: [M][N] (taps == 1), layout 1: OIHW [M][N][taps]"""
    v = rsum(mode, part, 0)
    v = v.permute(1, 2, 0).contiguous() if layout == 1 else v[0]
    return v if dst is None else dst + v


def _place(v, taps, M, N, layout, dst):
    v = v.reshape(taps, M, N)
    v = np.ascontiguousarray(v.transpose(1, 2, 0)) if layout == 1 else v[0]
    return v if dst is None else (np.asarray(dst, dtype=np.float32) + v).astype(np.float32)


def reduce_ordered_fp32(part, layout, dst=None):
    """the grid-stride kernel's documented order: fp32, z ascending from 0.0f; then dst + v"""
    part = np.asarray(part, dtype=np.float32)
    S, taps, M, N = part.shape
    v = np.zeros(taps * M * N, dtype=np.float32)
    for z in range(S):
        v = (v + part[z].reshape(-1)).astype(np.float32)
    return _place(v, taps, M, N, layout, dst)


def reduce_tree_fp32(part, layout, dst=None):
    """the one-block-per-output kernel's documented order: thread t of 256 adds partials t, t + 256, ... in ascending order
    from 0.0f, then the halving tree red[t] += red[t + o], o = 128, 64, ..., 1; then dst + red[0]"""
    part = np.asarray(part, dtype=np.float32)
    S, taps, M, N = part.shape
    flat = part.reshape(S, -1)
    red = np.zeros((256, flat.shape[1]), dtype=np.float32)
    for z in range(S):
        red[z % 256] = (red[z % 256] + flat[z]).astype(np.float32)
    o = 128
    while o:
        red[:o] = (red[:o] + red[o:2 * o]).astype(np.float32)
        o >>= 1
    return _place(red[0].copy(), taps, M, N, layout, dst)


# ---------------------------------------------------------------------------------------------------------------------
# column sums, BatchNorm, LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
CR_SUM, CR_SUM_SQ, CR_BN_BWD, CR_LN_BWD = 0, 1, 2, 3


def colsums_ref(cmode, a, y=None, z=None, mean=None, rstd=None, mode="plain"):
    """the two column sums of launch_colreduce's four modes over all rows: (s0 [C], s1 [C]).  CR_SUM_SQ: sum (a - a[0]) and
    sum (a - a[0])^2, from which mean = a[0] + s0 / R and var = s1 / R - (s0 / R)^2"""
    if cmode == CR_SUM:
        return rsum(mode, a, 0), torch.zeros(a.shape[1], dtype=a.dtype)
    if cmode == CR_SUM_SQ:  # about the channel's value in row 0
        d = a - a[0:1]
        return rsum(mode, d, 0), rsum(mode, d * d, 0)
    if cmode == CR_BN_BWD:
        g = a if y is None else a * (y > 0).to(a.dtype)
        return rsum(mode, g, 0), rsum(mode, g * ((z - mean[None, :]) * rstd[None, :]), 0)
    return rsum(mode, a, 0), rsum(mode, a * ((z - mean[:, None]) * rstd[:, None]), 0)


def bn_stats_ref(z, eps, momentum=None, run_mean=None, run_var=None, mode="plain"):
    """batch statistics of z [R][C]: mean, rstd = 1 / sqrt(biased variance + eps), and nn.BatchNorm2d's running update with the
    unbiased variance (the biased one where R == 1: the kernel's guard)"""
    R = z.shape[0]
    mean = rsum(mode, z, 0) / R
    var = rsum(mode, (z - mean[None, :]) ** 2, 0) / R
    out = dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps))
    if run_mean is not None:
        unb = var * R / (R - 1) if R > 1 else var
        out["run_mean"] = (1.0 - momentum) * run_mean + momentum * mean
        out["run_var"] = (1.0 - momentum) * run_var + momentum * unb
    return out


def bn_apply_ref(z, mean, rstd, gamma, beta, res=None, relu=False):
    t = (z - mean[None, :]) * rstd[None, :] * gamma[None, :] + beta[None, :]
    if res is not None:
        t = t + res
    return torch.clamp(t, min=0) if relu else t


def bn_bwd_ref(dy, y, z, mean, rstd, gamma, mode="plain"):
    """g = dy (y > 0 where y is given); s0 = sum g (d beta), s1 = sum g xhat (d gamma); dz = gamma rstd (g - s0 / R - xhat s1 / R)"""
    R = z.shape[0]
    g = dy if y is None else dy * (y > 0).to(dy.dtype)
    xh = (z - mean[None, :]) * rstd[None, :]
    s0, s1 = rsum(mode, g, 0), rsum(mode, g * xh, 0)
    dz = (gamma * rstd)[None, :] * (g - s0[None, :] / R - xh * s1[None, :] / R)
    return dict(g=g, s0=s0, s1=s1, dz=dz)


def bn_chain_ref(z, gamma, beta, res, relu, dy, eps, momentum, run_mean, run_var, mode="plain"):
    """finalize + apply + backward-apply on one set of operands, every stage on the previous stage's results"""
    st = bn_stats_ref(z, eps, momentum, run_mean, run_var, mode)
    y = bn_apply_ref(z, st["mean"], st["rstd"], gamma, beta, res, relu)
    bw = bn_bwd_ref(dy, y if relu else None, z, st["mean"], st["rstd"], gamma, mode)
    return dict(y=y, **st, **bw)


def ln_ref(x, gamma, beta, eps, mode="plain"):
    D = x.shape[1]
    mean = rsum(mode, x, 1) / D
    var = rsum(mode, (x - mean[:, None]) ** 2, 1) / D
    rstd = 1.0 / torch.sqrt(var + eps)
    return dict(y=(x - mean[:, None]) * rstd[:, None] * gamma[None, :] + beta[None, :], mean=mean, rstd=rstd)


def ln_bwd_ref(dy, x, mean, rstd, gamma, add=None, mode="plain"):
    D = x.shape[1]
    dg = dy * gamma[None, :]
    xh = (x - mean[:, None]) * rstd[:, None]
    a, b = rsum(mode, dg, 1) / D, rsum(mode, dg * xh, 1) / D
    dx = rstd[:, None] * (dg - a[:, None] - xh * b[:, None])
    return dx if add is None else dx + add


# ---------------------------------------------------------------------------------------------------------------------
# stem (3x3, pad 1 on an NCHW image), tap order (ci * 3 + kh) * 3 + kw
# ---------------------------------------------------------------------------------------------------------------------
def _stem_taps(img):
    """[9 Cin][B H W]: the image value every output pixel reads under each tap (zero in the padding)"""
    B, Cin, H, W = img.shape
    p = torch.zeros(B, Cin, H + 2, W + 2, dtype=img.dtype)
    p[:, :, 1:H + 1, 1:W + 1] = img
    return torch.stack([p[:, ci, kh:kh + H, kw:kw + W].reshape(-1) for ci in range(Cin) for kh in range(3) for kw in range(3)])


def stem_ref(img, w, mode="plain"):
    """z [B H W][Cout] = sum_tap image[tap][p] * w[co][tap]"""
    return mm(mode, _stem_taps(img).t().contiguous(), w.reshape(w.shape[0], -1).t().contiguous())


def stem_wgrad_ref(img, dz, chunk, mode="plain"):
    """part [nchunks][9 Cin][Cout] = sum_{p in chunk} image[tap][p] * dz[p][co]"""
    t = _stem_taps(img)
    P = dz.shape[0]
    n = (P + chunk - 1) // chunk
    return torch.stack([mm(mode, t[:, k * chunk:min((k + 1) * chunk, P)].contiguous(), dz[k * chunk:min((k + 1) * chunk, P)])
                        for k in range(n)])


# ---------------------------------------------------------------------------------------------------------------------
# movers
# ---------------------------------------------------------------------------------------------------------------------
def dilate_ref(src, DH, DW, SH, SW, offh, offw):
    """src [B][OH][OW][C] -> dst [B][DH][DW][C]: dst[b][oh SH + offh][ow SW + offw] = src[b][oh][ow] where inside, else 0"""
    B, OH, OW, C = src.shape
    dst = torch.zeros(B, DH, DW, C, dtype=src.dtype)
    for oh in range(OH):
        for ow in range(OW):
            h, w = oh * SH + offh, ow * SW + offw
            if h < DH and w < DW:
                dst[:, h, w] = src[:, oh, ow]
    return dst


def flip_oihw_ref(w):
    """[Cout][Cin][KH][KW] -> [Cin][Cout][KH][KW] with both filter axes reversed"""
    return w.flip(2).flip(3).permute(1, 0, 2, 3).contiguous()


def pad_cols_ref(src, Cd):
    out = torch.zeros(src.shape[0], Cd, dtype=src.dtype)
    out[:, :src.shape[1]] = src
    return out


def copy2d_ref(src, dst, cols):
    """src [rows][lds], dst [rows][ldd] (its other columns stay)"""
    out = dst.clone()
    out[:, :cols] = src[:, :cols]
    return out
