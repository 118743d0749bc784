"""Restatements of the encoder's record path (csrc/conv_common.h, conv_records.hip, ops.hip, engine_weights.hip) in plain
numpy / torch on the CPU, written from what the headers DOCUMENT, not from what the device returns: the three record formats
bit by bit, the plane layout, the row orders and remaps of the convolution epilogues, the kernels' K order and the BatchNorm
fold in float64.  Shared by tests/test_conv_records_gpu.py and tests/test_conv_record_refs_cpu.py, which pins every function
here to an independent torch operation.

Record formats (conv_common.h REC_*): 0 = bf16 hi | lo, 1 = ONE fp16 in the hi half (lo = 0), 2 = fp16 hi | fp16 lo.
"""
import numpy as np
import torch
import torch.nn.functional as F

REC_BF16, REC_F16, REC_F16_PAIR = 0, 1, 2
F16_MAX = 65504.0


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def bits_of(x):
    return _f32(x).view(np.uint32)


def bf16_bits_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f16_bits_to_f32(b):
    return np.ascontiguousarray(np.asarray(b, dtype=np.uint16)).view(np.float16).astype(np.float32)


def bf16_rne_bits(x):
    """fp32 -> bf16, round to nearest even, on the bits: add 0x7FFF plus the bit that will become the last one kept.  NaN
    stays a (quiet) NaN."""
    u = bits_of(x).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(_f32(x))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def f16_sat_bits(x):
    """conv_common.h f32_to_f16_bits: FINITE values saturate at +-65504, then round to nearest even; NaN and +-Inf pass"""
    x = _f32(x)
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.where(np.isfinite(x), np.clip(x, -F16_MAX, F16_MAX), x).astype(np.float32)
        return c.astype(np.float16).view(np.uint16)


def split_act(x, fmt):
    """One activation value -> (hi, lo) uint16 of a record.
    0: hi = the TRUNCATED upper 16 bits of the fp32, lo = RNE bf16 of the remainder x - hi (exact in fp32);
    1: hi = saturating fp16, lo = 0;  2: hi = saturating fp16, lo = saturating fp16 of the remainder x - hi (exact in fp32).
    A non-finite x leaves a NaN remainder (Inf - Inf) in the lo half of formats 0 and 2."""
    x = _f32(x)
    with np.errstate(invalid="ignore", over="ignore"):
        if fmt == REC_BF16:
            u = bits_of(x)
            hi = (u >> 16).astype(np.uint16)
            rem = x - (u & np.uint32(0xFFFF0000)).view(np.float32)
            return hi, bf16_rne_bits(rem)
        hi = f16_sat_bits(x)
        if fmt == REC_F16:
            return hi, np.zeros_like(hi)
        return hi, f16_sat_bits(x - f16_bits_to_f32(hi))


def join_act(hi, lo, fmt):
    """(hi, lo) -> fp32: hi + lo in fp32 (formats 0, 2), or the fp16 hi alone (format 1: the lo half is not read)"""
    with np.errstate(invalid="ignore", over="ignore"):
        if fmt == REC_BF16:
            return bf16_bits_to_f32(hi) + bf16_bits_to_f32(lo)
        if fmt == REC_F16:
            return f16_bits_to_f32(hi)
        return f16_bits_to_f32(hi) + f16_bits_to_f32(lo)


def mma_operand(hi, lo, fmt):
    """what the convolution's MFMAs multiply: float64 of hi + lo for bf16 records, of the hi half ALONE for fp16 records"""
    if fmt == REC_BF16:
        return bf16_bits_to_f32(hi).astype(np.float64) + bf16_bits_to_f32(lo).astype(np.float64)
    return f16_bits_to_f32(hi).astype(np.float64)


def split_weight_bf16(w):
    """weight planes (launch_split_bf16): hi = RNE bf16 of w, lo = RNE bf16 of w - hi"""
    w = _f32(w)
    hi = bf16_rne_bits(w)
    with np.errstate(invalid="ignore"):
        return hi, bf16_rne_bits(w - bf16_bits_to_f32(hi))


def split_weight_f16(w):
    """weight planes (launch_split_f16): hi = saturating fp16 of w, lo = saturating fp16 of w - hi"""
    w = _f32(w)
    hi = f16_sat_bits(w)
    with np.errstate(invalid="ignore"):
        return hi, f16_sat_bits(w - f16_bits_to_f32(hi))


def same_bits(a, b, kind):
    """a == b as uint16 halves of `kind` ("bf16" | "f16"), any NaN equal to any NaN (a NaN's sign and payload are not part of
    the contract)"""
    a, b = np.asarray(a, dtype=np.uint16), np.asarray(b, dtype=np.uint16)
    to = bf16_bits_to_f32 if kind == "bf16" else f16_bits_to_f32
    na, nb = np.isnan(to(a)), np.isnan(to(b))
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def edge_values():
    """+-0, fp16 subnormals, the fp16 range's end, non-finite values, values within 2^-9 of a bf16 step (the truncated hi
    leaves a remainder next to a whole step, which RNE may round UP to it), and exact RNE ties of both 16-bit formats"""
    v = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15, 1023 * 2.0 ** -24, 2.0 ** -14,
         65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 1e5, -1e5, 3e38, float("inf"), float("-inf"), float("nan")]
    for base in (1.0, -1.0, 300.0, 1e-3):
        step = float(np.spacing(np.float32(abs(base)))) * 65536  # one bf16 (8-bit mantissa) step at this magnitude
        for f in (1 - 2.0 ** -9, 1 - 2.0 ** -10, 1 - 2.0 ** -16, 0.5, 0.5 + 2.0 ** -9, 0.5 - 2.0 ** -9, 1.5, 2.0 ** -9):
            v.append(base + np.sign(base) * step * f)
    # ties: halfway between two bf16 values (bit 15 set, nothing below), even and odd last kept bit
    for u in (0x3F808000, 0x3F818000, 0xBF808000, 0x3F80FFFF, 0x3F808001, 0x7F7F8000):
        v.append(float(np.array([u], dtype=np.uint32).view(np.float32)[0]))
    # ties of fp16 (10-bit mantissa): 1 + 2^-11, 1 + 3 * 2^-11, and just beside them
    v += [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -11 - 2.0 ** -20, 2049.0, 2051.0]
    return np.array(v, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
def plane_idx(row, c, C):
    """conv_common.h plane_idx: index (uint16 units) of the hi half of element (row, c); the lo half lies 32 further"""
    return (row * C + (c & ~31)) * 2 + (c & 31)


def to_planes(hi, lo):
    """hi, lo [rows][C] -> raw planes, flat uint16 [rows * C * 2]: per row and 32-channel group [32 x hi | 32 x lo]"""
    rows, C = hi.shape
    out = np.zeros(rows * C * 2, dtype=np.uint16)
    r, c = np.meshgrid(np.arange(rows), np.arange(C), indexing="ij")
    i = plane_idx(r, c, C)
    out[i] = hi
    out[i + 32] = lo
    return out


def from_planes(planes, rows, C):
    r, c = np.meshgrid(np.arange(rows), np.arange(C), indexing="ij")
    i = plane_idx(r, c, C)
    planes = np.asarray(planes).reshape(-1)
    return planes[i], planes[i + 32]


def records_of(x, fmt):
    """fp32 [rows][C] -> raw planes"""
    return to_planes(*split_act(x, fmt))


def values_of(planes, rows, C, fmt):
    """raw planes -> fp32 [rows][C]"""
    return join_act(*from_planes(planes, rows, C), fmt)


def pooled_row_pixel(B, OH, OW):
    """ConvP::pool2: GEMM row m -> flat output pixel (b * OH + oh) * OW + ow, m = 4 * pooled pixel + (oh & 1) * 2 + (ow & 1),
    M = 4 * B * (OH // 2) * (OW // 2) (a last odd row / column belongs to no window)"""
    ph2, pw2 = OH // 2, OW // 2
    m = np.arange(4 * B * ph2 * pw2)
    q, sb = m >> 2, m & 3
    t = q // pw2
    ow = 2 * (q - t * pw2) + (sb & 1)
    b = t // ph2
    oh = 2 * (t - b * ph2) + (sb >> 1)
    return (b * OH + oh) * OW + ow


def remap_rows(M, rows_per_img, img_stride, row_off):
    """output row of GEMM row m: (m // rows_per_img) * img_stride + row_off + m % rows_per_img; rows_per_img == 0: m"""
    m = np.arange(M)
    if rows_per_img == 0:
        return m
    return (m // rows_per_img) * img_stride + row_off + m % rows_per_img


def row_add_rows(M, rows_per_img, row_add_off):
    """table row added to GEMM row m: row_add_off + m % rows_per_img (row_add_off alone without a remap)"""
    m = np.arange(M)
    return row_add_off + (m % rows_per_img if rows_per_img else 0 * m)


def kv_index(kv_B, kv_T, heads, hd, N):
    """STORE_KV: flat output index of element (m, n) of the plain rows [M = kv_B * kv_T][N]:
    out[(((slab * kv_B + b) * heads + head) * kv_T + j) * hd + e], n = (slab * heads + head) * hd + e, m = b * kv_T + j"""
    m, n = np.meshgrid(np.arange(kv_B * kv_T), np.arange(N), indexing="ij")
    d = heads * hd
    slab, within = n // d, n % d
    head, e = within // hd, within % hd
    b, j = m // kv_T, m % kv_T
    return (((slab * kv_B + b) * heads + head) * kv_T + j) * hd + e


def k_order(Cin, KH, KW):
    """position k of a packed weight row -> index into the row's OHWI order (kh, kw, c).  Cin % 32 == 0: 32-channel chunk, tap,
    channel in chunk; otherwise the plain OHWI order."""
    if Cin % 32:
        return np.arange(KH * KW * Cin)
    chunk, tap, ci = np.meshgrid(np.arange(Cin // 32), np.arange(KH * KW), np.arange(32), indexing="ij")
    return (tap * Cin + chunk * 32 + ci).reshape(-1)


def pack_rows(w_oihw):
    """[Cout][Cin][KH][KW] -> [Cout][K] in the kernels' K order (a second input's rows follow: np.concatenate along K)"""
    w = np.asarray(w_oihw)
    Cout, Cin, KH, KW = w.shape
    ohwi = w.transpose(0, 2, 3, 1).reshape(Cout, -1)
    return ohwi[:, k_order(Cin, KH, KW)]


def bn_fold(w_oihw, conv_bias, bn, eps):
    """eval BatchNorm folded into a convolution, float64: s = gamma / sqrt(var + eps), w' = w * s, b' = conv_bias * s +
    beta - mean * s (each part only where given).  bn = (gamma, beta, mean, var) or None.  -> (w' OIHW, b')"""
    w = np.asarray(w_oihw, dtype=np.float64)
    s = np.ones(w.shape[0])
    b = np.zeros(w.shape[0])
    if bn is not None:
        g, be, mu, var = (np.asarray(t, dtype=np.float64) for t in bn)
        s = g / np.sqrt(var + np.float64(np.float32(eps)))
    if conv_bias is not None:
        b = b + np.asarray(conv_bias, dtype=np.float64) * s
    if bn is not None:
        b = b + be - mu * s
    return w * s[:, None, None, None], b


# ---------------------------------------------------------------------------------------------------------------------
# the convolution in float64
# ---------------------------------------------------------------------------------------------------------------------
def conv_ref(x_rows, B, H, W, w_oihw, bias, stride, pad, OH=None, OW=None):
    """x_rows float64 [B*H*W][Cin] (NHWC rows) -> float64 [B*OH*OW][Cout]; an overridden OH x OW grid reads zeros beyond the
    bottom / right edge (the patch embedding)"""
    x = torch.as_tensor(np.asarray(x_rows, dtype=np.float64)).reshape(B, H, W, -1).permute(0, 3, 1, 2)
    w = torch.as_tensor(np.asarray(w_oihw, dtype=np.float64))
    KH, KW = w.shape[2:]
    if OH is not None:
        need_h, need_w = (OH - 1) * stride[0] + KH - 2 * pad[0], (OW - 1) * stride[1] + KW - 2 * pad[1]
        x = F.pad(x, (0, max(0, need_w - W), 0, max(0, need_h - H)))
    y = F.conv2d(x, w, None if bias is None else torch.as_tensor(np.asarray(bias, dtype=np.float64)), stride, pad)
    if OH is not None:
        y = y[:, :, :OH, :OW]
    y = y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])
    return y.numpy()


def finish_ref(y, act, res=None):
    """residual, then the activation (0 none, 1 ReLU), float64"""
    if res is not None:
        y = y + res
    return np.maximum(y, 0.0) if act == 1 else y
