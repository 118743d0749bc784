"""GPU: the cross-attention map kernel of the TFM decode alone (d2t_op_cross_attn_probs -> cross_attn_probs_kernel,
csrc/decode_maps.hip) against a float64 evaluation of softmax(q . K^T / sqrt(hd)) on seeded inputs.

Rule: the measured rule of tests/test_decode_ops_gpu.py -- e32 = max |p32 - p64| of a plain fp32 CPU evaluation of the same
inputs; the kernel gets max |p - p64| <= 8 e32 + 1e-6 max |p64|.
Key counts: 1, around the 16-key tile the decode's own kernels walk (15, 16, 17), the C2 memory (261), the longest memory
(4096), and one past every stride the kernel has: a wave's key loop is unrolled four times over 64 / (hd / 4) keys (32 keys
at hd 32, 16 at hd 64 -> 33 covers both), a wave's softmax passes stride by 64 lanes (65), the head mean by the block's 512
threads (513).  Row counts 1, 2, 3: one block per row, so an odd count has no partner row to repeat.
"""
import functools

import numpy as np
import pytest
import torch

from doc2tex_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = 1  # include/d2t.h D2T_EINVAL
H = 8
GUARD = 1024  # floats in front of and behind the output that must keep their pattern
SENTINEL = -12345.0
# (D, T, M)
SHAPES = [(D, T, 3) for D in (256, 512) for T in (1, 15, 16, 17, 33, 65, 261, 513, 4096)] + \
         [(D, 17, M) for D in (256, 512) for M in (1, 2)]


def _fig(name, **kv):
    print("FIG " + name + " " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _softmax_refs(q, k):
    """(p64, p32) [M, H, T] of q [M, D], k [M, H, T, hd] on the CPU."""
    M, D = q.shape
    hd = D // H

    def ev(dt):
        s = torch.einsum("mhe,mhte->mht", q.to(dt).reshape(M, H, hd), k.to(dt)) / (hd ** 0.5)
        return torch.softmax(s, dim=-1)
    return ev(torch.float64), ev(torch.float32)


@functools.lru_cache(maxsize=None)
def _case(D, T, M):
    """Seeded inputs and their references, computed once and shared (never written to)."""
    g = torch.Generator().manual_seed(7000 + D + 13 * T + M)
    q = torch.randn(M, D, generator=g) * 1.5
    k = torch.randn(M, H, T, D // H, generator=g) * 1.5
    return (q, k) + _softmax_refs(q, k)


def _run(q, k, per_head):
    """The operator on the GPU -> (out [M, H, T] or [M, T] on the CPU, the guard floats in front, behind)."""
    lib = _lib.require_device()
    M, D = q.shape
    T = k.shape[2]
    n = M * (H if per_head else 1) * T
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + n]
    qd, kd = q.contiguous().to(DEV), k.contiguous().to(DEV)
    rc = lib.d2t_op_cross_attn_probs(_lib.ptr(qd), _lib.ptr(kd), M, D, T, int(per_head), _lib.ptr(out), _lib.stream_of(qd))
    assert rc == 0, f"d2t_op_cross_attn_probs: rc {rc}"
    torch.cuda.synchronize()
    host = buf.cpu()
    shape = (M, H, T) if per_head else (M, T)
    return host[GUARD:GUARD + n].reshape(shape), host[:GUARD], host[GUARD + n:]


def _measured(name, p, p64, p32, **kv):
    assert torch.isfinite(p).all(), f"{name}: non-finite / unwritten elements"
    e32 = float((p32.double() - p64).abs().max())
    err = float((p.double() - p64).abs().max())
    mx = float(p64.abs().max())
    _fig(name, e32=e32, err=err, ratio=err / e32 if e32 > 0 else 0.0, max=mx, **kv)
    assert err <= 8 * e32 + 1e-6 * mx, f"{name}: |p - p64| = {err:.3e}, e32 = {e32:.3e}, max |p64| = {mx:.3e}"


def _in_order_mean(ph):
    """mean over the heads of ph [M, H, T] (fp32), summed in head order 0 .. 7 as torch's average_attn_weights does"""
    s = ph[:, 0].clone()
    for h in range(1, H):
        s = s + ph[:, h]
    return s * 0.125


@pytest.mark.parametrize("D,T,M", SHAPES)
def test_probs_vs_float64(D, T, M):
    q, k, p64, p32 = _case(D, T, M)
    ph, front, back = _run(q, k, True)
    assert (front == SENTINEL).all() and (back == SENTINEL).all(), "per-head form wrote outside its output"
    _measured(f"cross_probs_heads_D{D}_T{T}_M{M}", ph, p64, p32, D=D, T=T, M=M)
    rs = float((ph.double().sum(-1) - 1).abs().max())
    assert rs <= 1e-5, f"row sums off by {rs:.3e}"
    pm, front, back = _run(q, k, False)
    assert (front == SENTINEL).all() and (back == SENTINEL).all(), "mean form wrote outside its output"
    _measured(f"cross_probs_mean_D{D}_T{T}_M{M}", pm, p64.mean(1), p32.mean(1), D=D, T=T, M=M)
    assert float((pm.double().sum(-1) - 1).abs().max()) <= 1e-5
    # the mean is the in-order mean of the per-head output, within 1 ulp per head
    want = _in_order_mean(ph)
    ulp = torch.from_numpy(np.spacing(want.numpy()))
    assert bool(((pm - want).abs() <= H * ulp).all()), float((pm - want).abs().max())
    # ... and, the kernel adding the very eight floats it writes per head, in that order and each add rounded once, bit for bit
    # (what tells heads summed in another order apart: a difference of an ulp or two that no tolerance sees)
    assert torch.equal(pm, want)


@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("offset", [0.0, 120.0])
def test_wide_scores_stay_finite(D, offset):
    """Scores spread over +-80 (and the same spread around 120, where exp() of a raw score overflows fp32): the maximum is
    taken before any exponential, so every probability is finite and the measured rule holds."""
    M, T, hd = 2, 261, D // H
    g = torch.Generator().manual_seed(7100 + D)
    q = torch.randn(M, D, generator=g)
    qh = q.reshape(M, H, hd)
    # row 0: the scores in ascending order, so that the first keys (a tile, a chunk, a lane's first trips) hold the LOWEST scores
    # and a maximum taken over them alone is 140 below the true one (exp overflows); row 1: shuffled
    lin = torch.linspace(-80, 80, T)
    c = torch.stack([lin if i < H else lin[torch.randperm(T, generator=g)] for i in range(M * H)]).reshape(M, H, T) + offset
    # k_j = c_j sqrt(hd) q_h / |q_h|^2 (+ a little noise): score_j = c_j
    k = c[..., None] * (hd ** 0.5) * (qh / qh.pow(2).sum(-1, keepdim=True))[:, :, None, :] + 0.01 * torch.randn(M, H, T, hd, generator=g)
    p64, p32 = _softmax_refs(q, k)
    s64 = torch.einsum("mhe,mhte->mht", qh.double(), k.double()) / (hd ** 0.5)
    assert float(s64.max() - s64.min()) >= 150 and float(s64.max()) >= 79 + offset
    for per_head in (True, False):
        p, _, _ = _run(q, k, per_head)
        ref64, ref32 = (p64, p32) if per_head else (p64.mean(1), p32.mean(1))
        _measured(f"cross_probs_wide_D{D}_off{int(offset)}_{'heads' if per_head else 'mean'}", p, ref64, ref32, D=D)
        assert float((p.double().sum(-1) - 1).abs().max()) <= 1e-5


def test_refusals():
    lib = _lib.require_device()
    q = torch.zeros(1, 256, device=DEV)
    k = torch.zeros(1, H, 4, 32, device=DEV)
    out = torch.zeros(1, H, 4, device=DEV)
    s = _lib.stream_of(q)

    def call(M=1, D=256, T=4, q=q, k=k, out=out):
        return lib.d2t_op_cross_attn_probs(_lib.ptr(q), _lib.ptr(k), M, D, T, 1, _lib.ptr(out), s)
    assert call(T=0) == EINVAL and call(T=4097) == EINVAL and call(D=384) == EINVAL and call(M=0) == EINVAL
    assert call(q=None) == EINVAL and call(k=None) == EINVAL and call(out=None) == EINVAL
    assert call() == 0
