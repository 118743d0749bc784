"""Float64 restatement of what doc2tex_amd.optim's kernels compute (include/d2t.h, "fused optimizer step"): the global
gradient norm, clip_grad_norm_'s coefficient and one Adam / AdamW step, written from the formulas -- not from torch's code.
tests/test_optim_cpu.py holds it against torch.optim in float64 before any GPU test relies on it."""
import math

import torch


def grad_norm(grads):
    """sqrt(sum g^2) over every tensor, in float64."""
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


def clip_coef(norm, max_norm):
    """clip_grad_norm_: min(1, max_norm / (norm + 1e-6)); max_norm None or <= 0 = no clipping."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def adam_step(p, g, m, v, step, lr, betas, eps, weight_decay, decoupled, coef=1.0):
    """Step number `step` (1-based, after the increment) of Adam (decoupled False) or AdamW (True) on float64 copies (on the
    tensors' own device): returns the new (p, m, v)."""
    p, g, m, v = (t.detach().double().clone() for t in (p, g, m, v))
    b1, b2 = betas
    g = g * coef
    if decoupled:
        p = p * (1.0 - lr * weight_decay)
    else:
        g = g + weight_decay * p
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def ulp32(x):
    """One float32 unit in the last place at magnitude x (a positive float)."""
    x = abs(float(x))
    if x == 0.0 or not math.isfinite(x):
        return 2.0 ** -149
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23)


def within_yardstick(got, ref_got, yard, ref_yard):
    """The bound of the update tests: the largest absolute error of `got` against its float64 reference may be at most twice
    the yardstick's own (`yard`: torch's fp32 step, against ITS float64 reference -- the two differ only in whose reported
    norm formed the clip coefficient) plus one fp32 ulp of the tensor's largest magnitude.  Returns
    (ok, error of got, error of the yardstick, allowed)."""
    if ref_got.numel() == 0:
        return True, 0.0, 0.0, 0.0
    e_got = float((got.detach().to(ref_got.device).double() - ref_got).abs().max())
    e_yard = float((yard.detach().to(ref_yard.device).double() - ref_yard).abs().max())
    allowed = 2.0 * e_yard + ulp32(float(ref_got.abs().max()))
    return e_got <= allowed, e_got, e_yard, allowed
