"""Restatements of what doc2tex_amd.optim's LAMB, AdamP, MADGRAD and Lookahead kernels compute (include/d2t.h, "the optimizer
family"), written from the formulas and parameterised by dtype: in float64 they are the reference of the GPU tests, in
float32 -- run eagerly on the device -- their yardstick.  tests/test_optim_family_cpu.py holds the float64 form against
fixtures recorded from the reference's own classes (tests/golden/optim_family.*, tools/make_golden_optim.py) before any GPU
test relies on it.  Scalars stay Python floats, as in the reference; every function works on copies."""
import math

import torch

FIXTURE_STEPS = 13  # lookahead_k = 6 synchronises twice


def _copies(dtype, *ts):
    return [None if t is None else t.detach().to(dtype).clone() for t in ts]


def lamb_divisor(norm, max_grad_norm):
    """LAMB's own clip: the gradients are divided by norm / max_grad_norm where the global norm exceeds it, else by 1."""
    return float(norm) / float(max_grad_norm) if float(norm) > float(max_grad_norm) else 1.0


def _lamb_parts(p, g, m, v, step, betas, eps, weight_decay, divisor, bias_correction, grad_averaging, always_adapt, dtype):
    """The new moments, the update direction u and the trust ratio before any clipping (None where the tensor does not
    adapt)."""
    p, g, m, v = _copies(dtype, p, g, m, v)
    b1, b2 = betas
    g = g / divisor
    m = b1 * m + (1.0 - b1 if grad_averaging else 1.0) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = (1.0 - b1 ** step, 1.0 - b2 ** step) if bias_correction else (1.0, 1.0)
    u = (m / bc1) / (v.sqrt() / math.sqrt(bc2) + eps)
    if weight_decay != 0:
        u = u + weight_decay * p
    trust = None
    if weight_decay != 0 or always_adapt:
        pn, un = p.norm(), u.norm()
        trust = pn / un if float(pn) > 0 and float(un) > 0 else torch.ones((), dtype=dtype, device=p.device)
    return p, m, v, u, trust


def lamb_trust_ratio(p, g, m, v, step, betas, eps, weight_decay, divisor=1.0, bias_correction=True, grad_averaging=True,
                     always_adapt=False):
    """|p| / |u| of the step in float64 before trust_clip (1 where either norm is 0), or None where the tensor does not adapt."""
    trust = _lamb_parts(p, g, m, v, step, betas, eps, weight_decay, divisor, bias_correction, grad_averaging, always_adapt,
                        torch.float64)[4]
    return None if trust is None else float(trust)


def lamb_step(p, g, m, v, step, lr, betas, eps, weight_decay, divisor=1.0, bias_correction=True, grad_averaging=True,
              trust_clip=False, always_adapt=False, dtype=torch.float64):
    """Step number `step` (1-based) of LAMB on one tensor: returns the new (p, m, v)."""
    p, m, v, u, trust = _lamb_parts(p, g, m, v, step, betas, eps, weight_decay, divisor, bias_correction, grad_averaging,
                                    always_adapt, dtype)
    if trust is not None:
        if trust_clip:
            trust = trust.clamp(max=1.0)
        u = u * trust
    return p - lr * u, m, v


def _abs_cos(x, y, eps):
    """|F.cosine_similarity(x, y, dim=1, eps)|: x.y / (max(|x|, eps) max(|y|, eps)) per row."""
    return ((x * y).sum(1) / (x.norm(dim=1).clamp_min(eps) * y.norm(dim=1).clamp_min(eps))).abs()


def adamp_decision(p, g, delta, eps):
    """(mode, margin) of AdamP's projection on float64 copies: 1 channel where the largest row |cos| of reshape(size(0), -1)
    is below delta / sqrt(row length), else 2 layer where the whole tensor's |cos| is below delta / sqrt(numel), else 0.
    margin = the smallest |cos - threshold| / threshold over the comparisons made (inf for one dimension)."""
    if p.dim() <= 1:
        return 0, math.inf
    p, g = _copies(torch.float64, p, g)
    margin = math.inf
    for mode, shape in ((1, (p.shape[0], -1)), (2, (1, -1))):
        pv, gv = p.reshape(shape), g.reshape(shape)
        threshold = delta / math.sqrt(pv.shape[1])
        c = float(_abs_cos(gv, pv, eps).max())
        margin = min(margin, abs(c - threshold) / threshold)
        if c < threshold:
            return mode, margin
    return 0, margin


def adamp_step(p, g, m, v, step, lr, betas, eps, weight_decay, delta=0.1, wd_ratio=0.1, nesterov=False, coef=1.0, mode=None,
               dtype=torch.float64):
    """Step number `step` of AdamP on one tensor: returns the new (p, m, v), the projection mode and its margin.  The mode
    is decided in float64 whatever `dtype` (or taken from `mode`): the yardstick follows the same branch as the reference."""
    p, g, m, v = _copies(dtype, p, g, m, v)
    b1, b2 = betas
    g = g * coef
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    perturb = (b1 * m + (1.0 - b1) * g) / denom if nesterov else m / denom
    decided, margin = adamp_decision(p, g, delta, eps)
    mode = decided if mode is None else mode
    ratio = 1.0
    if mode:
        shape = (p.shape[0], -1) if mode == 1 else (1, -1)
        pv = p.reshape(shape)
        p_n = pv / (pv.norm(dim=1, keepdim=True) + eps)
        perturb = (perturb.reshape(shape) - p_n * (p_n * perturb.reshape(shape)).sum(1, keepdim=True)).reshape(p.shape)
        ratio = wd_ratio
    if weight_decay > 0:
        p = p * (1.0 - lr * weight_decay * ratio)
    return p - (lr / (1.0 - b1 ** step)) * perturb, m, v, mode, margin


def madgrad_step(p, g, grad_sum_sq, s, x0, step, lr, momentum, eps, weight_decay, decoupled_decay=False, coef=1.0,
                 dtype=torch.float64):
    """Step number `step` of MADGRAD (dense) on one tensor: returns the new (p, grad_sum_sq, s); x0 (None where momentum is
    0) is never changed."""
    p, g, q, s, x0 = _copies(dtype, p, g, grad_sum_sq, s, x0)
    lamb = (lr + eps) * math.sqrt(step)
    g = g * coef
    if weight_decay != 0:
        if decoupled_decay:
            p = p * (1.0 - lr * weight_decay)
        else:
            g = g + weight_decay * p
    if momentum == 0:
        x0 = p + s / (q.pow(1 / 3) + eps)
    q = q + lamb * g * g
    s = s + lamb * g
    z = x0 - s / (q.pow(1 / 3) + eps)
    ck = 1.0 - momentum
    return (z if momentum == 0 else (1.0 - ck) * p + ck * z), q, s


def lookahead_sync(fast, slow, alpha, dtype=torch.float64):
    """slow + alpha (fast - slow): the new slow AND fast weights."""
    fast, slow = _copies(dtype, fast, slow)
    return slow + alpha * (fast - slow)


# ---- the seeded problem of the fixtures ----------------------------------------------------------------------------------
def _hash_values(n, salt):
    """n exactly representable values in [-1, 1], the same on every platform."""
    i = torch.arange(n, dtype=torch.int64)
    return ((i * 7919 + salt * 104729 + 12345) % 2003 - 1001).double() / 1001.0


def fixture_grad(kind, p, step, index):
    """The float64 gradient of tensor `index` at `step`, a function of its present value `p`:
      random   seeded values plus 0.3 p: far from orthogonal to p, by row and as a whole (no projection);
      channel  seeded values made orthogonal to p row by row (AdamP's channel mode at every step);
      layer    rows a_i p_i with sum a_i |p_i|^2 = 0: every row (anti)parallel to p, the whole tensor orthogonal (layer mode);
      zero     zeros."""
    r = _hash_values(p.numel(), 31 * step + index).reshape(p.shape)
    if kind == "random":
        return r + 0.3 * p.double()
    if kind == "zero":
        return torch.zeros_like(p)
    pv, rv = p.double().reshape(p.shape[0], -1), r.reshape(p.shape[0], -1)
    pp = (pv * pv).sum(1, keepdim=True)
    if kind == "channel":
        return (rv - pv * ((rv * pv).sum(1, keepdim=True) / pp.clamp_min(1e-300))).reshape(p.shape)
    if kind == "layer":
        b = _hash_values(p.shape[0], 17 * step + index + 5).reshape(-1, 1)
        a = b - (b * pp).sum() / pp.sum()
        return (a * pv).reshape(p.shape)
    raise ValueError(kind)


# (shape, gradient kind) of the fixture tensors; tensors [:FIXTURE_SPLIT] are group 0, the rest group 1
FIXTURE_TENSORS = [((5,), "random"), ((4, 6), "random"), ((3, 8), "channel"), ((1, 7), "random"), ((17,), "zero"),
                   ((4, 2, 3, 3), "layer"), ((6, 5), "random")]
FIXTURE_SPLIT = 4
FIXTURE_NO_GRAD = 3  # this tensor never has a gradient

# name -> (class, constructor arguments of the base, per-group overrides (group 0, group 1), lookahead or None)
FIXTURE_CASES = {
    "lamb_a": ("Lamb", dict(lr=2e-2, weight_decay=0.01, max_grad_norm=1.0), ({"weight_decay": 0.0}, {}), None),
    "lamb_b": ("Lamb", dict(lr=1e-2, betas=(0.8, 0.95), weight_decay=0.0, bias_correction=False, grad_averaging=False,
                            trust_clip=True, always_adapt=True, max_grad_norm=1e3), ({}, {"lr": 3e-2, "weight_decay": 0.1}), None),
    "adamp_a": ("AdamP", dict(lr=1e-2, weight_decay=0.05, wd_ratio=0.01, nesterov=True), ({}, {"lr": 2e-2}), None),
    "adamp_b": ("AdamP", dict(lr=1e-2, betas=(0.8, 0.95), weight_decay=0.0, nesterov=False), ({}, {}), None),
    "madgrad_a": ("MADGRAD", dict(lr=1e-2, momentum=0.9, weight_decay=0.01), ({}, {"lr": 2e-2}), None),
    "madgrad_b": ("MADGRAD", dict(lr=1e-2, momentum=0.0, weight_decay=0.01, decoupled_decay=True), ({}, {}), None),
    "madgrad_c": ("MADGRAD", dict(lr=1e-2, momentum=0.0, weight_decay=0.0), ({}, {"weight_decay": 0.02}), None),
    "lookahead_lamb": ("Lamb", dict(lr=2e-2, weight_decay=0.01), ({"weight_decay": 0.0}, {}), dict(alpha=0.5, k=6)),
    "lookahead_madgrad": ("MADGRAD", dict(lr=1e-2, momentum=0.9), ({}, {}), dict(alpha=0.8, k=6)),
}


def fixture_start():
    """The start tensors (float64, seeded), one of them with an all-zero row."""
    gen = torch.Generator().manual_seed(20240607)
    ps = [torch.randn(shape, generator=gen, dtype=torch.float64) for shape, _ in FIXTURE_TENSORS]
    ps[6][2] = 0.0  # an all-zero row, as an embedding's padding row
    return ps


def fixture_groups(ps, overrides):
    return [dict(params=ps[:FIXTURE_SPLIT], **overrides[0]), dict(params=ps[FIXTURE_SPLIT:], **overrides[1])]


def fixture_grads(ps, step):
    gs = [None if i == FIXTURE_NO_GRAD else fixture_grad(kind, p.detach(), step, i)
          for i, (p, (_, kind)) in enumerate(zip(ps, FIXTURE_TENSORS))]
    gs[6][2] = 0.0  # the padding row receives no gradient
    return gs
