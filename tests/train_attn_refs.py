"""References of the training step's softmax attention (csrc/train_attn.hip: forward saving the probabilities, backward writing dS
over them) at the KERNELS' layouts: q [nb*Lq][D], kv [nb*Lk][2D] (keys | values), or one packed qkv [nb*L][3D]; heads are column
blocks of hd; keytok [nb][Lk] token ids whose PAD (0) keys are masked; keep [nb][heads][Lq][Lk] bytes, the dropout of
nn.MultiheadAttention on the probabilities (kept entries times `dropscale`).  Plain torch on the CPU, any dtype: float64 is the
reference, the same functions at float32 in the three reduction orders of tests/recurrent_refs.py give e32.

  attn_forward    scale, causal mask, key-padding mask, softmax, keep mask x scale, @ V -> y and the probabilities BEFORE dropout
  attn_autograd   torch.autograd on attn_forward: dq, dk, dv, and the gradient of the scores
  attn_backward   the formulas of train_attn.hip's header restated, so that dS has a reference and the backward an fp32 evaluation:
                  dV = (P o D)^T dO;  dP = (dO V^T) o D;  dS = P (dP - rowsum(dP P));  dQ = scale dS K;  dK = scale dS^T Q
tests/test_train_attn_refs_cpu.py pins them to F.scaled_dot_product_attention, nn.MultiheadAttention and autograd.
Every row needs at least one unmasked key (the first key of a row is never PAD, as in the decoder: [GO]).
"""
import torch

from recurrent_refs import MODES, mm, rsum

OUTPUTS = ("y", "probs", "ds", "dq", "dk", "dv")


def heads_of(x, nb, L, heads, hd):
    """[nb*L][>= heads*hd columns given] -> [nb][heads][L][hd]"""
    return x.reshape(nb, L, heads, hd).transpose(1, 2)


def rows_of(x):
    """[nb][heads][L][hd] -> [nb*L][heads*hd]"""
    nb, heads, L, hd = x.shape
    return x.transpose(1, 2).reshape(nb * L, heads * hd)


def operands(D, q=None, kv=None, qkv=None):
    """the three [rows][D] operands of either layout"""
    if qkv is not None:
        return qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    return q, kv[:, :D], kv[:, D:]


def valid_keys(nb, Lq, Lk, causal, keytok):
    """bool [nb][1][Lq][Lk]: True where query i may look at key j"""
    ok = torch.ones(nb, 1, Lq, Lk, dtype=torch.bool)
    if causal:
        ok &= ~torch.ones(Lq, Lk, dtype=torch.bool).triu(1)
    if keytok is not None:
        ok &= (keytok != 0)[:, None, None, :]
    return ok


def attn_forward(Q, K, V, valid, keep=None, dropscale=1.0, mode="plain", leaves=None):
    """Q [nb][heads][Lq][hd], K / V [nb][heads][Lk][hd] -> y [nb][heads][Lq][hd], probs [nb][heads][Lq][Lk] (before dropout).
    leaves (optional dict): receives the masked, scaled scores `s` with retain_grad."""
    hd = Q.shape[-1]
    s = mm(mode, Q, K.transpose(-1, -2)) * hd ** -0.5
    s = s.masked_fill(~valid, float("-inf"))
    if leaves is not None:
        s.retain_grad()
        leaves["s"] = s
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    P = e / rsum(mode, e, -1)[..., None]
    used = P if keep is None else P * (keep.to(P.dtype) * dropscale)
    return mm(mode, used, V), P


def attn_backward(Q, K, V, P, dO, keep=None, dropscale=1.0, mode="plain"):
    """the header's formulas; returns dQ, dK, dV, dS"""
    hd = Q.shape[-1]
    Dm = None if keep is None else keep.to(P.dtype) * dropscale
    used = P if Dm is None else P * Dm
    dV = mm(mode, used.transpose(-1, -2), dO)
    dP = mm(mode, dO, V.transpose(-1, -2))
    if Dm is not None:
        dP = dP * Dm
    dS = P * (dP - rsum(mode, dP * P, -1)[..., None])
    dQ = mm(mode, dS, K) * hd ** -0.5
    dK = mm(mode, dS.transpose(-1, -2), Q) * hd ** -0.5
    return dQ, dK, dV, dS


def _split(dt, nb, Lq, Lk, heads, hd, q, kv, qkv, dy):
    D = heads * hd
    q2, k2, v2 = operands(D, None if q is None else q.to(dt), None if kv is None else kv.to(dt), None if qkv is None else qkv.to(dt))
    return (heads_of(q2, nb, Lq, heads, hd), heads_of(k2, nb, Lk, heads, hd), heads_of(v2, nb, Lk, heads, hd),
            heads_of(dy.to(dt), nb, Lq, heads, hd))


def attn_eval(dt, mode, nb, Lq, Lk, heads, hd, causal, dy, q=None, kv=None, qkv=None, keytok=None, keep=None, dropscale=1.0):
    """forward and the explicit backward at dtype dt, reductions in `mode`, from and to the kernels' layouts: y, dq [nb*Lq][D],
    dk, dv [nb*Lk][D], probs, ds [nb][heads][Lq][Lk]"""
    Q, K, V, dO = _split(dt, nb, Lq, Lk, heads, hd, q, kv, qkv, dy)
    valid = valid_keys(nb, Lq, Lk, causal, keytok)
    y, P = attn_forward(Q, K, V, valid, keep, dropscale, mode)
    dQ, dK, dV, dS = attn_backward(Q, K, V, P, dO, keep, dropscale, mode)
    return dict(y=rows_of(y), probs=P, ds=dS, dq=rows_of(dQ), dk=rows_of(dK), dv=rows_of(dV))


def attn_autograd(nb, Lq, Lk, heads, hd, causal, dy, q=None, kv=None, qkv=None, keytok=None, keep=None, dropscale=1.0,
                  dt=torch.float64):
    """forward and torch.autograd: the same keys as attn_eval; ds is the gradient of the masked, scaled scores.  In the packed
    layout dq / dk / dv are the column slices of the one gradient of qkv."""
    D = heads * hd
    src = [None if t is None else t.to(dt).detach().clone().requires_grad_(True) for t in (q, kv, qkv)]
    Q, K, V, dO = _split(dt, nb, Lq, Lk, heads, hd, *src, dy)
    leaves = {}
    y, P = attn_forward(Q, K, V, valid_keys(nb, Lq, Lk, causal, keytok), keep, dropscale, "plain", leaves)
    y.backward(dO)
    if qkv is not None:
        g = src[2].grad
        dq, dk, dv = g[:, :D], g[:, D:2 * D], g[:, 2 * D:]
    else:
        dq, dk, dv = src[0].grad, src[1].grad[:, :D], src[1].grad[:, D:]
    return dict(y=rows_of(y.detach()), probs=P.detach(), ds=leaves["s"].grad, dq=dq, dk=dk, dv=dv)


def attn_ref_and_e32(**case):
    """(y64, e32): the float64 reference (autograd for dq / dk / dv, the explicit formula for ds) and, per output, the largest
    max |x32 - x64| over the three float32 evaluations of forward and explicit backward"""
    y64 = attn_autograd(**case)
    y64["ds"] = attn_eval(torch.float64, "plain", **case)["ds"]
    e32 = {k: 0.0 for k in OUTPUTS}
    for mode in MODES:
        y32 = attn_eval(torch.float32, mode, **case)
        for k in OUTPUTS:
            e32[k] = max(e32[k], float((y32[k].double() - y64[k]).abs().max()))
    return y64, e32


def make_inputs(nb, Lq, Lk, heads, hd, pad, seed):
    """q, kv, dy ~ N(0, 1) and, with pad, token rows that end in PAD (0) keys (never the first key)"""
    g = torch.Generator().manual_seed(seed)
    D = heads * hd
    q, kv, dy = torch.randn(nb * Lq, D, generator=g), torch.randn(nb * Lk, 2 * D, generator=g), torch.randn(nb * Lq, D, generator=g)
    keytok = None
    if pad:
        keytok = torch.randint(4, 100, (nb, Lk), generator=g)
        for b in range(nb):
            keytok[b, max(1, Lk - 3 * b - 2):] = 0
    return q, kv, dy, keytok


def keep_mask(nb, heads, Lq, Lk, p, seed):
    """a random keep mask, bytes: an entry is dropped with probability p"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(nb, heads, Lq, Lk, generator=g) >= p).to(torch.uint8)
