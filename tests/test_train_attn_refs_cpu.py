"""CPU: tests/train_attn_refs.py, the float64 references of tests/test_train_attn_ops_gpu.py, pinned to 1e-12 of each tensor's
largest magnitude against what torch itself computes: the forward against F.scaled_dot_product_attention with the causal and
key-padding masks; where the dropout sits against nn.MultiheadAttention in training mode (identity projections, zero biases,
torch.nn.functional.dropout replaced for the call by "multiply by the given mask and scale"); the explicit backward, dS
included, against autograd; the packed layout against the separate one."""
import pytest
import torch
import torch.nn.functional as F

import train_attn_refs as AR

F64 = torch.float64
TOL = 1e-12
# nb, Lq, Lk, heads, hd, causal, pad
CASES = [(2, 9, 9, 2, 32, 0, False), (3, 25, 25, 8, 32, 1, True), (2, 23, 23, 8, 64, 1, True), (3, 25, 70, 8, 32, 0, False),
         (1, 1, 1, 1, 32, 0, False), (1, 8, 65, 2, 64, 0, True), (2, 5, 5, 2, 32, 1, False)]
_id = lambda c: "x".join(map(str, c[:5])) + ("-causal" if c[5] else "") + ("-pad" if c[6] else "")


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _case(c, p=None):
    nb, Lq, Lk, heads, hd, causal, pad = c
    q, kv, dy, keytok = AR.make_inputs(nb, Lq, Lk, heads, hd, pad, seed=sum(c) + 7)
    k = dict(nb=nb, Lq=Lq, Lk=Lk, heads=heads, hd=hd, causal=causal, dy=dy, q=q, kv=kv, keytok=keytok)
    if p is not None:
        k.update(keep=AR.keep_mask(nb, heads, Lq, Lk, p, seed=sum(c)), dropscale=1.0 / (1.0 - p))
    return k


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_forward_is_scaled_dot_product_attention(c):
    nb, Lq, Lk, heads, hd, causal, pad = c
    k = _case(c)
    got = AR.attn_eval(F64, "plain", **k)
    D = heads * hd
    Q, K, V = (AR.heads_of(t.double(), nb, L, heads, hd) for t, L in ((k["q"], Lq), (k["kv"][:, :D], Lk), (k["kv"][:, D:], Lk)))
    valid = AR.valid_keys(nb, Lq, Lk, causal, k["keytok"])
    want = AR.rows_of(F.scaled_dot_product_attention(Q, K, V, attn_mask=valid))
    assert _rel(got["y"], want) <= TOL
    P = got["probs"]
    assert float((P.sum(-1) - 1).abs().max()) <= 1e-14 and bool((P[~valid.expand_as(P)] == 0).all())


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_dropout_sits_where_multihead_attention_puts_it(c, p, monkeypatch):
    nb, Lq, Lk, heads, hd, causal, pad = c
    k = _case(c, p)
    D = heads * hd
    got = AR.attn_eval(F64, "plain", **k)
    mha = torch.nn.MultiheadAttention(D, heads, dropout=p, batch_first=True).double().train()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(D, dtype=F64).repeat(3, 1))
        mha.in_proj_bias.zero_()
        mha.out_proj.weight.copy_(torch.eye(D, dtype=F64))
        mha.out_proj.bias.zero_()
    calls = []

    def given_mask(x, p=0.5, training=True, inplace=False):
        calls.append(tuple(x.shape))
        return x * (k["keep"].reshape(nb * heads, Lq, Lk).double() * k["dropscale"])
    monkeypatch.setattr(F, "dropout", given_mask)
    out, w = mha(k["q"].double().view(nb, Lq, D), k["kv"][:, :D].double().reshape(nb, Lk, D),
                 k["kv"][:, D:].double().reshape(nb, Lk, D),
                 key_padding_mask=None if k["keytok"] is None else k["keytok"] == 0,
                 attn_mask=torch.ones(Lq, Lk, dtype=torch.bool).triu(1) if causal else None, need_weights=True,
                 average_attn_weights=False)
    assert calls == [(nb * heads, Lq, Lk)]  # once, on the probabilities
    assert _rel(got["y"], out.reshape(nb * Lq, D)) <= TOL
    assert _rel(got["probs"] * (k["keep"].double() * k["dropscale"]), w) <= TOL  # (the module returns them after its dropout)


@pytest.mark.parametrize("p", [None, 0.1, 0.5])
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_explicit_backward_is_autograd(c, p):
    k = _case(c, p)
    got, want = AR.attn_eval(F64, "plain", **k), AR.attn_autograd(**k)
    for name in AR.OUTPUTS:
        assert got[name].shape == want[name].shape
        assert _rel(got[name], want[name]) <= TOL, name
    if c[6] or c[5]:  # masked entries take no gradient
        valid = AR.valid_keys(c[0], c[1], c[2], c[5], k["keytok"]).expand_as(got["ds"])
        assert bool((got["ds"][~valid] == 0).all()) and bool((want["ds"][~valid] == 0).all())


@pytest.mark.parametrize("p", [None, 0.5])
@pytest.mark.parametrize("c", [c for c in CASES if c[1] == c[2]], ids=_id)
def test_packed_layout_is_the_separate_one(c, p):
    k = _case(c, p)
    packed = dict(k, q=None, kv=None, qkv=torch.cat([k["q"], k["kv"]], 1))
    for fn in (lambda **kw: AR.attn_eval(F64, "plain", **kw), AR.attn_autograd):
        a, b = fn(**k), fn(**packed)
        for name in AR.OUTPUTS:
            assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("c", CASES[:4], ids=_id)
def test_float32_evaluations_surround_the_reference(c):
    """e32 is the error of fp32 arithmetic, not of a different function: the three orders stay within 1e-4 of float64, relative
    to each tensor's largest magnitude, and differ from each other where there is more than one term"""
    k = _case(c, 0.1)
    y64, e32 = AR.attn_ref_and_e32(**k)
    for name in AR.OUTPUTS:
        assert 0.0 < e32[name] <= 1e-4 * float(y64[name].abs().max()), (name, e32[name])
