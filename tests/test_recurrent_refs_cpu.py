"""CPU: the kernel-layout references of tests/recurrent_refs.py (what tests/test_recurrent_ops_gpu.py compares the recurrent
kernels with) agree in float64 with oracle.restatement -- the restatement tests/test_oracle_golden.py ties to the reference
project's recorded outputs -- and with torch.nn.LSTM.  This covers the folded wloc / bloc, the transposes, the tokgate
(one-hot) formulation, the key_off / init_mode conventions, and the three reduction orders of the fp32 evaluations."""
import pytest
import torch
import torch.nn.functional as F

import recurrent_refs as RR
from oracle import restatement as R

H = RR.H
F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _attn_state_dict(V, taps, kd, embed, seed):
    g = torch.Generator().manual_seed(seed)

    def r(*s, sc=1.0):
        return torch.randn(*s, generator=g, dtype=F64) * sc
    p, a = "Prediction.", "Prediction.attention_cell."
    nin = 2 * H if embed else H + V
    sd = {a + "attn.key_proj.weight": r(H, H, sc=H ** -0.5), a + "attn.key_proj.bias": r(H, sc=0.1),
          a + "attn.query_proj.weight": r(H, H, sc=H ** -0.5), a + "attn.query_proj.bias": r(H, sc=0.1),
          a + "attn.loc_conv.weight": r(kd, 1, taps), a + "attn.loc_conv.bias": r(kd, sc=0.1),
          a + "attn.loc_proj.weight": r(H, kd, sc=kd ** -0.5), a + "attn.loc_proj.bias": r(H, sc=0.1),
          a + "attn.score.weight": r(1, H, sc=4 * H ** -0.5), a + "attn.score.bias": r(1),
          a + "rnn.weight_ih": r(4 * H, nin, sc=(2 * H) ** -0.5), a + "rnn.bias_ih": r(4 * H, sc=0.1),
          a + "rnn.weight_hh": r(4 * H, H, sc=H ** -0.5), a + "rnn.bias_hh": r(4 * H, sc=0.1),
          a + "generator.weight": r(V, H, sc=2 * H ** -0.5), a + "generator.bias": r(V, sc=0.1),
          p + "proj_init_h.weight": r(H, H, sc=H ** -0.5), p + "proj_init_h.bias": r(H, sc=0.1),
          p + "proj_init_c.weight": r(H, H, sc=H ** -0.5), p + "proj_init_c.bias": r(H, sc=0.1)}
    if embed:
        sd[p + "embedding.weight"] = r(V, H)
    return sd


def _kernel_layout(sd, embed):
    """what the engine makes of the state dict (csrc/engine.hip), in float64"""
    p, a = "Prediction.", "Prediction.attention_cell."
    Wp, Wc = sd[a + "attn.loc_proj.weight"], sd[a + "attn.loc_conv.weight"][:, 0]
    wih = sd[a + "rnn.weight_ih"]
    W = dict(wq_t=sd[a + "attn.query_proj.weight"].t(), bq=sd[a + "attn.query_proj.bias"],
             wloc=Wp @ Wc, bloc=sd[a + "attn.loc_proj.bias"] + Wp @ sd[a + "attn.loc_conv.bias"],
             wscore=sd[a + "attn.score.weight"][0], bscore=float(sd[a + "attn.score.bias"][0]),
             bx=sd[a + "rnn.bias_ih"] + sd[a + "rnn.bias_hh"], wg_t=sd[a + "generator.weight"].t(), bg=sd[a + "generator.bias"],
             wih_t=sd[p + "proj_init_h.weight"].t(), bih=sd[p + "proj_init_h.bias"],
             wic_t=sd[p + "proj_init_c.weight"].t(), bic=sd[p + "proj_init_c.bias"])
    if embed:
        W["wx_t"] = torch.cat([wih.t(), sd[a + "rnn.weight_hh"].t()], 0)
        W["emb"] = sd[p + "embedding.weight"]
    else:  # one-hot targets: the columns behind the context are added per token; the embedding rows of wx_t meet zeros
        W["wx_t"] = torch.cat([wih[:, :H].t(), torch.full((H, 4 * H), 3.0, dtype=F64), sd[a + "rnn.weight_hh"].t()], 0)
        W["tokgate"] = wih[:, H:].t()
    return W


@pytest.mark.parametrize("attn_type,seqmodel,enc_init,embed,taps,flags", [
    ("coverage", "BiLSTM", True, True, 11, None), ("loc_aware", "TFM", True, False, 3, None),
    ("coverage", "first", False, True, 1, [1, 1, 0, 1, 0, 0]), ("loc_aware", "first", True, True, 11, None)])
def test_attn_reference_agrees_with_the_restatement(attn_type, seqmodel, enc_init, embed, taps, flags):
    B, T, S, V = 3, 9, 6, 23
    sd = _attn_state_dict(V, taps, 16, embed, seed=taps)
    g = torch.Generator().manual_seed(5)
    mem = torch.randn(B, T, H, generator=g, dtype=F64)
    teacher = torch.randint(0, V, (B, S), generator=g)
    teacher[:, 0] = R.ATTN_GO
    _, want = R.attn_greedy(mem, sd, "Prediction.", S, seqmodel, attn_type=attn_type, enc_init=enc_init, teacher=teacher, flags=flags,
                            embed_target=embed)
    a = "Prediction.attention_cell."
    kp = F.linear(mem, sd[a + "attn.key_proj.weight"], sd[a + "attn.key_proj.bias"])
    kw = dict(key_off=1 if seqmodel == "TFM" else 0, init_mode=0 if not enc_init else (1 if seqmodel == "BiLSTM" else 2),
              coverage=attn_type == "coverage", teacher=teacher, use_teacher=flags)
    W = _kernel_layout(sd, embed)
    for mode in RR.MODES:  # in float64 the three reduction orders are the same function
        got = RR.attn_ref(W, mem, kp, S, mode=mode, **kw)
        assert _rel(got["probs"], want) <= 1e-12, mode
    # greedy (no teacher): the same tokens and values
    toks, want = R.attn_greedy(mem, sd, "Prediction.", S, seqmodel, attn_type=attn_type, enc_init=enc_init, embed_target=embed)
    del kw["teacher"], kw["use_teacher"]
    got = RR.attn_ref(W, mem, kp, S, **kw)
    assert torch.equal(got["tokens"], toks) and _rel(got["probs"], want) <= 1e-12
    # the saved tensors are consistent with the loop: x = [context | embedding], state before / after
    assert torch.equal(got["hprev"][:, 1:], got["hafter"][:, :-1]) and torch.equal(got["cprev"][:, 1:], got["cafter"][:, :-1])
    assert _rel(got["alpha"].sum(-1), torch.ones(B, S, dtype=F64)) <= 1e-12


def test_attn_reference_step_mode_resumes_the_loop():
    B, T, S, V = 2, 7, 4, 11
    W = RR.cast(RR.attn_weights(V, 3, seed=3), F64)
    mem = torch.randn(B, T, H, generator=torch.Generator().manual_seed(1), dtype=F64)
    kp = mem @ W["wk"].t() + W["bk"]
    fed = torch.randint(0, V, (4, S), generator=torch.Generator().manual_seed(2))
    rows = [1, 0, 0, 1]
    loop = RR.attn_ref(W, mem, kp, S, rows=rows, key_off=1, init_mode=2, teacher=fed)
    state = None
    for s in range(S):
        st = RR.attn_ref(W, mem, kp, 1, rows=rows, key_off=1, init_mode=2, state=state, tok_in=fed[:, s],
                         teacher=fed[:, :1] if s == 0 else None)
        assert _rel(st["probs"][:, 0], loop["probs"][:, s]) <= 1e-12
        state = st["state"]


@pytest.mark.parametrize("B,T", [(1, 1), (3, 5)])
def test_bilstm_reference_agrees_with_the_restatement_and_nn_lstm(B, T):
    g = torch.Generator().manual_seed(B + T)
    nin = 40
    sd = {}
    for sfx in ("", "_reverse"):
        sd["S.rnn.weight_ih_l0" + sfx] = torch.randn(4 * H, nin, generator=g, dtype=F64) * nin ** -0.5
        sd["S.rnn.weight_hh_l0" + sfx] = torch.randn(4 * H, H, generator=g, dtype=F64) * H ** -0.5
        sd["S.rnn.bias_ih_l0" + sfx] = torch.randn(4 * H, generator=g, dtype=F64) * 0.1
        sd["S.rnn.bias_hh_l0" + sfx] = torch.randn(4 * H, generator=g, dtype=F64) * 0.1
    sd["S.linear.weight"] = torch.randn(H, 2 * H, generator=g, dtype=F64) * (2 * H) ** -0.5
    sd["S.linear.bias"] = torch.randn(H, generator=g, dtype=F64)
    x = torch.randn(B, T, nin, generator=g, dtype=F64)
    want = R.bilstm(x, sd, "S.")
    gates = torch.cat([F.linear(x, sd["S.rnn.weight_ih_l0" + s], sd["S.rnn.bias_ih_l0" + s] + sd["S.rnn.bias_hh_l0" + s])
                       for s in ("", "_reverse")], 2)
    whh_t = torch.stack([sd["S.rnn.weight_hh_l0"].t(), sd["S.rnn.weight_hh_l0_reverse"].t()])
    for mode in RR.MODES:
        out, sg, sc = RR.bilstm_ref(gates, whh_t, mode)
        assert _rel(F.linear(out, sd["S.linear.weight"], sd["S.linear.bias"]), want) <= 1e-12
    lstm = torch.nn.LSTM(nin, H, bidirectional=True, batch_first=True).double()
    lstm.load_state_dict({k[len("S.rnn."):]: v for k, v in sd.items() if k.startswith("S.rnn.")})
    with torch.no_grad():
        ref, _ = lstm(x)
    assert _rel(out, ref) <= 1e-12
    # the saves: c from the saved gates, h = o tanh(c); the backward reference is autograd through the same function
    i, f, gg, o = sg[..., :4 * H].chunk(4, -1)
    assert _rel(o * torch.tanh(sc[..., :H]), out[..., :H]) <= 1e-12
    dout = torch.randn(B, T, 2 * H, generator=g, dtype=F64)
    xl = x.clone().requires_grad_(True)
    (lstm(xl)[0] * dout).sum().backward()
    dg = RR.bilstm_bwd_ref(gates, whh_t, dout)
    wcat = torch.cat([sd["S.rnn.weight_ih_l0"], sd["S.rnn.weight_ih_l0_reverse"]], 0)  # dx = dgates . [W_ih ; W_ih_reverse]
    assert _rel(dg @ wcat, xl.grad) <= 1e-12
    hf, hr = RR.bilstm_hprev_ref(out)
    assert torch.equal(hf[:, 0], torch.zeros(B, H, dtype=F64)) and torch.equal(hr[:, -1], torch.zeros(B, H, dtype=F64))
    if T > 1:
        assert torch.equal(hf[:, 1], out[:, 0, :H]) and torch.equal(hr[:, 0], out[:, 1, H:])
