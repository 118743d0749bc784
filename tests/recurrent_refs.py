"""References of the recurrent kernels (csrc/recurrent.hip, train_recurrent.hip) written from each operation's definition, at
the KERNELS' layouts (transposed weights, the folded location filter wloc / bloc, gates [B][T][8H]).  Plain torch on the CPU,
any dtype: float64 is the reference, and the same functions at float32 give e32.  Shared by tests/test_recurrent_ops_gpu.py
and tests/test_recurrent_refs_cpu.py (which pins them to oracle.restatement).

`mode` selects how every reduction is evaluated (it matters at float32 only):
  "plain"  torch's own matmul / sum
  "rev"    every reduction axis reversed
  "chunk"  every reduction split into 16 chunks that are summed left to right
A single sequential fp32 evaluation does not sample the kernels' part-wise sums; the three together do.
"""
import torch
import torch.nn.functional as F

H = 256
MODES = ("plain", "rev", "chunk")


def mm(mode, a, b):
    """a [..., K] @ b [..., K, N]"""
    if mode == "plain":
        return a @ b
    if mode == "rev":
        return a.flip(-1) @ b.flip(-2)
    acc = None
    for ac, bc in zip(a.chunk(16, dim=-1), b.chunk(16, dim=-2)):
        v = ac @ bc
        acc = v if acc is None else acc + v
    return acc


def rsum(mode, x, dim):
    if mode == "plain":
        return x.sum(dim)
    if mode == "rev":
        return x.flip(dim).sum(dim)
    acc = None
    for c in x.chunk(16, dim=dim):
        v = c.sum(dim)
        acc = v if acc is None else acc + v
    return acc


def lstm_cell(pre, c_prev):
    """gate order i, f, g, o; returns the gates after their nonlinearities, c, h"""
    i, f, g, o = pre.chunk(4, dim=-1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return torch.cat([i, f, g, o], -1), c, o * torch.tanh(c)


# ---------------------------------------------------------------------------------------------------------------------
# bidirectional LSTM from its input projection
# ---------------------------------------------------------------------------------------------------------------------
def bilstm_ref(g, whh_t, mode="plain"):
    """g [B][T][2*4H] (forward | reverse pre-activation input projections, biases included), whh_t [2][H][4H].
    Returns out [B][T][2H], sv_gates [B][T][2*4H] (after the nonlinearities), sv_c [B][T][2H]."""
    B, T, _ = g.shape
    outs, gates, cs = [], [], []
    for d in range(2):
        h = torch.zeros(B, H, dtype=g.dtype)
        c = torch.zeros(B, H, dtype=g.dtype)
        o_t, g_t, c_t = [None] * T, [None] * T, [None] * T
        for step in range(T):
            t = step if d == 0 else T - 1 - step
            pre = g[:, t, d * 4 * H:(d + 1) * 4 * H] + mm(mode, h, whh_t[d])
            act, c, h = lstm_cell(pre, c)
            o_t[t], g_t[t], c_t[t] = h, act, c
        outs.append(torch.stack(o_t, 1))
        gates.append(torch.stack(g_t, 1))
        cs.append(torch.stack(c_t, 1))
    return torch.cat(outs, 2), torch.cat(gates, 2), torch.cat(cs, 2)


def bilstm_hprev_ref(out):
    B, T, _ = out.shape
    hf = torch.zeros(B, T, H, dtype=out.dtype)
    hr = torch.zeros(B, T, H, dtype=out.dtype)
    hf[:, 1:] = out[:, :-1, :H]
    hr[:, :-1] = out[:, 1:, H:]
    return hf, hr


# ---------------------------------------------------------------------------------------------------------------------
# LSTM-attention decoder loop
# ---------------------------------------------------------------------------------------------------------------------
def attn_weights(V, taps, seed, tokgate=False, gen_scale=2.0):
    """Random decoder weights at the kernel's layouts (float32).  N(0, 1) fan-in-scaled, the generator at gen_scale / sqrt(H),
    biases at 0.1."""
    g = torch.Generator().manual_seed(seed)

    def r(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc
    W = dict(
        wk=r(H, H, sc=H ** -0.5), bk=r(H, sc=0.1),  # key projection (the test forms kp with it)
        wq_t=r(H, H, sc=H ** -0.5), bq=r(H, sc=0.1),
        wloc=r(H, taps, sc=1.0), bloc=r(H, sc=0.1), wscore=r(H, sc=4 * H ** -0.5), bscore=0.3,
        wx_t=r(3 * H, 4 * H, sc=(2 * H) ** -0.5), bx=r(4 * H, sc=0.1),
        wg_t=r(H, V, sc=gen_scale * H ** -0.5), bg=r(V, sc=0.1),
        wih_t=r(H, H, sc=H ** -0.5), bih=r(H, sc=0.1), wic_t=r(H, H, sc=H ** -0.5), bic=r(H, sc=0.1))
    if tokgate:
        W["tokgate"] = r(V, 4 * H, sc=0.5)
    else:
        W["emb"] = r(V, H)
    return W


def cast(W, dt):
    return {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in W.items()}


def loc_term(mode, m, wloc, bloc):
    """m [B][Tk] alignment memory -> [B][Tk][H]: bloc[n] + sum_j wloc[n][j] m[t + j - taps // 2], zeros outside"""
    taps = wloc.shape[1]
    half = taps // 2
    u = F.pad(m, (half, taps - 1 - half)).unfold(1, taps, 1)  # [B][Tk][taps]
    return mm(mode, u, wloc.t()) + bloc


def attn_ref(W, mem, kp, S, *, key_off=0, init_mode=0, coverage=True, end_token=1, teacher=None, use_teacher=None,
             dropmask=None, dropscale=1.0, rows=None, state=None, tok_in=None, leaves=None, mode="plain"):
    """The decoder loop.  mem / kp [N][T][H]; rows (optional): the sample of each row (default row b -> sample b).
    state (optional) = (h, c, m) to resume from with the input token tok_in (step mode).  teacher [B][S]: the input token of
    step t is teacher[:, t] at t = 0 and wherever use_teacher[t] != 0 (default everywhere), else the previous argmax.
    leaves (optional dict): receives the tensors the backward is taken with respect to (retain_grad) -- pre [S], hq [S],
    emb [S], h0, c0, and the scores e [S].
    Returns a dict: probs [B][S][V], tokens, end_step, the kernel's sv_* tensors, mem [B][S][Tk] (the alignment memory
    AFTER each step: what step mode leaves in st_mem_out), and the final state."""
    dt = mem.dtype
    rows = list(range(mem.shape[0])) if rows is None else list(rows)
    B = len(rows)
    T = mem.shape[1]
    keys = mem[rows][:, key_off:]
    kpk = kp[rows][:, key_off:]
    Tk = T - key_off
    V = W["wg_t"].shape[1]
    if state is not None:
        h, c, m = state
        tok = tok_in.clone()
    else:
        if init_mode == 0:
            h = torch.zeros(B, H, dtype=dt)
            c = torch.zeros(B, H, dtype=dt)
        else:
            init = rsum(mode, mem[rows], 1) / T if init_mode == 1 else mem[rows][:, 0]
            h = mm(mode, init, W["wih_t"]) + W["bih"]
            c = mm(mode, init, W["wic_t"]) + W["bic"]
        m = torch.zeros(B, Tk, dtype=dt)
        tok = torch.zeros(B, dtype=torch.long)  # [GO]
    if leaves is not None:
        h = h.detach().requires_grad_(True)
        c = c.detach().requires_grad_(True)
        leaves.update(h0=h, c0=c, pre=[], hq=[], emb=[], e=[])
    o = {k: [] for k in ("probs", "tokens", "tok", "hprev", "cprev", "hafter", "cafter", "gates", "alpha", "hq", "x", "mem")}
    for step in range(S):
        if teacher is not None and (step == 0 or use_teacher is None or use_teacher[step]):
            tok = teacher[:, step]
        o["tok"].append(tok)
        o["hprev"].append(h)
        o["cprev"].append(c)
        hq = mm(mode, h, W["wq_t"]) + W["bq"]
        if leaves is not None:
            hq.retain_grad()
            leaves["hq"].append(hq)
        u = torch.tanh(kpk + hq[:, None, :] + loc_term(mode, m, W["wloc"], W["bloc"]))
        e = mm(mode, u, W["wscore"][:, None]).squeeze(-1) + W["bscore"]
        if leaves is not None:
            e.retain_grad()
            leaves["e"].append(e)
        ex = torch.exp(e - e.max(dim=1, keepdim=True).values)
        alpha = ex / rsum(mode, ex, 1)[:, None]
        m = m + alpha if coverage else alpha
        ctx = mm(mode, alpha[:, None, :], keys).squeeze(1)
        if "emb" in W:
            emb = W["emb"][tok]
            if leaves is not None:
                emb = emb.detach().requires_grad_(True)
                leaves["emb"].append(emb)
            pre = mm(mode, torch.cat([ctx, emb, h], 1), W["wx_t"]) + W["bx"]
        else:  # one-hot targets: [ctx ; onehot(tok) ; h] through [W_ctx ; tokgate ; W_h]
            emb = torch.zeros(B, H, dtype=dt)
            wfull = torch.cat([W["wx_t"][:H], W["tokgate"], W["wx_t"][2 * H:]], 0)
            pre = mm(mode, torch.cat([ctx, F.one_hot(tok, V).to(dt), h], 1), wfull) + W["bx"]
        if leaves is not None:
            pre.retain_grad()
            leaves["pre"].append(pre)
        act, c, h = lstm_cell(pre, c)
        logit = mm(mode, h, W["wg_t"]) + W["bg"]
        if dropmask is not None:
            logit = logit * dropmask[:, step].to(dt) * dropscale
        tok = logit.argmax(1)
        for k, v in (("probs", logit), ("tokens", tok), ("hafter", h), ("cafter", c), ("gates", act), ("alpha", alpha), ("hq", hq),
                     ("x", torch.cat([ctx, emb], 1)), ("mem", m)):
            o[k].append(v)
    out = {k: torch.stack(v, 1) for k, v in o.items()}
    toks = out["tokens"]
    is_end = toks == end_token
    out["end_step"] = torch.where(is_end.any(1), is_end.float().argmax(1), torch.full((B,), -1)).to(torch.int32)
    out["state"] = (h, c, m)
    return out


def attn_bwd_ref(W, mem, kp, teacher, dlogits, *, key_off, coverage, mode="plain"):
    """Backward of the teacher-forced loop by torch.autograd on attn_ref, ONE ROW AT A TIME (the score / location layer
    gradients are per-row partials): the per-(row, step) factors the kernel leaves for the caller's GEMMs and the rest of
    AttnTrainBwdP's outputs.  h0 = c0 = 0 (init_mode 0) are leaves.
    dbscore is the sum of the score gradients over steps and keys, which is zero in exact arithmetic (a softmax does not see a
    shift of its scores): what an evaluation returns is the rounding residue of that sum, and it depends on the association
    alone.  autograd sums the keys of a step first and the steps afterwards; dbscore_steps_first is the same sum of the same
    score gradients with the steps summed first and the keys afterwards (each in `mode`'s order), the association of a
    kernel whose threads own keys and walk the steps."""
    B, S = teacher.shape
    out = {k: [] for k in ("dgates", "dhq", "demb", "dh0", "dc0", "dmem", "dkp", "dwloc", "dbloc", "dwscore", "dbscore",
                           "dbscore_steps_first")}
    for b in range(B):
        Wb = dict(W)
        for k in ("wloc", "bloc", "wscore"):
            Wb[k] = W[k].detach().clone().requires_grad_(True)
        Wb["bscore"] = torch.tensor(float(W["bscore"]), dtype=mem.dtype, requires_grad=True)
        mb = mem[b:b + 1].detach().clone().requires_grad_(True)
        kb = kp[b:b + 1].detach().clone().requires_grad_(True)
        lv = {}
        r = attn_ref(Wb, mb, kb, S, key_off=key_off, init_mode=0, coverage=coverage, teacher=teacher[b:b + 1], leaves=lv, mode=mode)
        (r["probs"] * dlogits[b:b + 1]).sum().backward()
        z = torch.zeros(1, H, dtype=mem.dtype)
        out["dgates"].append(torch.stack([p.grad for p in lv["pre"]], 1))
        out["dhq"].append(torch.stack([p.grad for p in lv["hq"]], 1))
        out["demb"].append(torch.stack([p.grad if p.grad is not None else z for p in lv["emb"]], 1))
        out["dh0"].append(lv["h0"].grad)
        out["dc0"].append(lv["c0"].grad)
        out["dmem"].append(mb.grad)
        out["dkp"].append(kb.grad)
        out["dwloc"].append(Wb["wloc"].grad[None])
        out["dbloc"].append(Wb["bloc"].grad[None])
        out["dwscore"].append(Wb["wscore"].grad[None])
        out["dbscore"].append(Wb["bscore"].grad.reshape(1))
        de = torch.stack([p.grad for p in lv["e"]], 1)  # [1][S][Tk]
        out["dbscore_steps_first"].append(rsum(mode, rsum(mode, de, 1), 1))
    return {k: torch.cat(v, 0) for k, v in out.items()}


def bilstm_bwd_ref(g, whh_t, dout, mode="plain"):
    """dgates [B][T][8H] = d sum(out * dout) / d g by autograd (the pre-activation gates are g + h W_hh^T, so their gradient
    is g's)."""
    gl = g.detach().clone().requires_grad_(True)
    out, _, _ = bilstm_ref(gl, whh_t, mode)
    (out * dout).sum().backward()
    return gl.grad


def e32_of(fn, keys=None):
    """fn(dtype, mode) -> dict of tensors (or one tensor).  Returns (y64, e32): the float64 evaluation and, per key, the largest
    max |y32 - y64| over the three float32 evaluations."""
    y64 = fn(torch.float64, "plain")
    single = torch.is_tensor(y64)
    if single:
        y64 = {"y": y64}
    keys = keys or [k for k, v in y64.items() if torch.is_tensor(v) and v.is_floating_point()]
    e32 = {k: 0.0 for k in keys}
    for mode in MODES:
        y32 = fn(torch.float32, mode)
        if single:
            y32 = {"y": y32}
        for k in keys:
            e32[k] = max(e32[k], float((y32[k].double() - y64[k]).abs().max()))
    return (y64["y"], e32["y"]) if single else (y64, e32)
