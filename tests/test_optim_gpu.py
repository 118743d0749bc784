"""GPU: doc2tex_amd.optim's fused step (clip + Adam / AdamW + engine weight refresh, include/d2t.h "fused optimizer step")
against the float64 restatement in tests/optim_refs.py.

The yardstick of every update comparison is torch's own fp32 step on the same device and inputs --
clip_grad_norm_ + torch.optim.Adam(W)(foreach=False, fused=False): for each of p, exp_avg and exp_avg_sq the fused kernel's
largest absolute error against float64 may be at most TWICE torch's on that tensor plus one fp32 ulp of the tensor's largest
magnitude (both are chains of about a dozen roundings that differ only in operation order and FMA contraction).  Each side
is held against the float64 step whose clip coefficient comes from its OWN reported norm, so the norm's error (bounded
separately, test_norm_*) is not counted twice.  The measured pairs are in DESIGN.md ("fused optimizer step")."""
import ctypes as C
import functools

import pytest
import torch

import optim_refs as OR
from conftest import engine_model
from doc2tex_amd import _lib, synth
from doc2tex_amd import optim as O
from test_oracle_golden import _case, train_step_labels

pytestmark = pytest.mark.gpu
DEV = "cuda"
CH = O.CHUNK
NUMELS = [1, 3, 4, 5, 255, 256, 257, 1023, 1025, CH - 1, CH, CH + 1, 2 * CH + 7]
ZERO_GRAD, NO_GRAD, SPLIT = 4, 6, 7  # an all-zero gradient; grad None; tensors [:SPLIT] form group 0, the rest group 1
HYPER = [(1e-3, 0.01), (3e-3, 0.1)]  # (lr, weight_decay) of the two groups
BETAS, EPS = (0.9, 0.999), 1e-8


@functools.lru_cache(maxsize=None)
def _problem(seed=11):
    """Seeded CPU tensors, never written: p, g, m ~ normal, v = normal^2."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(NUMELS):
        p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        m, v = 0.1 * torch.randn(n, generator=gen), (0.1 * torch.randn(n, generator=gen)) ** 2
        if i == ZERO_GRAD:
            g = torch.zeros(n)
        out.append((p, g, m, v))
    return out


def _instantiate(prob, grads=None):
    """Fresh device parameters with their gradients set: every odd tensor's gradient is a view that starts one float into a
    larger buffer (4-byte aligned only: the kernels' scalar path, as the data-parallel bucket views are)."""
    ps = []
    for i, (p, g, _, _) in enumerate(prob):
        q = torch.nn.Parameter(p.to(DEV).clone())
        g = g if grads is None else grads[i]
        if i == NO_GRAD:
            q.grad = None
        elif i % 2 == 1:
            buf = torch.zeros(g.numel() + 1, device=DEV)
            buf[1:] = g.to(DEV)
            q.grad = buf[1:]
            assert q.grad.data_ptr() % 16 == 4
        else:
            q.grad = g.to(DEV).clone()
            assert q.grad.data_ptr() % 16 == 0
        ps.append(q)
    return ps


def _groups(ps):
    return [{"params": ps[:SPLIT], "lr": HYPER[0][0], "weight_decay": HYPER[0][1]},
            {"params": ps[SPLIT:], "lr": HYPER[1][0], "weight_decay": HYPER[1][1]}]


def _load_state(opt, prob, start):
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(start)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
                   for i, (_, _, m, v) in enumerate(prob)}
    opt.load_state_dict(sd)


def _fused_step(decoupled, mgn, start, prob=None):
    prob = prob or _problem()
    ps = _instantiate(prob)
    opt = (O.FusedAdamW if decoupled else O.FusedAdam)(_groups(ps), betas=BETAS, eps=EPS, max_grad_norm=mgn)
    _load_state(opt, prob, start)
    grads_before = [None if p.grad is None else p.grad.clone() for p in ps]
    opt.step()
    torch.cuda.synchronize()
    for p, g in zip(ps, grads_before):  # the gradients are read only: left unclipped, bit for bit
        assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))
    return {"p": [p.detach().cpu() for p in ps], "m": [opt.state[p]["exp_avg"].cpu() for p in ps],
            "v": [opt.state[p]["exp_avg_sq"].cpu() for p in ps], "step": [float(opt.state[p]["step"]) for p in ps],
            "norm": None if opt.grad_norm is None else opt.grad_norm.cpu()}


_fused_step_cached = functools.lru_cache(maxsize=None)(_fused_step)


def _torch_step(snap, decoupled, mgn):
    """The yardstick: clip_grad_norm_ + torch's single-tensor fp32 step on clones of `snap` (a list of dicts p, g, m, v, step,
    lr, wd; g None = no gradient), one group per tensor.  Returns ([(p, m, v)], the norm it reported)."""
    qs = [torch.nn.Parameter(s["p"].to(DEV).clone()) for s in snap]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{"params": [q], "lr": s["lr"], "weight_decay": s["wd"]} for q, s in zip(qs, snap)], betas=BETAS, eps=EPS,
              foreach=False, fused=False)
    for q, s in zip(qs, snap):
        q.grad = None if s["g"] is None else s["g"].to(DEV).clone()
        opt.state[q] = {"step": torch.tensor(float(s["step"])), "exp_avg": s["m"].to(DEV).clone(),
                        "exp_avg_sq": s["v"].to(DEV).clone()}
    norm = None
    if mgn is not None:
        norm = float(torch.nn.utils.clip_grad_norm_(qs, mgn, foreach=False))
    opt.step()
    return [(q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]) for q in qs], norm


def _check_update(snap, got, norm_fused, decoupled, mgn, label):
    """got[i] = (p, m, v) after the fused step from `snap`.  Asserts the yardstick bound on every tensor; returns the worst
    (fused error, torch error, allowed) per quantity for the record."""
    yard, norm_torch = _torch_step(snap, decoupled, mgn)
    ck = OR.clip_coef(norm_fused, mgn) if mgn is not None else 1.0
    ct = OR.clip_coef(norm_torch, mgn) if mgn is not None else 1.0
    worst = {}
    for i, s in enumerate(snap):
        if s["g"] is None:
            continue
        args = (s["p"].to(DEV), s["g"].to(DEV), s["m"].to(DEV), s["v"].to(DEV), s["step"] + 1, s["lr"], BETAS, EPS, s["wd"], decoupled)
        ref_k, ref_t = OR.adam_step(*args, ck), OR.adam_step(*args, ct)
        for q, name in enumerate("pmv"):
            ok, e_got, e_yard, allowed = OR.within_yardstick(got[i][q], ref_k[q], yard[i][q], ref_t[q])
            if name not in worst or e_got - allowed > worst[name][0] - worst[name][2]:
                worst[name] = (e_got, e_yard, allowed, i)
            assert ok, (label, i, s["p"].numel(), name, "fused", e_got, "torch", e_yard, "allowed", allowed)
    print(f"[optim] {label}: " + "  ".join(f"{k}: fused {w[0]:.3e} torch {w[1]:.3e} allowed {w[2]:.3e} (tensor {w[3]})"
                                          for k, w in sorted(worst.items())))
    return worst


def _snap(prob, start, grads=None):
    return [{"p": p, "g": None if i == NO_GRAD else (g if grads is None else grads[i]), "m": m, "v": v, "step": start,
             "lr": HYPER[i >= SPLIT][0], "wd": HYPER[i >= SPLIT][1]} for i, (p, g, m, v) in enumerate(prob)]


# ---- 5. the norm ---------------------------------------------------------------------------------------------------
def test_norm_is_the_float64_norm_and_reproducible():
    """2e-5 relative, derived: a thread's serial fp32 sum has at most CHUNK / 256 = 128 terms at 2^-24 each (7.6e-6), all
    above it is double, the square root halves the relative error, and one fp32 rounding (6e-8) stores it."""
    assert CH // 256 <= 256
    r = _fused_step_cached(True, 5.0, 0)
    want = OR.grad_norm([g for i, (_, g, _, _) in enumerate(_problem()) if i != NO_GRAD])
    got = float(r["norm"])
    print(f"[optim] norm: fused {got!r} float64 {want!r} rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 2e-5 * want
    again = _fused_step(True, 5.0, 0)
    assert torch.equal(again["norm"], r["norm"])
    assert _fused_step_cached(True, None, 0)["norm"] is None  # no clipping: the norm kernel is skipped


# ---- 6. the update -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 999])
@pytest.mark.parametrize("mgn", [5.0, 1e4, None], ids=["clip", "noclip", "none"])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_update_within_twice_torchs_error(decoupled, mgn, start):
    prob = _problem()
    r = _fused_step_cached(decoupled, mgn, start)
    if mgn is not None:
        norm = float(r["norm"])
        assert (norm > mgn) == (mgn == 5.0)  # the clamp is active in the one case and not in the other
    got = list(zip(r["p"], r["m"], r["v"]))
    _check_update(_snap(prob, start), got, None if mgn is None else float(r["norm"]), decoupled, mgn,
                  f"{'adamw' if decoupled else 'adam'} mgn={mgn} step={start + 1}")
    # the tensor without a gradient: parameter, state and step count untouched
    p, _, m, v = prob[NO_GRAD]
    assert torch.equal(r["p"][NO_GRAD], p) and torch.equal(r["m"][NO_GRAD], m) and torch.equal(r["v"][NO_GRAD], v)
    assert r["step"][NO_GRAD] == start and all(s == start + 1 for i, s in enumerate(r["step"]) if i != NO_GRAD)
    # a zero gradient still moves its tensor (momentum, decay), exactly as the reference says
    assert not torch.equal(r["p"][ZERO_GRAD], prob[ZERO_GRAD][0])


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_update_is_bit_reproducible(decoupled):
    a, b = _fused_step_cached(decoupled, 5.0, 999), _fused_step(decoupled, 5.0, 999)
    for k in "pmv":
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k


def test_no_clipping_equals_a_huge_bound_bit_for_bit():
    """coef = 1 multiplies exactly: max_grad_norm=None (two launches fewer) and a bound never reached give the same bits."""
    a, b = _fused_step_cached(True, None, 0), _fused_step_cached(True, 1e4, 0)
    for k in "pmv":
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k


# ---- 7. interchange with torch.optim -------------------------------------------------------------------------------
def test_state_from_torch_adamw_continues_in_the_fused_step():
    prob = _problem()
    gen = torch.Generator().manual_seed(23)
    step_grads = [[torch.randn(n, generator=gen) for n in NUMELS] for _ in range(3)]
    ps = _instantiate(prob)
    topt = torch.optim.AdamW(_groups(ps), betas=BETAS, eps=EPS, foreach=False, fused=False)
    for grads in step_grads[:2]:
        for i, p in enumerate(ps):
            p.grad = None if i == NO_GRAD else grads[i].to(DEV)
        torch.nn.utils.clip_grad_norm_(ps, 5.0)
        topt.step()
    sd = topt.state_dict()
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    fopt = O.FusedAdamW(_groups(qs), betas=BETAS, eps=EPS, max_grad_norm=5.0)
    fopt.load_state_dict(sd)
    snap = []
    for i, p in enumerate(ps):
        st = topt.state.get(p, {})
        snap.append({"p": p.detach().cpu().clone(), "g": None if i == NO_GRAD else step_grads[2][i],
                     "m": st["exp_avg"].cpu().clone() if st else None, "v": st["exp_avg_sq"].cpu().clone() if st else None,
                     "step": 2, "lr": HYPER[i >= SPLIT][0], "wd": HYPER[i >= SPLIT][1]})
    for i, q in enumerate(qs):
        q.grad = None if i == NO_GRAD else step_grads[2][i].to(DEV)
    fopt.step()
    torch.cuda.synchronize()
    assert NO_GRAD not in sd["state"] and qs[NO_GRAD] not in fopt.state
    got = [(q.detach(), fopt.state[q]["exp_avg"], fopt.state[q]["exp_avg_sq"]) if i != NO_GRAD else None for i, q in enumerate(qs)]
    assert all(float(fopt.state[q]["step"]) == 3.0 for i, q in enumerate(qs) if i != NO_GRAD)
    snap[NO_GRAD].update(m=torch.zeros(NUMELS[NO_GRAD]), v=torch.zeros(NUMELS[NO_GRAD]))
    _check_update(snap, got, float(fopt.grad_norm), True, 5.0, "third step on torch.optim.AdamW's state")
    # and back: torch's AdamW loads what the fused class saves and steps on
    back = torch.optim.AdamW(_groups(qs), betas=BETAS, eps=EPS)
    back.load_state_dict(fopt.state_dict())
    back.step()
    assert float(back.state[qs[0]]["step"]) == 4.0


# ---- 8. GradScaler -------------------------------------------------------------------------------------------------
def test_grad_scaler_skips_on_inf_and_steps_otherwise():
    prob = _problem()
    ps = _instantiate(prob)
    opt = O.FusedAdamW(_groups(ps), betas=BETAS, eps=EPS, max_grad_norm=5.0)
    _load_state(opt, prob, 5)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    scaler.scale(torch.ones((), device=DEV))  # creates the scale tensor, as scaler.scale(loss) does in a training loop
    for p in ps:
        if p.grad is not None:
            p.grad.mul_(1024.0)
    unscaled = [None if p.grad is None else p.grad / 1024.0 for p in ps]
    ps[9].grad[17] = float("inf")
    before = [p.detach().clone() for p in ps]
    scaler.unscale_(opt)
    scaler.step(opt)
    scaler.update()
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before))
    assert all(float(opt.state[p]["step"]) == 5.0 for p in ps)
    assert all(torch.equal(opt.state[p]["exp_avg"].cpu(), prob[i][2]) for i, p in enumerate(ps))
    assert float(scaler.get_scale()) == 512.0
    for p, g in zip(ps, unscaled):
        if g is not None:
            p.grad.copy_(g * 512.0)
    scaler.unscale_(opt)
    for p, g in zip(ps, unscaled):
        assert g is None or torch.equal(p.grad, g)  # powers of two: the unscaled gradients are the plain ones
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert float(scaler.get_scale()) == 512.0
    plain = _fused_step_cached(True, 5.0, 5)
    for i, p in enumerate(ps):
        assert float(opt.state[p]["step"]) == (5.0 if i == NO_GRAD else 6.0)
        assert torch.equal(p.detach().cpu(), plain["p"][i]), i  # the very step a loop without a scaler takes


# ---- 9. the whole model ----------------------------------------------------------------------------------------------
def _forward_backward(m, img, text):
    m.train()
    m.zero_grad()
    _, preds, _ = m(img, text[:, :-1])
    cost = torch.nn.functional.cross_entropy(preds.view(-1, preds.shape[-1]), text[:, 1:].contiguous().view(-1),
                                             ignore_index=0, reduction="none")
    cost.mean().backward()
    return preds.detach()


@pytest.mark.parametrize("bucket_views", [False, True], ids=["gather", "gradsync"])
def test_whole_model_step_refreshes_the_engine(cases, bucket_views):
    c = _case(cases, "train_step", "t2_train_step")
    _, m = engine_model(c["config"], c["max_seq_len"], c["wseed"])
    if bucket_views:
        from doc2tex_amd.dist import GradSync
        m.grad_sync = GradSync()  # one process: no collective, but the gradients arrive as views of flat buckets
    img = synth.synth_images(c["B"], c["H"], c["W"], seed=c["iseed"]).to(DEV)
    text = train_step_labels(c).to(DEV)
    opt = O.create_optimizer(m, opt="adamw", lr=1e-3, weight_decay=0.01, momentum=0.9, filter_bias_and_bn=True,
                             max_grad_norm=5.0)
    assert isinstance(opt, O.FusedAdamW)
    _forward_backward(m, img, text)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert all(p.grad is not None for _, p in named)
    if bucket_views:
        # views into the flat buckets, packed without padding (at this model's sizes they happen to stay 16-byte aligned;
        # the 4-byte aligned path is what the free-standing tests above feed)
        assert any(p.grad.storage_offset() > 0 for _, p in named)
    hyper = {id(p): (g["lr"], g["weight_decay"]) for g in opt.param_groups for p in g["params"]}
    snap = [{"p": p.detach().clone(), "g": p.grad.clone(), "m": torch.zeros_like(p), "v": torch.zeros_like(p), "step": 0, "lr": hyper[id(p)][0], "wd": hyper[id(p)][1]} for _, p in named]
    eng = m._engine
    uploads = eng.weight_uploads
    assert uploads >= 1
    versions = [p._version for _, p in named]
    opt.step()
    torch.cuda.synchronize()
    assert all(p._version > v for (_, p), v in zip(named, versions))
    got = [(p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for _, p in named]
    _check_update(snap, got, float(opt.grad_norm), True, 5.0, f"t2_train_step, {len(named)} tensors, bucket_views={bucket_views}")
    for name, p in m.named_parameters():  # the engine's raw copies ARE the stepped parameters
        raw = torch.empty_like(p, dtype=torch.float32).contiguous()
        eng.read_weight(name, raw)
        assert torch.equal(raw, p.detach()), name
    sd = {k: v.detach().clone() for k, v in m.state_dict().items() if not k.endswith("image_positional_encoder.pe")}
    logits = _forward_backward(m, img, text)
    assert eng.weight_uploads == uploads  # neither the step nor the next training forward uploaded anything
    # a fresh model given the stepped state uploads the ordinary way and must compute the same bits
    _, fresh = engine_model(c["config"], c["max_seq_len"], c["wseed"])
    fresh.load_state_dict(sd, strict=False)
    want = _forward_backward(fresh, img, text)
    assert fresh._engine.weight_uploads >= 1
    assert torch.equal(logits, want)
    go = torch.full((c["B"], 1), 1, dtype=torch.long, device=DEV)
    outs = []
    for model in (m, fresh):
        model.eval()
        with torch.no_grad():
            outs.append(model(img, go, is_train=False)[0])
    assert torch.equal(outs[0], outs[1])
    # a second step keeps the engine in step as well (the mirrors are cached pointers)
    opt.step()
    logits2 = _forward_backward(m, img, text)
    assert eng.weight_uploads == uploads  # nor did the eval forward (it re-finalized from the raw copies) or the second step
    assert not torch.equal(logits2, logits)


# ---- 10. the raw ABI -------------------------------------------------------------------------------------------------
def test_raw_abi_refusals():
    lib = _lib.require_device()
    h = C.c_void_p()
    assert lib.d2t_optim_create(C.byref(h)) == 0
    try:
        assert lib.d2t_optim_chunk() == CH == _lib.OPTIM_CHUNK
        n = 8
        p, g, m, v = (torch.ones(n, device=DEV) for _ in range(4))
        norm = torch.zeros((), device=DEV)
        stream = _lib.stream_of(p)

        def rec(grad_ptr, numel=n):
            return _lib.D2TOptimTensor(p.data_ptr(), grad_ptr, m.data_ptr(), v.data_ptr(), None, numel,
                                       1e-3, 0.0, 0.9, 0.999, 1e-8, 0.1, 0.0316)

        def call(r, count, mgn=1.0, norm_ptr=None):
            arr = (_lib.D2TOptimTensor * 1)(r)
            rc = lib.d2t_optim_step(h, arr, count, 1, mgn, _lib.ptr(norm) if norm_ptr is None else norm_ptr, stream)
            return rc, lib.d2t_optim_last_error(h).decode()

        host = (C.c_float * n)()
        rc, msg = call(rec(C.addressof(host)), 1)
        assert rc == 1 and "grad" in msg and "device memory" in msg, (rc, msg)
        rc, msg = call(rec(g.data_ptr()), 1, norm_ptr=C.c_void_p(C.addressof(host)))
        assert rc == 1 and "norm" in msg, (rc, msg)
        rc, msg = call(rec(g.data_ptr()), -1)
        assert rc == 1 and "-1" in msg, (rc, msg)
        rc, msg = call(rec(g.data_ptr(), numel=-5), 1)
        assert rc == 1 and "negative" in msg, (rc, msg)
        torch.cuda.synchronize()
        assert torch.equal(p, torch.ones(n, device=DEV))  # nothing was launched by the refused calls
        rc, msg = call(rec(g.data_ptr()), 1)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert abs(float(norm) - n ** 0.5) <= 1e-6 and not torch.equal(p, torch.ones(n, device=DEV))
    finally:
        lib.d2t_optim_destroy(h)
    from doc2tex_amd.engine import Engine
    eng = Engine(synth.make_config("T2", device=DEV, max_seq_len=6))
    ptr, numel = C.c_void_p(), C.c_int64()
    rc = lib.d2t_weight_ptr(eng.ctx, b"no.such.tensor", C.byref(ptr), C.byref(numel))
    assert rc != 0 and "no.such.tensor" in lib.d2t_last_error(eng.ctx).decode()
    assert eng.weight_ptr("no.such.tensor") is None
