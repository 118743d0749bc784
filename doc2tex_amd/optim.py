"""The optimizer of the reference's training step as fused HIP kernels, and its optimizer builder.

Mirrors doc2tex/modules/optim/builder.py and how engine/training.py:94-164 uses it:
`optimizer = create_optimizer(model, filter_bias_and_bn=..., **optimizer_kwargs(cfg))`, then per step
`clip_grad_norm_(model.parameters(), grad_clip)` and `optimizer.step()`.  Here `opt: 'adam'` / `'adamw'` give `FusedAdam` /
`FusedAdamW`: `d2t_optim_step` (include/d2t.h) computes the global gradient norm, applies the clip coefficient on the fly,
takes the Adam step in torch's order of operations and writes every new parameter twice -- into the module's tensor and into
the engine's raw copy of it -- in at most three launches, with no host synchronisation.  The next training forward then
uploads nothing.

    optimizer = create_optimizer(model, filter_bias_and_bn=True, max_grad_norm=cfg["grad_clip"], **optimizer_kwargs(cfg))
    loss.backward()
    optimizer.step()            # no clip_grad_norm_ call: optimizer.grad_norm is what it would have returned

Differences from `clip_grad_norm_` + `torch.optim.AdamW`, all deliberate:
  * `.grad` is left UNCLIPPED (the coefficient is applied inside the update; the gradients are only read);
  * `amsgrad`, `maximize`, `capturable`, `differentiable`, sparse gradients and parameters that are not contiguous fp32 ROCm
    tensors raise at `step()` -- there is no eager fallback.
State (`step`, `exp_avg`, `exp_avg_sq`) and `state_dict()` are torch's, so checkpoints move between the two freely.
"""
import ctypes as C

import torch

from . import _lib

CHUNK = _lib.OPTIM_CHUNK  # elements per block of the kernels (include/d2t.h D2T_OPTIM_CHUNK)


class _FusedAdamBase(torch.optim.Optimizer):
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, model=None,
                 amsgrad=False, maximize=False):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("fused Adam: a tensor lr is not supported (pass a float; schedulers set floats)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad or maximize:
            raise NotImplementedError("fused Adam: amsgrad / maximize are not on the accelerated path")
        # the same keys as torch.optim.Adam's groups, so that a state_dict moves either way
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=self._decoupled)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.model = model
        self.grad_norm = None  # device scalar: the norm of the last step's gradients before clipping
        self._handle = None    # (device index, d2t_optim*)
        self._mirror_key, self._mirrors = None, {}

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            try:
                with torch.cuda.device(h[0]):
                    _lib.load().d2t_optim_destroy(h[1])
            except Exception:
                pass

    def _optim(self, device):
        if self._handle is None or self._handle[0] != device:
            if self._handle is not None:
                raise RuntimeError(f"fused Adam: parameters moved from cuda:{self._handle[0]} to cuda:{device}; build a new optimizer")
            lib = _lib.require_device()
            h = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(lib.d2t_optim_create(C.byref(h)), None, "optim_create")
            self._handle = (device, h)
        return self._handle[1]

    def _engine_mirrors(self):
        """{id(parameter): (state_dict key, pointer of the engine's raw copy)} for the attached model, or {}."""
        eng = getattr(self.model, "_engine", None) if self.model is not None else None
        if eng is None or eng._sig is None:
            return None, {}
        key = eng._load_epoch  # an object of that engine's, held here: no other engine or later load can pass for it
        if key is not self._mirror_key:
            self._mirrors = {}
            for name, p in self.model.named_parameters():
                got = eng.weight_ptr(name)
                if got is not None and got[1] == p.numel():
                    self._mirrors[id(p)] = (name, got[0])
            self._mirror_key = key
        return eng, self._mirrors

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        eng, mirrors = self._engine_mirrors()
        recs, keep, params, mirrored = [], [], [], []
        device = None
        for group in self.param_groups:
            for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(flag):
                    raise NotImplementedError(f"fused Adam: {flag}=True is not on the accelerated path")
            if bool(group.get("decoupled_weight_decay", self._decoupled)) != self._decoupled:
                raise NotImplementedError(f"{type(self).__name__}: a group with decoupled_weight_decay="
                                          f"{group['decoupled_weight_decay']} belongs to the other class")
            lr, wd, eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
            beta1, beta2 = (float(b) for b in group["betas"])
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("fused Adam: parameters must be contiguous float32 ROCm tensors (there is no CPU or "
                                       f"eager path); got {p.dtype} on {p.device}")
                if g.is_sparse:
                    raise RuntimeError("fused Adam does not support sparse gradients")
                if g.dtype != torch.float32 or g.device != p.device:
                    raise RuntimeError(f"fused Adam: gradient is {g.dtype} on {g.device}, its parameter float32 on {p.device}")
                if device is None:
                    device = p.device.index
                elif p.device.index != device:
                    raise RuntimeError("fused Adam: all parameters of one optimizer must live on one device")
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                for what, t in (("exp_avg", m), ("exp_avg_sq", v)):
                    if t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous() or t.numel() != p.numel():
                        raise RuntimeError(f"fused Adam: state '{what}' must be a contiguous float32 tensor like its parameter")
                state["step"] += 1
                t = float(state["step"])
                mir = mirrors.get(id(p))
                if mir is not None:
                    mirrored.append(mir[0])
                recs.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), mir[1] if mir else None, p.numel(),
                             lr, wd, beta1, beta2, eps, 1.0 - beta1 ** t, (1.0 - beta2 ** t) ** 0.5))
                params.append(p)
                keep += [m, v]
        if not recs:
            return loss
        clip = self.max_grad_norm is not None and float(self.max_grad_norm) > 0.0
        dev = torch.device("cuda", device)
        norm = torch.empty((), dtype=torch.float32, device=dev) if clip else None
        arr = (_lib.D2TOptimTensor * len(recs))(*recs)
        h = self._optim(device)
        lib = _lib.load()
        rc = lib.d2t_optim_step(h, arr, len(recs), int(self._decoupled), float(self.max_grad_norm) if clip else 0.0,
                                _lib.ptr(norm), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != _lib.D2T_OK:
            raise RuntimeError(f"libd2t optim_step failed (code {rc}) {lib.d2t_optim_last_error(h).decode()}")
        self.grad_norm = norm
        torch.autograd.graph.increment_version(params)  # written behind autograd's back
        torch.autograd.graph.increment_version(keep)
        if eng is not None and eng.device == device and mirrored:
            # the engine's raw copies of these tensors are the new values already: nothing to upload for them
            eng.weights_current(self.model, mirrored)
        return loss


class FusedAdamW(_FusedAdamBase):
    """torch.optim.AdamW (decoupled weight decay) on the fused kernels; `max_grad_norm` replaces the separate
    clip_grad_norm_ call, `model` (a doc2tex_amd.Model) lets the step refresh the engine's weights in the same pass."""
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, model=None,
                 amsgrad=False, maximize=False):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, model, amsgrad, maximize)


class FusedAdam(_FusedAdamBase):
    """torch.optim.Adam (weight decay added to the gradient) on the fused kernels; see FusedAdamW."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, model=None,
                 amsgrad=False, maximize=False):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, model, amsgrad, maximize)


def add_weight_decay(model, weight_decay=1e-5, skip_list=()):
    """modules/optim/builder.py:13-26: two groups -- every trainable tensor that is 1-D, named '*.bias' or listed in
    `skip_list` without decay, the rest with `weight_decay`."""
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if p.dim() == 1 or name.endswith(".bias") or name in skip_list else decay).append(p)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


def optimizer_kwargs(cfg):
    """modules/optim/builder.py:29-45: the optimizer keys of a training configuration -> create_optimizer arguments."""
    kwargs = {"opt": cfg["opt"], "lr": cfg["lr"], "weight_decay": cfg["weight_decay"], "momentum": cfg["momentum"]}
    if cfg.get("opt_eps") is not None:
        kwargs["eps"] = cfg["opt_eps"]
    if cfg.get("opt_betas") is not None:
        kwargs["betas"] = cfg["opt_betas"]
    if cfg.get("opt_args") is not None:
        kwargs.update(cfg["opt_args"])
    return kwargs


_NOT_PORTED = ("adamp", "lamb", "madgrad")


def create_optimizer(model, opt, lr, weight_decay, momentum, filter_bias_and_bn, layer_decay=1.0, train_mode="scratch",
                     **kwargs):
    """modules/optim/builder.py:48-96 with the fused kernels behind 'adam' / 'adamw'.  `max_grad_norm` (the configuration's
    `grad_clip`) may be passed through `kwargs` for those two; `momentum`, `layer_decay` and `train_mode` are accepted and,
    as in the reference, unused by the optimizers served here."""
    if weight_decay and filter_bias_and_bn:
        skip = model.no_weight_decay() if hasattr(model, "no_weight_decay") else ()
        parameters = add_weight_decay(model, weight_decay, skip)
        weight_decay = 0.0
    else:
        parameters = model.parameters()
    parts = opt.lower().split("_")
    name = parts[-1]
    if len(parts) > 1 and parts[0] == "lookahead":
        raise NotImplementedError(f"optimizer '{opt}': the lookahead_ wrapper is not on the accelerated path")
    if name in _NOT_PORTED:
        raise NotImplementedError(f"optimizer '{name}' is not on the accelerated path (the shipped configuration uses 'adamw')")
    args = dict(weight_decay=weight_decay, **kwargs)
    if lr is not None:
        args.setdefault("lr", lr)
    if name in ("adam", "adamw"):
        return (FusedAdam if name == "adam" else FusedAdamW)(parameters, model=model, **args)
    args.pop("max_grad_norm", None)  # torch's optimizers do not clip: the caller keeps its clip_grad_norm_ call
    if name == "adadelta":
        return torch.optim.Adadelta(parameters, **args)
    if name == "adagrad":
        args.setdefault("eps", 1e-8)
        return torch.optim.Adagrad(parameters, **args)
    raise NotImplementedError(f"optimizer '{opt}' is not one the reference's builder knows")
