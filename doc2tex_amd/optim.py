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

The builder's other optimizers are fused on the same pattern (csrc/optim_family.hip): `FusedLamb`, `FusedAdamP`,
`FusedMADGRAD` and the `Lookahead` wrapper, with the reference classes' arguments, groups and state keys, so a
`state_dict()` moves to and from those too.  `build_optimizer` is the reference's builder in full and returns them for
`opt: 'lamb' | 'adamp' | 'madgrad'` and behind the `lookahead_` prefix; `create_optimizer` serves the four names it served
before and names `build_optimizer` when it refuses the rest.  `_FusedBase.step` is what all of them do around the launch.
"""
import ctypes as C
from collections import defaultdict

import torch

from . import _lib

CHUNK = _lib.OPTIM_CHUNK  # elements per block of the kernels (include/d2t.h D2T_OPTIM_CHUNK)


class _OptimHandle:
    """Owner of a d2t_optim (include/d2t.h): the staging buffers and scratch of the optimizer kernels on one device."""
    _label = "fused optimizer"
    _handle = None  # (device index, d2t_optim*)

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
                raise RuntimeError(f"{self._label}: parameters moved from cuda:{self._handle[0]} to cuda:{device}; build a new optimizer")
            lib = _lib.require_device()
            h = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(lib.d2t_optim_create(C.byref(h)), None, "optim_create")
            self._handle = (device, h)
        return self._handle[1]

    def _call(self, fn, device, arr, *args):
        """fn(handle, records, count, *args, stream) on the current stream of `device`; raises with the library's message."""
        h = self._optim(device)
        lib = _lib.load()
        stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda", device)).cuda_stream)
        rc = getattr(lib, fn)(h, arr, len(arr), *args, stream)
        if rc != _lib.D2T_OK:
            raise RuntimeError(f"libd2t {fn[4:]} failed (code {rc}) {lib.d2t_optim_last_error(h).decode()}")

    def _checked_param(self, p, device):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError(f"{self._label}: parameters must be contiguous float32 ROCm tensors (there is no CPU or "
                               f"eager path); got {p.dtype} on {p.device}")
        if device is not None and p.device.index != device:
            raise RuntimeError(f"{self._label}: all parameters of one optimizer must live on one device")

    def _state_tensors(self, state, p, names, keep):
        out = []
        for what in names:
            t = state[what]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous() \
                    or t.numel() != p.numel():
                raise RuntimeError(f"{self._label}: state '{what}' must be a contiguous float32 tensor like its parameter")
            out.append(t)
        keep += out
        return out


class _FusedBase(_OptimHandle, torch.optim.Optimizer):
    """What every fused optimizer does around its launch: collects one record per parameter that has a gradient, refuses
    what the kernels cannot take (there is no eager path), finds the engine's raw copies of the attached model's weights,
    and afterwards tells autograd and the engine what was written behind their backs.  A subclass gives `_label`,
    `_group_scalars`, `_record` and `_launch`."""
    def _attach(self, model, max_grad_norm=None):
        self.max_grad_norm = max_grad_norm
        self.model = model
        self.grad_norm = None  # device scalar: the norm of the last step's gradients before clipping
        self._mirror_key, self._mirrors = None, {}

    def _engine_mirrors(self):
        """(engine, {id(parameter): (state_dict key, pointer of the engine's raw copy)}) for the attached model, or (None, {})."""
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

    def _checked_grad(self, p, keep, device):
        """The contiguous fp32 gradient of `p` on its device (a copy goes to `keep`), after every refusal."""
        g = p.grad
        self._checked_param(p, device)
        if g.is_sparse:
            raise RuntimeError(f"{self._label} does not support sparse gradients")
        if g.dtype != torch.float32 or g.device != p.device:
            raise RuntimeError(f"{self._label}: gradient is {g.dtype} on {g.device}, its parameter float32 on {p.device}")
        if not g.is_contiguous():
            g = g.contiguous()
            keep.append(g)
        return g

    def _clip(self, device):
        """(max_grad_norm for the kernels, the device scalar that receives the norm or None)."""
        clip = self.max_grad_norm is not None and float(self.max_grad_norm) > 0.0
        norm = torch.empty((), dtype=torch.float32, device=torch.device("cuda", device)) if clip else None
        return (float(self.max_grad_norm) if clip else 0.0), norm

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        eng, mirrors = self._engine_mirrors()
        recs, keep, params, mirrored = [], [], [], []
        device = None
        self._counts = []  # (group or state, its new "step"): these counts move only once nothing can refuse the step any more
        for group in self.param_groups:
            scalars = self._group_scalars(group)
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = self._checked_grad(p, keep, device)
                device = p.device.index
                mir = mirrors.get(id(p))
                if mir is not None:
                    mirrored.append(mir[0])
                recs.append(self._record(group, scalars, p, g, mir[1] if mir else None, keep))
                params.append(p)
        if recs:
            self._launch(device, recs, params)
        for holder, count in self._counts:
            holder["step"] = count
        if not recs:
            return loss
        torch.autograd.graph.increment_version(params)  # written behind autograd's back
        torch.autograd.graph.increment_version(keep)
        if eng is not None and eng.device == device and mirrored:
            # the engine's raw copies of these tensors are the new values already: nothing to upload for them
            eng.weights_current(self.model, mirrored)
        return loss


class _FusedAdamBase(_FusedBase):
    _decoupled = False
    _label = "fused Adam"

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
        self._attach(model, max_grad_norm)

    def _group_scalars(self, group):
        for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
            if group.get(flag):
                raise NotImplementedError(f"fused Adam: {flag}=True is not on the accelerated path")
        if bool(group.get("decoupled_weight_decay", self._decoupled)) != self._decoupled:
            raise NotImplementedError(f"{type(self).__name__}: a group with decoupled_weight_decay="
                                      f"{group['decoupled_weight_decay']} belongs to the other class")
        beta1, beta2 = (float(b) for b in group["betas"])
        return float(group["lr"]), float(group["weight_decay"]), float(group["eps"]), beta1, beta2

    def _record(self, group, scalars, p, g, mirror, keep):
        lr, wd, eps, beta1, beta2 = scalars
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        m, v = self._state_tensors(state, p, ("exp_avg", "exp_avg_sq"), keep)
        state["step"] += 1
        t = float(state["step"])
        return (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), mirror, p.numel(),
                lr, wd, beta1, beta2, eps, 1.0 - beta1 ** t, (1.0 - beta2 ** t) ** 0.5)

    def _launch(self, device, recs, params):
        mgn, norm = self._clip(device)
        arr = (_lib.D2TOptimTensor * len(recs))(*recs)
        self._call("d2t_optim_step", device, arr, int(self._decoupled), mgn, _lib.ptr(norm))
        self.grad_norm = norm


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


class FusedLamb(_FusedBase):
    """The reference's Lamb (optim/lamb.py: the NvLamb variant) on the fused kernels, four launches per step; the reference's
    arguments, groups and state (`exp_avg`, `exp_avg_sq`, the step count in `group["step"]`).  `max_grad_norm` is LAMB's own
    clip, read from `defaults` as in the reference: the gradients are divided by norm / max_grad_norm where the global norm
    exceeds it (no 1e-6).  A caller who keeps `clip_grad_norm_(params, 5.0)` in front gets both: gradients of norm at most
    5, then LAMB's division down to `max_grad_norm` -- with the default 1.0 the first clip changes nothing but the bits.
    `optimizer.grad_norm` is the norm before LAMB's clip.  `.grad` is only read (the reference divides it in place)."""
    _label = "fused Lamb"

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01,
                 grad_averaging=True, max_grad_norm=1.0, trust_clip=False, always_adapt=False, model=None):
        defaults = dict(lr=lr, bias_correction=bias_correction, betas=betas, eps=eps, weight_decay=weight_decay,
                        grad_averaging=grad_averaging, max_grad_norm=max_grad_norm, trust_clip=trust_clip, always_adapt=always_adapt)
        super().__init__(params, defaults)
        self._attach(model)

    def _group_scalars(self, group):
        beta1, beta2 = (float(b) for b in group["betas"])
        t = group["step"] + 1 if "step" in group else 1  # one count per group, as in the reference, gradients or not
        self._counts.append((group, t))
        bc1, sbc2 = (1.0 - beta1 ** t, (1.0 - beta2 ** t) ** 0.5) if group["bias_correction"] else (1.0, 1.0)
        wd = float(group["weight_decay"])
        return (float(group["lr"]), wd, beta1, beta2, 1.0 - beta1 if group["grad_averaging"] else 1.0, float(group["eps"]), bc1, sbc2,
                int(wd != 0 or bool(group["always_adapt"])), int(bool(group["trust_clip"])))

    def _record(self, group, scalars, p, g, mirror, keep):
        state = self.state[p]
        if len(state) == 0:
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        m, v = self._state_tensors(state, p, ("exp_avg", "exp_avg_sq"), keep)
        return (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), mirror, p.numel()) + scalars

    def _launch(self, device, recs, params):
        norm = torch.empty((), dtype=torch.float32, device=torch.device("cuda", device))
        arr = (_lib.D2TOptimLambTensor * len(recs))(*recs)
        self._call("d2t_optim_lamb_step", device, arr, float(self.defaults["max_grad_norm"]), _lib.ptr(norm))
        self.grad_norm = norm


class FusedAdamP(_FusedBase):
    """The reference's AdamP (optim/adamp.py) on the fused kernels, three launches per step (five with `max_grad_norm`, the
    global-norm clip of FusedAdam); the reference's arguments, groups and state (`step` an int, `exp_avg`, `exp_avg_sq`).
    Whether a tensor is projected per row, as a whole or not at all is decided on the device: `step()` reads nothing back,
    and `projection_modes()` has the decisions of the last step."""
    _label = "fused AdamP"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, delta=0.1, wd_ratio=0.1, nesterov=False,
                 max_grad_norm=None, model=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, delta=delta, wd_ratio=wd_ratio, nesterov=nesterov)
        super().__init__(params, defaults)
        self._attach(model, max_grad_norm)
        self._modes = self._next_modes = None

    def projection_modes(self):
        """Device int32 tensor, one entry per parameter in the order of the groups: what the last step did with it -- 0 no
        projection (also: one dimension, no gradient), 1 channel (per row of reshape(size(0), -1)), 2 layer.  None before
        the first step."""
        return self._modes

    def step(self, closure=None):
        self._slot = {id(p): i for i, p in enumerate(p for group in self.param_groups for p in group["params"])}
        self._next_modes = None
        return super().step(closure)

    def _group_scalars(self, group):
        beta1, beta2 = (float(b) for b in group["betas"])
        return (float(group["lr"]), float(group["weight_decay"]), beta1, beta2, float(group["eps"]), float(group["delta"]),
                float(group["wd_ratio"]), int(bool(group["nesterov"])))

    def _record(self, group, scalars, p, g, mirror, keep):
        lr, wd, beta1, beta2, eps, delta, wd_ratio, nesterov = scalars
        state = self.state[p]
        if len(state) == 0:
            state["step"] = 0
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        m, v = self._state_tensors(state, p, ("exp_avg", "exp_avg_sq"), keep)
        t = int(state["step"]) + 1
        self._counts.append((state, t))
        if self._next_modes is None:
            self._next_modes = torch.zeros(len(self._slot), dtype=torch.int32, device=p.device)
        mode = self._next_modes.data_ptr() + 4 * self._slot[id(p)]
        return (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), mirror, mode, p.numel(), p.size(0) if p.dim() > 1 else 0,
                lr, wd, beta1, beta2, eps, 1.0 - beta1 ** t, (1.0 - beta2 ** t) ** 0.5, delta, wd_ratio, nesterov, 0)

    def _launch(self, device, recs, params):
        mgn, norm = self._clip(device)
        arr = (_lib.D2TOptimAdampTensor * len(recs))(*recs)
        self._call("d2t_optim_adamp_step", device, arr, mgn, _lib.ptr(norm))
        self.grad_norm, self._modes = norm, self._next_modes


class FusedMADGRAD(_FusedBase):
    """The reference's MADGRAD (optim/madgrad.py, dense gradients) on the fused kernels, one launch per step (three with
    `max_grad_norm`, the global-norm clip of FusedAdam); the reference's arguments, groups and state (`step` an int,
    `grad_sum_sq`, `s`, and `x0` where momentum != 0).  `.grad` is only read (the reference's coupled decay adds to it)."""
    _label = "fused MADGRAD"

    def __init__(self, params, lr=1e-2, momentum=0.9, weight_decay=0, eps=1e-6, decoupled_decay=False, max_grad_norm=None,
                 model=None):
        if momentum < 0 or momentum >= 1:
            raise ValueError(f"Momentum {momentum} must be in the range [0,1]")
        if lr <= 0:
            raise ValueError(f"Learning rate {lr} must be positive")
        if weight_decay < 0:
            raise ValueError(f"Weight decay {weight_decay} must be non-negative")
        if eps < 0:
            raise ValueError("Eps must be non-negative")
        defaults = dict(lr=lr, eps=eps, momentum=momentum, weight_decay=weight_decay, decoupled_decay=decoupled_decay)
        super().__init__(params, defaults)
        self._attach(model, max_grad_norm)

    def _group_scalars(self, group):
        return (float(group["lr"]), float(group["weight_decay"]), float(group["momentum"]), float(group["eps"]),
                int(bool(group["decoupled_decay"])))

    def _record(self, group, scalars, p, g, mirror, keep):
        lr, wd, momentum, eps, decoupled = scalars
        state = self.state[p]
        if len(state) == 0:
            state["step"] = 0
            state["grad_sum_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state["s"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if momentum != 0:
                state["x0"] = torch.clone(p, memory_format=torch.contiguous_format).detach()
        names = ("grad_sum_sq", "s", "x0") if momentum != 0 else ("grad_sum_sq", "s")
        tensors = self._state_tensors(state, p, names, keep)
        t = int(state["step"]) + 1
        self._counts.append((state, t))
        lamb = (lr + eps) * float(t) ** 0.5
        return (p.data_ptr(), g.data_ptr(), tensors[0].data_ptr(), tensors[1].data_ptr(),
                tensors[2].data_ptr() if momentum != 0 else None, mirror, p.numel(), lr, wd, momentum, eps, lamb, decoupled, 0)

    def _launch(self, device, recs, params):
        mgn, norm = self._clip(device)
        arr = (_lib.D2TOptimMadgradTensor * len(recs))(*recs)
        self._call("d2t_optim_madgrad_step", device, arr, mgn, _lib.ptr(norm))
        self.grad_norm = norm


class Lookahead(_OptimHandle, torch.optim.Optimizer):
    """The reference's Lookahead wrapper (optim/lookahead.py) around any optimizer whose parameters are contiguous float32
    ROCm tensors: every `k` steps of the base, slow += alpha (fast - slow) and fast = slow in one launch for all groups that
    are due.  The slow weights live in the base optimizer's state (`lookahead_slow_buff`) and `lookahead_alpha/k/step` in
    its groups, so `state_dict()` is the base's.  A slow buffer is created as a copy of its fast weights at the first
    synchronisation, which therefore changes nothing.  Around a fused optimizer with a model attached the engine's raw
    copies are written in the same pass.  As in the reference, Optimizer.__init__ is not called."""
    _label = "Lookahead"

    def __init__(self, base_optimizer, alpha=0.5, k=6):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        defaults = dict(lookahead_alpha=alpha, lookahead_k=k, lookahead_step=0)
        self._base_optimizer = base_optimizer
        self.param_groups = base_optimizer.param_groups
        self.defaults = base_optimizer.defaults
        self.defaults.update(defaults)
        self.state = defaultdict(dict)
        for name, default in defaults.items():
            for group in self._base_optimizer.param_groups:
                group.setdefault(name, default)

    @torch.no_grad()
    def _sync(self, groups):
        base = self._base_optimizer
        fused = isinstance(base, _FusedBase) and base.model is not None
        eng, mirrors = base._engine_mirrors() if fused else (None, {})
        device = None
        by_alpha = {}  # alpha -> records: one launch per distinct alpha (one, unless the groups were edited)
        written, mirrored = [], []
        for group in groups:
            recs = by_alpha.setdefault(float(group["lookahead_alpha"]), [])
            for fast in group["params"]:
                if fast.grad is None:
                    continue
                self._checked_param(fast, device)
                device = fast.device.index
                state = base.state[fast]
                if "lookahead_slow_buff" not in state:
                    state["lookahead_slow_buff"] = fast.detach().clone(memory_format=torch.contiguous_format)
                slow, = self._state_tensors(state, fast, ("lookahead_slow_buff",), written)
                mir = mirrors.get(id(fast))
                if mir is not None:
                    mirrored.append(mir[0])
                recs.append((fast.data_ptr(), slow.data_ptr(), mir[1] if mir else None, fast.numel()))
                written.append(fast)
        for alpha, recs in by_alpha.items():
            if recs:
                self._call("d2t_optim_lookahead_sync", device, (_lib.D2TOptimLookaheadTensor * len(recs))(*recs), alpha)
        if written:
            torch.autograd.graph.increment_version(written)
        if eng is not None and eng.device == device and mirrored:
            eng.weights_current(base.model, mirrored)

    def update_slow(self, group):
        self._sync([group])

    def sync_lookahead(self):
        self._sync(self._base_optimizer.param_groups)

    @torch.no_grad()
    def step(self, closure=None):
        loss = self._base_optimizer.step(closure)
        due = []
        for group in self._base_optimizer.param_groups:
            group["lookahead_step"] += 1
            if group["lookahead_step"] % group["lookahead_k"] == 0:
                due.append(group)
        if due:
            self._sync(due)
        return loss

    def zero_grad(self, set_to_none=True):
        self._base_optimizer.zero_grad(set_to_none=set_to_none)

    def state_dict(self):
        return self._base_optimizer.state_dict()

    def load_state_dict(self, state_dict):
        self._base_optimizer.load_state_dict(state_dict)
        self.param_groups = self._base_optimizer.param_groups


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


def build_optimizer(model, opt, lr, weight_decay, momentum, filter_bias_and_bn, layer_decay=1.0, train_mode="scratch", **kwargs):
    """modules/optim/builder.py:48-96 in full: 'adam' / 'adamw' / 'adamp' / 'lamb' / 'madgrad' give the fused classes with
    the model attached, 'adadelta' / 'adagrad' torch's, and a 'lookahead_' prefix wraps any of them in Lookahead.
    `max_grad_norm` (the configuration's `grad_clip`) may be passed through `kwargs`: the global-norm clip of the fused
    Adam, AdamP and MADGRAD steps, LAMB's own clip for 'lamb'; torch's optimizers do not clip, and the caller keeps its
    clip_grad_norm_ call.  `layer_decay` and `train_mode` are accepted and, as in the reference, unused."""
    if weight_decay and filter_bias_and_bn:
        skip = model.no_weight_decay() if hasattr(model, "no_weight_decay") else ()
        parameters = add_weight_decay(model, weight_decay, skip)
        weight_decay = 0.0
    else:
        parameters = model.parameters()
    parts = opt.lower().split("_")
    name = parts[-1]
    args = dict(weight_decay=weight_decay, **kwargs)
    if lr is not None:
        args.setdefault("lr", lr)
    if name in ("adam", "adamw"):
        optimizer = (FusedAdam if name == "adam" else FusedAdamW)(parameters, model=model, **args)
    elif name == "adamp":
        optimizer = FusedAdamP(parameters, wd_ratio=0.01, nesterov=True, model=model, **args)
    elif name == "lamb":
        optimizer = FusedLamb(parameters, model=model, **args)
    elif name == "madgrad":
        optimizer = FusedMADGRAD(parameters, momentum=momentum, model=model, **args)
    else:
        args.pop("max_grad_norm", None)
        if name == "adadelta":
            optimizer = torch.optim.Adadelta(parameters, **args)
        elif name == "adagrad":
            args.setdefault("eps", 1e-8)
            optimizer = torch.optim.Adagrad(parameters, **args)
        else:
            raise NotImplementedError(f"optimizer '{opt}' is not one the reference's builder knows")
    if len(parts) > 1 and parts[0] == "lookahead":
        optimizer = Lookahead(optimizer)
    return optimizer


_NOT_PORTED = ("adamp", "lamb", "madgrad")


def create_optimizer(model, opt, lr, weight_decay, momentum, filter_bias_and_bn, layer_decay=1.0, train_mode="scratch",
                     **kwargs):
    """build_optimizer for the names served before the optimizer family was fused: 'adam' / 'adamw' / 'adadelta' /
    'adagrad'.  It keeps refusing 'adamp', 'lamb', 'madgrad' and the 'lookahead_' prefix; the messages
    name build_optimizer, which takes them."""
    parts = opt.lower().split("_")
    if len(parts) > 1 and parts[0] == "lookahead":
        raise NotImplementedError(f"optimizer '{opt}': create_optimizer does not wrap in lookahead_; "
                                  "doc2tex_amd.optim.build_optimizer takes the same arguments and does (Lookahead)")
    if parts[-1] in _NOT_PORTED:
        raise NotImplementedError(f"optimizer '{parts[-1]}': create_optimizer does not serve it; "
                                  "doc2tex_amd.optim.build_optimizer takes the same arguments and does (fused kernels)")
    return build_optimizer(model, opt, lr, weight_decay, momentum, filter_bias_and_bn, layer_decay, train_mode, **kwargs)
