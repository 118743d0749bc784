"""The criteria of the reference's training step as fused HIP kernel pairs.

Mirrors doc2tex/modules/loss/builder.py and how engine/training.py:46-53,83,90,126 uses it:
`criterion = create_criterion(cfg["name"], criterion_kwargs(cfg)).to(device)`, then
`criterion(preds.view(-1, V), target.contiguous().view(-1))` followed by `.mean()`.  The three configurations that code accepts:

  * `name: 'entropy'` -> `CrossEntropyLoss(ignore_index, reduction)`: `d2t_ce_forward` / `d2t_ce_backward`, one pass over
    the logits each way instead of torch's log_softmax + nll_loss chain;
  * `name: 'entropy'` with `weight` and / or `loss_args: {label_smoothing: e}` -> `CrossEntropyLoss(weight=, label_smoothing=)`:
    `d2t_ce_smooth_forward` / `d2t_ce_smooth_backward` in torch mode (same values, gradients and reductions as
    nn.CrossEntropyLoss; 'mean' divides by the weights of the live rows' targets);
  * `name: 'smooth'` -> the reference's own `LabelSmoothingLoss` (modules/loss/labelsmoothing.py), quirks included: the same
    kernel pair in reference mode.  `create_criterion("smooth", ...)` does not route to it yet; construct
    `doc2tex_amd.loss.LabelSmoothingLoss` directly.

All take fp32 ROCm logits [rows, V] and int64 targets [rows].  Anything the fused kernels do not cover (non-fp32 or CPU
inputs, the legacy `size_average` / `reduce` flags) raises -- there is no eager fallback.
"""
import torch
import torch.nn as nn

from . import _lib

CE_TORCH, CE_REFERENCE = 0, 1  # include/d2t.h D2T_CE_TORCH / D2T_CE_REFERENCE


def _check_inputs(logits, target):
    if not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 2:
        raise RuntimeError("doc2tex_amd.loss: logits must be a [rows, V] float32 ROCm tensor (the engine has no CPU path)")
    if target.shape != logits.shape[:1]:
        raise ValueError(f"target shape {tuple(target.shape)} does not match logits {tuple(logits.shape)}")


class _FusedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        lib = _lib.require_device()
        _check_inputs(logits, target)
        logits = logits.contiguous()
        target = target.to(device=logits.device, dtype=torch.int64).contiguous()
        rows, V = logits.shape
        loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
        lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
        _lib.check(lib.d2t_ce_forward(_lib.ptr(logits), _lib.ptr(target), _lib.ptr(loss), _lib.ptr(lse), rows, V,
                                      int(ignore_index), _lib.stream_of(logits)), None, "ce_forward")
        ctx.save_for_backward(logits, target, lse)
        ctx.ignore_index = int(ignore_index)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse = ctx.saved_tensors
        lib = _lib.load()
        dloss = dloss.to(torch.float32).contiguous()
        dlogits = torch.empty_like(logits)
        rows, V = logits.shape
        _lib.check(lib.d2t_ce_backward(_lib.ptr(logits), _lib.ptr(target), _lib.ptr(lse), _lib.ptr(dloss), _lib.ptr(dlogits),
                                       rows, V, ctx.ignore_index, _lib.stream_of(logits)), None, "ce_backward")
        return dlogits, None, None


class _FusedSmoothCE(torch.autograd.Function):
    """Per-row loss of d2t_ce_smooth_forward: `on` of the mass on the target, `off` on every class of the mode's set
    (include/d2t.h), times the class weights in torch mode."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, on, off, mode, pad_index):
        lib = _lib.require_device()
        _check_inputs(logits, target)
        logits = logits.contiguous()
        target = target.to(device=logits.device, dtype=torch.int64).contiguous()
        rows, V = logits.shape
        if weight is not None:
            weight = weight.contiguous()
        loss, lse, mass = (torch.empty(rows, dtype=torch.float32, device=logits.device) for _ in range(3))
        ctx.args = (int(ignore_index), float(on), float(off), int(mode), int(pad_index))
        _lib.check(lib.d2t_ce_smooth_forward(_lib.ptr(logits), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(loss), _lib.ptr(lse),
                                             _lib.ptr(mass), rows, V, *ctx.args, _lib.stream_of(logits)), None, "ce_smooth_forward")
        ctx.save_for_backward(logits, target, lse, mass)
        ctx.weight = weight  # a buffer of the criterion, not a graph tensor
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse, mass = ctx.saved_tensors
        lib = _lib.load()
        dloss = dloss.to(torch.float32).contiguous()
        dlogits = torch.empty_like(logits)
        rows, V = logits.shape
        _lib.check(lib.d2t_ce_smooth_backward(_lib.ptr(logits), _lib.ptr(target), _lib.ptr(ctx.weight), _lib.ptr(lse),
                                              _lib.ptr(mass), _lib.ptr(dloss), _lib.ptr(dlogits), rows, V, *ctx.args,
                                              _lib.stream_of(logits)), None, "ce_smooth_backward")
        return (dlogits,) + (None,) * 7


class CrossEntropyLoss(nn.Module):
    """Drop-in for the `nn.CrossEntropyLoss(weight=..., ignore_index=..., reduction=..., label_smoothing=...)` the reference
    builds (modules/loss/builder.py:21): same arguments, same forward signature `criterion(input [rows, V], target [rows])`.
    `weight` is a buffer: `criterion.to(device)` moves it, as the trainer does (engine/training.py:53)."""

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
        super().__init__()
        if size_average is not None or reduce is not None:
            raise NotImplementedError("fused cross-entropy: the legacy reduction flags (size_average / reduce) are not supported")
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"{reduction} is not a valid value for reduction")
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"label_smoothing must be between 0.0 and 1.0. Got: {label_smoothing}")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).detach().clone()
            if weight.dim() != 1:
                raise ValueError(f"weight must be a vector of one entry per class, got shape {tuple(weight.shape)}")
        self.register_buffer("weight", weight)
        self.ignore_index, self.reduction, self.label_smoothing = int(ignore_index), reduction, float(label_smoothing)

    def forward(self, input, target):
        if self.weight is None and self.label_smoothing == 0.0:
            loss = _FusedCE.apply(input, target, self.ignore_index)
            if self.reduction == "none":
                return loss
            if self.reduction == "sum":
                return loss.sum()
            # torch's 'mean' divides by the number of non-ignored targets
            return loss.sum() / (target != self.ignore_index).sum().clamp(min=1).to(loss.dtype)
        V = input.shape[-1]
        w = self.weight
        if w is not None:
            if w.numel() != V:
                raise ValueError(f"weight has {w.numel()} entries, the logits have {V} classes")
            if w.dtype != torch.float32:
                raise TypeError(f"weight is {w.dtype}: the fused criterion reads float32 weights (criterion.double() / .half() converted the buffer)")
            if w.device != input.device:
                raise RuntimeError(f"weight is on {w.device}, the logits on {input.device}: move the criterion with .to(device)")
        e = self.label_smoothing
        loss = _FusedSmoothCE.apply(input, target, w, self.ignore_index, 1.0 - e, e / V, CE_TORCH, -1)
        if self.reduction == "none":
            return loss
        if self.reduction == "sum":
            return loss.sum()
        # torch's 'mean' divides by the weights of the live rows' targets.  No live row -> 0, decided by their COUNT: a
        # weight sum may legitimately lie far below 1.
        target = target.to(input.device)
        live = (target != self.ignore_index) & (target >= 0) & (target < V)
        count = live.sum()
        denom = count.to(loss.dtype) if w is None else (w[target.clamp(0, V - 1)] * live).sum()
        return torch.where(count > 0, loss.sum() / torch.where(count > 0, denom, torch.ones_like(denom)), torch.zeros_like(denom))


class LabelSmoothingLoss(nn.Module):
    """The reference's LabelSmoothingLoss (modules/loss/labelsmoothing.py) on the fused kernel pair: same constructor, same
    attributes, same values and gradients.  The target's class gets `confidence = 1 - smoothing`, every other class but the
    padding column `smoothing / (classes - 2)`; rows whose target is `ignore_index` give 0.  The reference's quirks are kept:

      * a truthy `reduction` (ANY non-empty string, 'mean' included) returns the per-row losses; a falsy one (None, '')
        their mean over ALL rows, ignored ones included;
      * `classes` only enters the denominator and need not be the width of the logits;
      * `classes == 2` raises ZeroDivisionError, an `ignore_index` outside [0, V) IndexError, both at the call."""

    def __init__(self, reduction, classes, ignore_index, smoothing=0.0, dim=-1):
        super().__init__()
        self.confidence = 1.0 - smoothing
        self.smoothing = smoothing
        self.cls = classes
        self.dim = dim
        self.padding_idx = ignore_index
        self.reduction = reduction

    def forward(self, pred, target):
        if self.dim not in (-1, 1):
            raise NotImplementedError(f"LabelSmoothingLoss: dim={self.dim}; the fused criterion reduces the class dimension of [rows, V] logits")
        off = self.smoothing / (self.cls - 2)
        V = pred.shape[-1]
        if not 0 <= self.padding_idx < V:
            raise IndexError(f"index {self.padding_idx} is out of bounds for dimension 1 with size {V}")
        loss = _FusedSmoothCE.apply(pred, target, None, self.padding_idx, self.confidence, off, CE_REFERENCE, self.padding_idx)
        if not self.reduction:
            return torch.mean(loss)
        return loss


def criterion_kwargs(cfg):
    """modules/loss/builder.py:6-15: the `criterion` section of a training configuration -> constructor arguments
    (`ignore_index` and `reduction` always, `weight` if given, then whatever `loss_args` holds)."""
    kwargs = {"ignore_index": cfg["ignore_index"], "reduction": cfg["reduction"]}
    weight = cfg.get("weight")
    if weight is not None:
        kwargs["weight"] = weight
    kwargs.update(cfg.get("loss_args") or {})
    return kwargs


def create_criterion(loss, loss_kwargs):
    """modules/loss/builder.py:18-24 with the fused kernels behind "entropy" (weight / label_smoothing included)."""
    if loss == "entropy":
        return CrossEntropyLoss(**loss_kwargs)
    if loss == "smooth":
        raise NotImplementedError("criterion 'smooth' is not routed by name yet: construct doc2tex_amd.loss.LabelSmoothingLoss(**kwargs) "
                                  "directly (same constructor as the reference's class)")
    raise NotImplementedError(f"criterion '{loss}' is not on the accelerated path (the shipped configs use 'entropy')")
