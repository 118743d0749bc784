"""Training-mode forward/backward of `Model` as one autograd node.

The reference trains through PyTorch autograd (`loss.backward()`, engine/training.py:137) on the logits that
`model(image, text[:, :-1])` returns (`forward_step`, training.py:76-91).  Here the whole network is one
`torch.autograd.Function`: forward = `d2t_train_forward` (BatchNorm on batch statistics, teacher-forced decoder),
backward = `d2t_train_backward` on dL/dlogits, after which every parameter's gradient is copied out of the engine.
The caller's criterion, `clip_grad_norm_` and optimizer run unchanged (torch's, or the fused ones of doc2tex_amd.loss and
doc2tex_amd.optim).
"""
import torch


class _TrainStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, image, text, names, *params):
        # the LSTM-attention head reads the engine's derived (transposed / folded) decoder weights, so it needs the
        # finalize pass, and so does a BiLSTM encoder (its packed input projections); the TFM head reads the raw copies only
        eng = model.engine(finalize=model.stages["Pred"] != "TFM" or model.stages["Seq"] == "BiLSTM")
        # dropout (nn.TransformerDecoderLayer(dropout=p) / the LSTM head's droprate on its generator output): masks from
        # the engine's Philox stream, seeded like torch's generator
        pp = model.opt["Prediction"]["params"]
        tfm = model.stages["Pred"] == "TFM"
        p = float(pp.get("dropout" if tfm else "droprate", 0.0) or 0.0)
        eng.set_dropout(p, torch.initial_seed())
        if not tfm:
            # scheduled sampling (seq2seq.py:311-316): one random.random() per step but the last, drawn exactly as the
            # reference draws them, so seeding `random` reproduces its choices
            import random
            tf = float(pp.get("teacher_forcing", 1.0))
            flags = [1] + [0 if tf < random.random() else 1 for _ in range(text.shape[1] - 1)]
            eng.set_teacher_flags(None if all(flags) else flags)
        logits = eng.train_forward(image, text)
        pred = model.predicter.Prediction
        if not tfm and getattr(pred, "viz_attn", False):
            # alpha_stores (seq2seq.py:267-272,300-301) from the alignments the step saved for its backward pass.  Unlike the
            # reference's, this tensor is detached: no gradient flows through it
            B, _, H, W = image.shape
            Tk = eng.attn_keys(eng.encoder_shape(H, W)[0])
            pred.alpha_stores = eng.read_attn_alpha(B, text.shape[1], Tk, logits.device).unsqueeze(-1)
        # BatchNorm side effects of module.train(): running statistics and the batch counter
        with torch.no_grad():
            stats = [(name, buf) for name, buf in model.named_buffers() if name.endswith(("running_mean", "running_var"))]
            if stats:  # one gather kernel + one multi-tensor copy instead of a device copy per buffer
                got = eng.train_gather([n for n, _ in stats], [b for _, b in stats], source="weight")
                torch._foreach_copy_([b for _, b in stats], got)
            for name, buf in model.named_buffers():
                if name.endswith("num_batches_tracked"):
                    buf += 1
        # the statistics copied out above are the engine's own: its raw copies are current, its finalized weights are not
        eng.weights_current(model, [n for n, _ in stats])
        ctx.model, ctx.names, ctx.params = model, names, params
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        eng = ctx.model._engine
        eng.train_backward(dlogits)  # enqueues the whole backward on the current stream and returns
        sync = getattr(ctx.model, "grad_sync", None)
        if sync is None:
            grads = tuple(eng.train_gather(ctx.names, ctx.params))  # views of one flat buffer, filled by one kernel
        else:  # data-parallel: bucketed all-reduce-mean overlapped with the rest of the backward (dist.GradSync)
            grads = tuple(sync.collect(eng.train_grad_into, ctx.names, ctx.params))
        return (None, None, None, None) + grads


def train_forward(model, image, text):
    """logits [B, L, V] with autograd history reaching every trainable parameter of `model`."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    if model.stages["Seq"] != "BiLSTM":
        # mean_height False without a BiLSTM: the reference builds proj_feat and never reads it (build_feat.py:37-40,50-61), so
        # it is no input of the step and its .grad stays None
        named = [(n, p) for n, p in named if not n.startswith("featextractor.proj_feat.")]
    names = tuple(n for n, _ in named)
    return _TrainStep.apply(model, image, text, names, *[p for _, p in named])
