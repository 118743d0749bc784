#!/usr/bin/env python3
"""Time the training step (config C3 per-GPU shard: HybridViT + TFM-6, 128x512 crops, B=32, 150-token labels):
forward (module.train()) + CE + backward in the HIP engine + the optimizer step: clip_grad_norm_ + torch.optim.AdamW
(--optimizer torch, the default: earlier numbers stay comparable) or doc2tex_amd.optim.FusedAdamW with max_grad_norm
(--optimizer fused: clip, update and engine weight refresh in one pass).
usage: train_bench.py [B] [steps] [fp32|bf16x3] [C2|S0] [--criterion entropy|entropy_smooth|smooth] [--optimizer torch|fused]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from doc2tex_amd import Model, synth

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=32)
ap.add_argument("steps", nargs="?", type=int, default=5)
ap.add_argument("precision", nargs="?", default="bf16x3")
ap.add_argument("config", nargs="?", default="C2")  # "S0" = HybridViT + Attnv2 (the LSTM head of config/train.yaml)
ap.add_argument("--criterion", choices=["entropy", "entropy_smooth", "smooth"], default="entropy")
ap.add_argument("--optimizer", choices=["torch", "fused"], default="torch")
args = ap.parse_args()
B, steps, CFG = args.B, args.steps, args.config
cfg = synth.make_config(CFG, device="cuda")
H, W = synth.crop_shape(CFG)
L = cfg["batch_max_length"]
m = Model(cfg)
tmpl = {k: v for k, v in m.state_dict().items()}
m.load_state_dict(synth.synth_state_dict(tmpl), strict=False)
m = m.cuda().train()
m.conv_precision = args.precision
if args.optimizer == "fused":
    from doc2tex_amd.optim import FusedAdamW
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, max_grad_norm=5.0, model=m)
else:
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4)
img = synth.synth_images(B, H, W, seed=7).cuda()
text = synth.synth_labels(B, max_len=L, seed=7)
if cfg["Prediction"]["name"] != "TFM":  # Attn converter: [GO] = 0, [s] = 1 (attn_converter.py:8)
    t = text.clone(); t[text == 1] = 0; t[text == 2] = 1; text = t
text = text.cuda()
from doc2tex_amd.loss import LabelSmoothingLoss, create_criterion
if args.criterion == "entropy":
    crit = create_criterion("entropy", {"ignore_index": 0, "reduction": "none"})  # fused log-softmax + NLL (d2t_ce_*)
elif args.criterion == "entropy_smooth":  # loss_args: {label_smoothing: 0.1} (d2t_ce_smooth_*, torch mode)
    crit = create_criterion("entropy", {"ignore_index": 0, "reduction": "none", "label_smoothing": 0.1})
else:  # name: 'smooth' (d2t_ce_smooth_*, reference mode)
    crit = LabelSmoothingLoss("none", synth.VOCAB, 0, smoothing=0.1)


def step():
    _, preds, _ = m(img, text[:, :-1])
    loss = crit(preds.view(-1, preds.shape[-1]), text[:, 1:].contiguous().view(-1)).mean()
    loss.backward()
    if args.optimizer == "torch":
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
    opt.step()
    m.zero_grad()
    return loss


for _ in range(2):
    l = step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    l = step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
print(f"train step {CFG} B={B} {m.conv_precision} criterion {args.criterion} optimizer {args.optimizer}: {dt * 1e3:.1f} ms = {B / dt:.1f} formulas/s, loss {float(l):.4f}, "
      f"peak mem {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB (torch), weight uploads {m._engine.weight_uploads} in {steps + 2} steps")
