#!/usr/bin/env python3
"""Validation throughput on one MI355X: `doc2tex_amd.validate.validation_step` on C2 (HybridViT + TFM-6, 128x512 crops,
B = 64, 151 steps, seeded weights) over resident batches, against the same loop with the forward pass only.  The
difference is what the second half of the reference's validation loop costs on this engine: labels encoded, the
criterion, token ids -> strings (native host code), the edit-distance and BLEU-count kernels, one download.

Prints one JSON line: formulas/s with metrics, formulas/s forward only, and the host milliseconds per batch between the
two.  A report, not a gate."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from doc2tex_amd import Model, synth
from doc2tex_amd.loss import CrossEntropyLoss
from doc2tex_amd.postprocess import LabelDecoder
from doc2tex_amd.validate import validation_step

SYMBOLS = ["\\frac", "{", "}", "x", "y", "a", "b", "1", "2", "^", "_", "\\mathrm", "\\operatorname", "*", "\\alpha", "+", "=",
           "(", ")", "\\,", "d", "\\hspace", "\\mathbf", "\\left", "\\right", ".", "~", "\\\\", "&", "e", "\\sum", "\\int", "|"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8, help="batches per validation run")
    ap.add_argument("--warmup", type=int, default=2, help="batches of the untimed first run")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--end-bias", type=float, default=1.8, help="raises the [s] logit so that greedy rows end (synth.py)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = synth.make_config("C2", device=str(dev))
    model = Model(cfg)
    tmpl = {k: v for k, v in model.state_dict().items() if not k.endswith("image_positional_encoder.pe")}
    model.load_state_dict(synth.synth_state_dict(tmpl, end_bias=args.end_bias), strict=False)
    model.eval().to(dev)
    vocab = [SYMBOLS[i % len(SYMBOLS)] + ("" if i < len(SYMBOLS) else f"_{i}") for i in range(synth.VOCAB - 4)]
    converter = LabelDecoder(vocab, head="TFM", device=str(dev))
    criterion = CrossEntropyLoss(ignore_index=0, reduction="none")
    B, L = args.batch, cfg["batch_max_length"]
    h, w = synth.crop_shape("C2")
    rng = np.random.default_rng(5)
    loader = []
    for i in range(args.batches):
        images = synth.synth_images(B, h, w, seed=7000 + i).to(dev)
        labels = [[vocab[int(t)] for t in rng.integers(0, len(SYMBOLS), size=int(rng.integers(20, L)))] for _ in range(B)]
        loader.append((images, labels, [f"{i}_{j}.png" for j in range(B)]))
    config = {"Prediction": {"name": "TFM"}, "batch_max_length": L, "use_amp": False, "export_csv": False,
              "sanity_check": False, "token_level": "word", "postprocess": True}

    def forward_only(batches):
        for images, _, _ in batches:
            text = torch.full((images.shape[0], 1), converter.dict["[GO]"], dtype=torch.long, device=dev)
            model(images, text)
        torch.cuda.synchronize()

    with torch.no_grad():
        validation_step(model, None, criterion, loader[:args.warmup], converter, config, None, "cuda")
        forward_only(loader[:args.warmup])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = validation_step(model, None, criterion, loader, converter, config, None, "cuda")
        torch.cuda.synchronize()
        t_val = time.perf_counter() - t0
        t0 = time.perf_counter()
        forward_only(loader)
        t_fwd = time.perf_counter() - t0
    n = out[10]
    chars = sum(len(s) for s in out[7] + out[8]) / (2.0 * n)
    print(json.dumps({"metric": "validation formulas/s (C2, B=%d, one MI355X)" % B, "with_metrics": round(n / t_val, 1),
                      "forward_only": round(n / t_fwd, 1), "extra_ms_per_batch": round((t_val - t_fwd) / args.batches * 1e3, 2),
                      "samples": n, "mean_chars_per_string": round(chars, 1), "accuracy": out[3], "bleu": out[4],
                      "norm_ED": out[5], "word_ED": out[6]}))


if __name__ == "__main__":
    main()
