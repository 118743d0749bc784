#!/usr/bin/env python3
"""Times ONE LSTM-attention beam search (no encoder, no post-processing) on the host loop and on the device-side loop
(DESIGN.md section 5.4d): C4's geometry under the shipped Attnv2 parameters, as tools/serve_mixed_bench.py --head attnv2
builds it, searched over seeded random memories [N, T, 256].

  --n N --t T --beam K    samples, memory length, beam width (rows of a step = N x K while every hypothesis lives)
  --max-length L          batch_max_length (the loop has L + 1 steps)
  --end-bias B            bias of the generator's [s] logit: 0 lets every hypothesis run to the limit, a large one ends every
                          search after a step or two -- the device-side graph then pays L - 1 empty steps

Prints one JSON line: median milliseconds per search of `--reps` searches after `--warmup`, host loop and device-side loop
alternating, the steps the search executed (from a submitted search's ticket) and the per-step time of each loop."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch

from doc2tex_amd import Model, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--t", type=int, default=161)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--max-length", type=int, default=150)
    ap.add_argument("--end-bias", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = synth.make_config("C4", device=str(dev))
    cfg["Prediction"] = {"name": "Attnv2", "params": {
        "seqmodel": "TFM", "input_size": 256, "hidden_size": 256, "kernel_size": 2, "kernel_dim": 128, "embed_target": True,
        "enc_init": True, "attn_type": "coverage", "method": "concat", "teacher_forcing": 1.0, "droprate": 0.2}}
    cfg["batch_max_length"] = args.max_length
    model = Model(cfg)
    tmpl = {k: v for k, v in model.state_dict().items() if not k.endswith("image_positional_encoder.pe")}
    model.load_state_dict(synth.synth_state_dict(tmpl, end_bias=args.end_bias), strict=False)
    model.eval().to(dev)
    eng = model.engine()
    mem = torch.randn(args.n, args.t, 256, generator=torch.Generator().manual_seed(5)).to(dev)
    packed, lengths = mem.reshape(-1, 256), [args.t] * args.n

    def search():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = eng.decode_attn_beam_batch_ragged(packed, lengths, args.beam)
        return (time.perf_counter() - t0) * 1e3, out

    times = {0: [], 1: []}
    for i in range(args.warmup + args.reps):
        for on in (0, 1):
            eng.set_attn_beam_device(on)
            ms, out = search()
            if i >= args.warmup:
                times[on].append(ms)
    eng.set_attn_beam_device(0)
    sub = eng.decode_attn_beam_batch_async(packed, lengths, args.beam)
    steps = eng.decode_steps(sub[-1])[0]
    host, devl = statistics.median(times[0]), statistics.median(times[1])
    print(json.dumps({"n": args.n, "t": args.t, "beam": args.beam, "rows": args.n * args.beam, "max_length": args.max_length,
                      "end_bias": args.end_bias, "steps_executed": steps, "mean_result_len": round(sum(r[0].shape[1] for r in out) / len(out), 1),
                      "host_ms": round(host, 3), "device_ms": round(devl, 3), "host_min_ms": round(min(times[0]), 3),
                      "device_min_ms": round(min(times[1]), 3), "host_us_per_executed_step": round(host / steps * 1e3, 1),
                      "device_us_per_loop_step": round(devl / (args.max_length + 1) * 1e3, 1)}))


if __name__ == "__main__":
    main()
