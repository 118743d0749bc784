#!/usr/bin/env python3
"""Time one step of FusedLamb, FusedAdamP, FusedMADGRAD and one Lookahead synchronisation over the parameter shapes of a
synthetic model (default C3) against the float32 eager restatement of the same rule (tests/optim_family_refs.py, tensor by
tensor: what a user who carried the reference's Python classes over would run; its LAMB trust ratio and AdamP decision read
the device once per tensor, as the reference's AdamP does).  Device events around `iters` steps, warm-up first, the two sides
alternating round by round; the best round of each side is reported beside all rounds.  Prints one JSON line per optimizer.

Usage: python tools/optim_family_bench.py [--config C3] [--iters 20] [--eager-iters 3] [--rounds 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import optim_family_refs as FR  # noqa: E402
from doc2tex_amd import Model, synth  # noqa: E402
from doc2tex_amd import optim as O  # noqa: E402


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters  # ms per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--eager-iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_family_bench: needs the GPU (a CPU timing says nothing about it)")
    shapes = [tuple(p.shape) for p in Model(synth.make_config(a.config)).parameters() if p.requires_grad]
    gen = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen).cuda()
    numel = sum(p.numel() for p in ps)
    wd = 0.01

    states = {"lamb": {}, "adamp": {}, "madgrad": {}}

    def eager_lamb():
        state = states["lamb"]
        step = state["step"] = state.get("step", 0) + 1
        norm = float(torch.sqrt(sum((p.grad * p.grad).sum() for p in ps)))
        div = FR.lamb_divisor(norm, 1.0)
        for i, p in enumerate(ps):
            m, v = state.get(i) or (torch.zeros_like(p), torch.zeros_like(p))
            new, m, v = FR.lamb_step(p, p.grad, m, v, step, 1e-3, (0.9, 0.999), 1e-6, wd, div, dtype=torch.float32)
            state[i] = (m, v)

    def eager_adamp():
        state = states["adamp"]
        step = state["step"] = state.get("step", 0) + 1
        for i, p in enumerate(ps):
            m, v = state.get(i) or (torch.zeros_like(p), torch.zeros_like(p))
            new, m, v, _, _ = FR.adamp_step(p, p.grad, m, v, step, 1e-3, (0.9, 0.999), 1e-8, wd, 0.1, 0.01, True, dtype=torch.float32)
            state[i] = (m, v)

    def eager_madgrad():
        state = states["madgrad"]
        step = state["step"] = state.get("step", 0) + 1
        for i, p in enumerate(ps):
            q, s, x0 = state.get(i) or (torch.zeros_like(p), torch.zeros_like(p), p.detach().clone())
            new, q, s = FR.madgrad_step(p, p.grad, q, s, x0, step, 1e-2, 0.9, 1e-6, wd, dtype=torch.float32)
            state[i] = (q, s, x0)

    slow = [p.detach().clone() for p in ps]

    def eager_lookahead():
        for p, s in zip(ps, slow):
            FR.lookahead_sync(p, s, 0.5, dtype=torch.float32)

    look = O.Lookahead(O.FusedLamb(ps, lr=0.0), alpha=0.5, k=1)
    look.sync_lookahead()  # creates the slow weights
    sides = {
        "lamb": (O.FusedLamb(ps, lr=1e-3, weight_decay=wd).step, eager_lamb),
        "adamp": (O.FusedAdamP(ps, lr=1e-3, weight_decay=wd, wd_ratio=0.01, nesterov=True).step, eager_adamp),
        "madgrad": (O.FusedMADGRAD(ps, lr=1e-2, momentum=0.9, weight_decay=wd).step, eager_madgrad),
        "lookahead_sync": (look.sync_lookahead, eager_lookahead),
    }
    for name, (fused, eager) in sides.items():
        timed(fused, 3)  # warm-up: code objects, staging buffers, allocator
        timed(eager, 1)
        rounds = {"fused": [], "eager": []}
        for _ in range(a.rounds):
            rounds["fused"].append(timed(fused, a.iters))
            rounds["eager"].append(timed(eager, a.eager_iters))
        print(json.dumps({"optimizer": name, "config": a.config, "tensors": len(ps), "numel": numel,
                          "fused_ms": min(rounds["fused"]), "eager_fp32_ms": min(rounds["eager"]),
                          "fused_rounds_ms": [round(t, 4) for t in rounds["fused"]],
                          "eager_rounds_ms": [round(t, 3) for t in rounds["eager"]]}), flush=True)


if __name__ == "__main__":
    main()
