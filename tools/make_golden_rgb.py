#!/usr/bin/env python3
"""Generate the colour (input_channel 3, rgb: True) fixtures from the REFERENCE: tests/golden/rgb_cases.json,
rgb_manifests.json and one rgb_*.npz per case.  Authoring-container only, like tools/make_golden.py, whose case runners
this tool calls (they build the reference Model, load the seeded weights, run it on seeded three-plane crops, assert that
oracle/restatement.py agrees and write the reference's outputs).

Every greedy / beam case records the reference's smallest decision gap and its image seed is advanced until that gap is
>= MIN_GAP = 2e-3: two values that are each within the project's 1e-3 bar cannot change order across 2e-3, so the exact
token / sequence assertions of the GPU tests cannot fail for a correct engine.
  greedy:  min over all rows and steps of (top-1 logit - top-2 logit)                       -> "min_top2_gap"
  beam:    every torch.topk the reference's search calls (tools/beam.py:75, seq2seq.py:145-147, seq2seq_v2.py:97-99) is
           watched: min over steps of the gaps between neighbouring candidates down to the first one that is NOT kept
           (the order among the kept hypotheses and the selection boundary)                   -> "min_top2_gap"
The last entry pins the image seed of the GPU suite's headline-size comparison (C2C, 128x512, B = 2, first 20 steps
against the restatement): the seed is advanced until at most 1 in 10 of the 40 (row, step) pairs has a gap below MIN_GAP.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_rgb.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

import make_golden as MG
from doc2tex_amd import synth
from oracle import restatement as R

MIN_GAP = 2e-3
MAX_TRIES = 40

# name, config, B, H, W, max_seq_len, weight seed, first input seed, end_bias, is_test
GREEDY = [("rgb_t2c_greedy", "T2C", 2, 48, 64, 12, 1234, 3000, 0.0, False),
          ("rgb_ts0c_greedy", "TS0C", 2, 48, 64, 12, 1234, 3100, 0.0, False),
          # 12 steps: with these seeded weights the VGG + BiLSTM head's step 12 has a top-2 gap of 4.4e-4 whatever the crop
          # (its output hardly depends on the image), so the case stops in front of it
          ("rgb_c0c_greedy", "C0C", 2, 32, 320, 11, 1234, 3200, 0.0, False),
          ("rgb_t1c_greedy", "T1C", 2, 32, 64, 12, 1234, 3300, 0.0, False)]
# name, config, H, W, max_seq_len, weight seed, first input seed, end_bias, beam
BEAM = [("rgb_t2c_beam5", "T2C", 48, 64, 16, 1234, 3400, 1.8, 5)]
ATTN_BEAM = [("rgb_ts0c_beam5", "TS0C", 48, 64, 14, 1234, 3500, 0.3, 5)]
# name, config, B, H, W, L, weight seed, input seed
TRAIN_STEP = [("rgb_t2c_train_step", "T2C", 3, 48, 64, 24, 1234, 3600),
              ("rgb_ts0c_train_step", "TS0C", 3, 48, 64, 24, 1234, 3601),
              ("rgb_c0c_train_step", "C0C", 3, 32, 160, 24, 1234, 3602)]
C2C_PARITY = {"config": "C2C", "B": 2, "H": 128, "W": 512, "max_seq_len": 150, "steps": 20, "wseed": 1234, "first_iseed": 3700}


class TopkWatch:
    """Records, for every 1-D torch.topk(k) while active, the smallest gap between neighbours among the k + 1 largest."""

    def __init__(self):
        self.min_gap, self.calls = float("inf"), 0

    def __enter__(self):
        self._fn, self._method = torch.topk, torch.Tensor.topk
        watch = self

        def see(t, k):
            flat = t.detach().reshape(-1).double()
            if flat.numel() > k:
                v = torch.sort(flat, descending=True).values[:k + 1]
                gaps = (v[:-1] - v[1:])[torch.isfinite(v[:-1]) & torch.isfinite(v[1:])]
                if gaps.numel():
                    watch.min_gap = min(watch.min_gap, float(gaps.min()))
                watch.calls += 1

        def fn(t, k, *a, **kw):
            if t.dim() == 1:
                see(t, k)
            return watch._fn(t, k, *a, **kw)

        def method(t, k, *a, **kw):
            if t.dim() == 1:
                see(t, k)
            return watch._method(t, k, *a, **kw)

        torch.topk, torch.Tensor.topk = fn, method
        return self

    def __exit__(self, *exc):
        torch.topk, torch.Tensor.topk = self._fn, self._method


def with_seed(case, pos, run, gap_of):
    """Run `case` with its image seed advanced until the recorded gap is >= MIN_GAP."""
    for t in range(MAX_TRIES):
        c = list(case)
        c[pos] = case[pos] + t
        out = run(tuple(c))
        gap = gap_of(out)
        if gap >= MIN_GAP:
            return out
        print("  ", case[0], "seed", c[pos], "gap", gap, "< MIN_GAP: next seed", flush=True)
    raise SystemExit(f"{case[0]}: no seed within {MAX_TRIES} tries has a gap >= {MIN_GAP}")


def run_beam_watched(runner):
    def run(case):
        with TopkWatch() as w:
            rep = runner(case)
        assert w.calls > 0, "the beam search never called topk"
        rep["min_top2_gap"] = w.min_gap
        rep["topk_calls"] = w.calls
        return rep
    return run


def c2c_parity():
    """Image seed for the headline-size comparison: the restatement alone must leave at most 1 in 10 of the (row, step) pairs
    of the first `steps` steps below MIN_GAP."""
    p = C2C_PARITY
    cfg, m, sd = MG.build_ref(p["config"], p["max_seq_len"], beam_size=1, wseed=p["wseed"])
    text = torch.full((p["B"], 1), R.GO, dtype=torch.long)
    for t in range(MAX_TRIES):
        iseed = p["first_iseed"] + t
        img = synth.synth_images(p["B"], p["H"], p["W"], seed=iseed, channels=3)
        with torch.no_grad():
            preds, logits, _ = R.forward(cfg, sd, img, text, is_test=False, faithful=False)
        top2 = logits[:, :p["steps"]].topk(2, dim=-1).values
        low = int(((top2[..., 0] - top2[..., 1]) < MIN_GAP).sum())
        print("c2c_parity seed", iseed, "pairs below the gap:", low, "of", p["B"] * p["steps"], flush=True)
        if low * 10 <= p["B"] * p["steps"]:
            rep = {k: v for k, v in p.items() if k != "first_iseed"}
            rep.update(case="rgb_c2c_parity", iseed=iseed, low_gap_pairs=low, tokens=preds[:, :p["steps"]].tolist())
            return rep, MG.manifest(sd)
    raise SystemExit("c2c_parity: no seed found")


def main():
    summary = {"min_gap": MIN_GAP, "greedy": [], "beam": [], "attn_beam": [], "train_step": []}
    manifests = {}
    for case in GREEDY:
        rep, man, cname = with_seed(case, 7, MG.run_greedy, lambda o: o[0]["min_top2_gap"])
        manifests[cname] = man
        summary["greedy"].append(rep)
        print("greedy", rep["case"], "seed", rep["iseed"], "dmem", rep["diff_mem_folded"], "dlogit", rep["diff_logits_cached"],
              "gap", rep["min_top2_gap"], flush=True)
    for kind, cases, runner in (("beam", BEAM, MG.run_beam), ("attn_beam", ATTN_BEAM, MG.run_attn_beam)):
        for case in cases:
            rep = with_seed(case, 6, run_beam_watched(runner), lambda o: o["min_top2_gap"])
            summary[kind].append(rep)
            print(kind, rep["case"], "seed", rep["iseed"], rep["seq"], rep["score"], "gap", rep["min_top2_gap"], flush=True)
    for case in TRAIN_STEP:
        rep = MG.run_train_step(case)
        summary["train_step"].append(rep)
        print("train_step", rep["case"], rep["loss"], rep["oracle_worst_rel_grad_diff"], flush=True)
    rep, man = c2c_parity()
    summary["c2c_parity"] = rep
    manifests["C2C"] = man
    with open(os.path.join(MG.GOLD, "rgb_cases.json"), "w") as f:
        json.dump(summary, f, indent=1)
    with open(os.path.join(MG.GOLD, "rgb_manifests.json"), "w") as f:
        json.dump(manifests, f)
    print("wrote the rgb fixtures to", MG.GOLD)


if __name__ == "__main__":
    main()
