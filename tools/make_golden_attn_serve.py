#!/usr/bin/env python3
"""Generate the fixtures of the pipelined LSTM-attention serving path (tests/golden/attn_serve_*.npz,
tests/golden/attn_serve_cases.json) from the REFERENCE.

Authoring-container only, like tools/make_golden.py (whose build_ref it reuses).  Unlike every other LSTM-head fixture
the rows of these batches emit [s] at DIFFERENT steps (synth.staggered_images), so an early exit that stops a block as
soon as "all rows have ended" -- before the largest end step -- leaves steps unwritten that the reference produces.

For every case the reference runs with is_test=True and viz_attn on; stored: tokens [B, S], probs [B, S, V] (the
reference's full-size, pre-zeroed tensors), Prediction.alpha_stores [B, S, Tk], the end step of every row and the step
count.  The generator asserts what the tests rely on:
  stagger   end steps not all equal, all >= 0, exit step < S - 1;
  noend     some row never ends: nothing is zeroed, the step count is S;
  both      smallest top-1 / top-2 logit gap over the live steps >= 5e-3 (5x the 1e-3 logits bar of the GPU tests);
            the CPU oracle equals the reference (tokens exact, probs <= 2e-6).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_attn_serve.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

import numpy as np
import torch

import make_golden as G  # noqa: E402  (puts the reference on sys.path)
from doc2tex_amd import synth  # noqa: E402
from oracle import restatement as R  # noqa: E402

GOLD = G.GOLD
MIN_GAP = 5e-3
ORACLE_TOL = 2e-6

# name, kind, config, batch_max_length, weight seed, input seed, end_bias, expected end steps
CASES = [
    ("attn_serve_ts0_stagger", "stagger", "TS0", 40, 1234, 1300, 0.18, [6, 6, 14, 6]),
    ("attn_serve_to0_stagger", "stagger", "TO0", 40, 1234, 1300, 0.6, [5, 6, 5, 5]),
    # a row that never ends.  At batch_max_length 40 no bias leaves a row without [s] AND keeps the gap (0.15 gives these
    # end steps with a gap of 6.8e-4 at steps 6 and 10); 10 steps at 0.16 do: rows 1 and 2 would end at steps 26 / 14
    ("attn_serve_ts0_noend", "noend", "TS0", 9, 1234, 1300, 0.16, [6, -1, -1, 6]),
]


def run(case):
    name, kind, cname, L, wseed, iseed, end_bias, want_ends = case
    cfg, m, sd = G.build_ref(cname, L, beam_size=1, wseed=wseed, end_bias=end_bias)
    m.predicter.Prediction.viz_attn = True
    img = synth.staggered_images(seed=iseed)
    B, S = img.shape[0], L + 1
    text = torch.full((B, 1), R.GO, dtype=torch.long)
    with torch.no_grad():
        preds, probs, add = m(img, text, is_train=False, is_test=True)
        po, lo, _ = R.forward(cfg, sd, img, text, is_test=True, faithful=False)
    assert add == {}, add.keys()
    assert tuple(preds.shape) == (B, S) and tuple(probs.shape[:2]) == (B, S), (preds.shape, probs.shape)
    alpha = m.predicter.Prediction.alpha_stores[..., 0]
    ends = [int((preds[b] == 1).nonzero()[0]) if (preds[b] == 1).any() else -1 for b in range(B)]
    assert ends == want_ends, (name, ends)
    if kind == "stagger":
        assert len(set(ends)) > 1 and min(ends) >= 0 and max(ends) < S - 1, ends
        steps = max(ends) + 1
        assert float(probs[:, steps:].abs().max()) == 0.0 and int(preds[:, steps:].abs().max()) == 0
        assert float(alpha[:, steps:].abs().max()) == 0.0
    else:
        assert min(ends) < 0 <= max(ends), ends
        steps = S
    top2 = probs[:, :steps].topk(2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    assert gap >= MIN_GAP, (name, gap)
    assert torch.equal(po, preds), "oracle tokens differ from the reference"
    d = float((lo - probs).abs().max())
    assert d <= ORACLE_TOL, (name, d)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), tokens=preds.numpy().astype(np.int32),
                        probs=probs.numpy().astype(np.float32), alpha=alpha.numpy().astype(np.float32))
    return {"case": name, "kind": kind, "config": cname, "B": B, "H": int(img.shape[2]), "W": int(img.shape[3]),
            "max_seq_len": L, "wseed": wseed, "iseed": iseed, "end_bias": end_bias, "end_steps": ends, "steps": steps,
            "min_top2_gap": gap, "oracle_diff": d, "keys": int(alpha.shape[2]), "vocab": int(probs.shape[2])}


def main():
    out = {"cases": [], "torch": torch.__version__}
    for case in CASES:
        out["cases"].append(run(case))
        print(json.dumps(out["cases"][-1]), flush=True)
    with open(os.path.join(GOLD, "attn_serve_cases.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
