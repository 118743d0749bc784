#!/usr/bin/env python3
"""Generate tests/golden/loss_smooth.{json,npz} from the REFERENCE's LabelSmoothingLoss (modules/loss/labelsmoothing.py).

Authoring-time only: imports the reference checkout (never shipped, never read at test / bench time), runs its criterion
in fp32 on the CPU on seeded inputs (tests/test_criterion_cpu.py smooth_case_inputs regenerates them; they are not stored)
and writes, per case, what it returned -- the per-row losses, or the scalar for a falsy `reduction` -- and 64 entries of
d/dlogits with their (row, column) indices: for each sampled row the target column, the padding column and random others.
Data only; the float64 restatement in the tests is checked against it.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_loss.py <path of the reference checkout>
"""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True

import numpy as np
import torch

# name, rows, V, pad, which rows are padding, classes, smoothing, reduction, seed
CASES = [
    ("r37_v93", 37, 93, 0, "fifth", 93, 0.1, "none", 7101),          # V no multiple of 4 or 64, rows no multiple of 4
    ("r5_v1025", 5, 1025, 0, "fifth", 1025, 0.1, "none", 7102),      # scalar tail behind the vector loads, odd row bases
    ("r4_v11", 4, 11, 2, "one", 11, 0.1, "none", 7103),              # V < 64: lanes without an element
    ("r4_v11_classes9", 4, 11, 2, "one", 9, 0.1, "none", 7103),      # classes != V: only the denominator moves
    ("r24_v16384", 24, 16384, 0, "fifth", 16384, 0.1, "none", 7104),  # the wide vocabulary
    ("r8_v500_no_pad", 8, 500, 0, "none", 500, 0.1, "none", 7105),
    ("r8_v500_all_pad", 8, 500, 0, "all", 500, 0.1, "none", 7106),
    ("r64_v1000_none", 64, 1000, 0, "fifth", 1000, 0.1, "none", 7107),  # the reduction quirks: truthy -> per row ...
    ("r64_v1000_mean", 64, 1000, 0, "fifth", 1000, 0.1, "mean", 7107),
    ("r64_v1000_empty", 64, 1000, 0, "fifth", 1000, 0.1, "", 7107),     # ... falsy -> mean over all rows
    ("r64_v1000_null", 64, 1000, 0, "fifth", 1000, 0.1, None, 7107),
    ("r37_v93_smoothing0", 37, 93, 0, "fifth", 93, 0.0, "none", 7101),  # degenerates to plain cross-entropy
]
KEYS = ("name", "rows", "V", "pad", "pad_rows", "classes", "smoothing", "reduction", "seed")
SAMPLES = 64


def sample_index(c, target):
    """[64, 2] (row, column): up to eight evenly spaced rows (a padding row among them where there is one), each with its
    target column, the padding column and random columns; random pairs fill the rest."""
    g = torch.Generator().manual_seed(c["seed"] + 1)
    rows, V = c["rows"], c["V"]
    n = min(rows, 8)
    picked = sorted({int(r) for r in torch.linspace(0, rows - 1, n).round().tolist()})
    pads = (target == c["pad"]).nonzero().flatten().tolist()
    if pads and not set(pads) & set(picked):
        picked[-1] = pads[0]
    per = SAMPLES // len(picked)
    out = []
    for r in picked:
        cols = [int(target[r]), c["pad"]] + torch.randint(0, V, (per - 2,), generator=g).tolist()
        out += [(r, v) for v in cols]
    while len(out) < SAMPLES:
        r = picked[int(torch.randint(0, len(picked), (1,), generator=g))]
        out.append((r, int(torch.randint(0, V, (1,), generator=g))))
    return np.asarray(out, dtype=np.int32)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "doc2tex")):
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    with contextlib.redirect_stdout(io.StringIO()):
        from doc2tex.modules.loss.labelsmoothing import LabelSmoothingLoss as RefLoss
    cases = [dict(zip(KEYS, c)) for c in CASES]
    with open(os.path.join(GOLD, "loss_smooth.json"), "w") as f:  # the tests read the case list from here
        f.write("[\n" + ",\n".join("  " + json.dumps(c) for c in cases) + "\n]\n")
    # order matters: tests/test_criterion_cpu.py reads loss_smooth.json when it is imported, so the case list is written first
    from test_criterion_cpu import smooth_case_inputs, smooth_restated
    out = {}
    for c in cases:
        x, t, up = smooth_case_inputs(c)
        x.requires_grad_(True)
        crit = RefLoss(c["reduction"], c["classes"], c["pad"], smoothing=c["smoothing"])
        res = crit(x, t)
        assert res.shape == ((c["rows"],) if c["reduction"] else ())
        ((res * up).sum() if c["reduction"] else res).backward()
        gi = sample_index(c, t)
        out[c["name"] + ":loss"] = res.detach().numpy().astype(np.float32)
        out[c["name"] + ":gi"] = gi
        out[c["name"] + ":grad"] = x.grad.numpy()[gi[:, 0], gi[:, 1]].astype(np.float32)
        x64 = x.detach().double()
        err = float((smooth_restated(x64, t, c["classes"], c["pad"], c["smoothing"], c["reduction"]) - res.detach().double()).abs().max())
        print(f"{c['name']:22s} loss max {float(res.detach().abs().max()):9.4f}  fp32 reference vs float64 formula {err:.2e}")
    np.savez_compressed(os.path.join(GOLD, "loss_smooth.npz"), **out)
    print("wrote", os.path.join(GOLD, "loss_smooth.npz"), os.path.getsize(os.path.join(GOLD, "loss_smooth.npz")), "bytes")


if __name__ == "__main__":
    main()
