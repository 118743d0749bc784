#!/usr/bin/env python3
"""Generate the ViT self-attention map fixtures (tests/golden/vitattn_*.npz, tests/golden/vitattn_cases.json) from the
REFERENCE.

Authoring-container only, like tools/make_golden.py (whose build_ref it reuses): the reference model is built with the
seeded synthetic weights, a forward hook goes on every module whose name contains `attn_drop` -- as the reference's own
attention rollout does (tools/interpretation/vit_visualize.py:26-93) -- and `forward_encoder` runs on synth.synth_images.
Each hook's output is the block's post-softmax attention [B, heads, T, T] (seq_modeling/vit/vision_transformer.py:74-76).
For every case it stores:
  full      the maps of every block, [depth, B, heads, T, T];
  sampled   (the C2 geometry, whose maps would be 13 MB) per block and head the rows 0, two in between and T - 1, and the
            argmax and maximum of every row.
The case list records the reference's module names that contain `attn_drop`.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_vit_attn.py
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

GOLD = G.GOLD
L = 12  # batch_max_length of the built models (the encoder does not read it)

# name, config, kind, B, H, W, weight seed, input seed
CASES = [
    ("vitattn_ts0", "TS0", "full", 2, 48, 64, 1234, 1200),
    ("vitattn_v1_full", "T2V1", "full", 1, 96, 128, 1234, 1201),   # the learned table's own grid: read as it is
    ("vitattn_v1_small", "T2V1", "full", 2, 48, 64, 1234, 1202),   # smaller crop: the table is bicubic-resized
    ("vitattn_v2_small", "T2V2", "full", 2, 48, 64, 1234, 1203),   # learned table, flat prefix slice
    ("vitattn_c2", "C2", "sampled", 1, 128, 512, 1234, 1204),
]


def sample_rows(T):
    return [0, T // 3, (2 * T) // 3, T - 1]


def run(case):
    name, cname, kind, B, H, W, wseed, iseed = case
    cfg, m, _ = G.build_ref(cname, L, wseed=wseed)
    names = [n for n, _ in m.named_modules() if "attn_drop" in n]
    got = {}
    for n, mod in m.named_modules():
        if "attn_drop" in n:
            mod.register_forward_hook(lambda mod_, inp, out, n=n: got.__setitem__(n, out.detach().clone()))
    img = synth.synth_images(B, H, W, seed=iseed)
    with torch.no_grad():
        mem, shape, pad = m.forward_encoder(img)
    assert sorted(got) == sorted(names), (sorted(got), names)
    maps = torch.stack([got[n] for n in names]).numpy().astype(np.float32)  # [depth, B, heads, T, T], block order
    depth, _, heads, T, _ = maps.shape
    assert T == mem.shape[1], (T, mem.shape)
    rep = {"case": name, "config": cname, "kind": kind, "B": B, "H": H, "W": W, "wseed": wseed, "iseed": iseed,
           "max_seq_len": L, "depth": depth, "heads": heads, "T": T, "attn_drop_modules": names,
           "row_sum_max_err": float(np.abs(maps.astype(np.float64).sum(-1) - 1).max())}
    if kind == "full":
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), maps=maps)
    else:
        rows = sample_rows(T)
        rep["rows"] = rows
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), rows=maps[:, :, :, rows, :],
                            argmax=maps.argmax(-1).astype(np.int16), max=maps.max(-1))
    print(f"{name}: {cname} B={B} {H}x{W} T={T} depth={depth} heads={heads} "
          f"{os.path.getsize(os.path.join(GOLD, name + '.npz'))} bytes")
    return rep


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    reps = [run(c) for c in CASES]
    with open(os.path.join(GOLD, "vitattn_cases.json"), "w") as f:
        json.dump({"generator": "tools/make_golden_vit_attn.py", "cases": reps}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
