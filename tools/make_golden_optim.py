#!/usr/bin/env python
"""Record tests/golden/optim_family.{npz,json} from the reference's own optimizer classes.

    PYTHONPATH=<reference checkout> python tools/make_golden_optim.py

Runs doc2tex.modules.optim's Lamb, AdamP, MADGRAD and Lookahead in float64 on the CPU for FIXTURE_STEPS steps over the
seeded problem of tests/optim_family_refs.py (start tensors, gradients as functions of the present parameters, cases with
their arguments) and writes, per case, the final parameters and tensor state (npz) and, in the JSON header: the torch
version, each class's defaults, group keys and state keys, the scalar state and groups after the last step, and AdamP's
projection decision per step and tensor (0 none, 1 channel, 2 layer), read off the calls the reference's projection makes.
Only data goes into the repository; the reference is needed to record, never to test."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import optim_family_refs as FR  # noqa: E402

from doc2tex.modules.optim import adamp as ref_adamp  # noqa: E402
from doc2tex.modules.optim import AdamP, Lamb, Lookahead, MADGRAD  # noqa: E402

CLASSES = {"Lamb": Lamb, "AdamP": AdamP, "MADGRAD": MADGRAD}


class ProjectionLog:
    """Counts the view calls of one projection: channel x3 = projected per row; channel x2 + layer x3 = projected as a
    whole; channel x2 + layer x2 = not projected."""

    def __init__(self):
        self.calls = []
        self.views = {"c": ref_adamp._channel_view, "l": ref_adamp._layer_view}
        ref_adamp._channel_view = lambda x: self._view("c", x)
        ref_adamp._layer_view = lambda x: self._view("l", x)

    def _view(self, which, x):
        self.calls.append(which)
        return self.views[which](x)

    def take(self):
        calls, self.calls = "".join(self.calls), []
        return {"": 0, "ccc": 1, "cclll": 2, "ccll": 0}[calls]


def plain(v):
    return list(v) if isinstance(v, tuple) else v


def main():
    log = ProjectionLog()
    arrays = {"start": torch.cat([p.reshape(-1) for p in FR.fixture_start()]).numpy()}
    header = {"torch": torch.__version__, "steps": FR.FIXTURE_STEPS, "classes": {}, "cases": {}}
    for name, (cls, args, overrides, look) in FR.FIXTURE_CASES.items():
        ps = [torch.nn.Parameter(p.clone()) for p in FR.fixture_start()]
        base = CLASSES[cls](FR.fixture_groups(ps, overrides), **args)
        opt = Lookahead(base, **look) if look else base
        modes = []
        for step in range(1, FR.FIXTURE_STEPS + 1):
            for p, g in zip(ps, FR.fixture_grads(ps, step)):
                p.grad = g
            if cls == "AdamP":  # one step per tensor, in order, to attribute the projection calls
                row = []
                for i, p in enumerate(ps):
                    keep = [q.grad for q in ps]
                    for q in ps:
                        q.grad = None
                    p.grad = keep[i]
                    opt.step()
                    row.append(log.take())
                    for q, g in zip(ps, keep):
                        q.grad = g
                modes.append(row)
            else:
                opt.step()
        sd = opt.state_dict()
        scalars, flat = {}, {}
        for i, st in sd["state"].items():
            for k, v in st.items():
                if isinstance(v, torch.Tensor):
                    flat.setdefault(k, []).append(v.reshape(-1))
                else:
                    scalars.setdefault(str(i), {})[k] = v
        # one vector per state key: the tensors that have it, in index order (state_keys says which), flattened
        for k, vs in flat.items():
            arrays[f"{name}/{k}"] = torch.cat(vs).numpy()
        arrays[f"{name}/p"] = torch.cat([p.detach().reshape(-1) for p in ps]).numpy()
        header["cases"][name] = {
            "state_keys": {str(i): sorted(st) for i, st in sd["state"].items()}, "state_scalars": scalars,
            "param_groups": [{k: plain(v) for k, v in g.items()} for g in sd["param_groups"]], "modes": modes}
    for cls, ctor in CLASSES.items():
        opt = ctor([torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))])
        header["classes"][cls] = {"defaults": {k: plain(v) for k, v in opt.defaults.items()},
                                  "group_keys": list(opt.param_groups[0])}
    look = Lookahead(Lamb([torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))]))
    header["classes"]["Lookahead"] = {"defaults": {k: plain(v) for k, v in look.defaults.items()},
                                      "group_keys": list(look.param_groups[0])}
    out = os.path.join(ROOT, "tests", "golden", "optim_family")
    np.savez_compressed(out + ".npz", **arrays)
    with open(out + ".json", "w") as f:
        json.dump(header, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}.npz ({os.path.getsize(out + '.npz')} bytes) and {out}.json")


if __name__ == "__main__":
    main()
