#!/usr/bin/env python3
"""tools/serve_bench.py's end-to-end loop on MIXED-SIZE traffic: every page set holds pages that land on the three crop
sizes of config C4 (96x384, 128x512, 160x640), a few per size, so `Preprocessor.batch` hands back three small batches per
set and consecutive forwards differ in row count and memory length.

  --mixed 0   decode groups as they were: a change of size launches the group collected so far, so every small batch pays
              for a step loop of its own (this mode only touches what Model had before decode_group_mixed existed);
  --mixed 1   Model.decode_group_mixed: batches of any size share a loop until the group holds --group batches or
              --group-rows rows.

  --beam K    beam search (width K) instead of greedy decoding, synchronous as Model.beam_search_batch is:
              --mixed 0   one beam_search_batch call per size bucket (three searches per page set, a captured loop per size);
              --mixed 1   the list form: the buckets are encoded one by one, their memories packed, ONE search per page set
                          (d2t_decode_beam_batch_ragged).

  --head attnv2   the stack every shipped configuration of the reference serves: C4's encoder and geometry under the Attnv2
                  coverage-LSTM head with the parameters of config/test.yaml:38-51.
                  --beam K: --mixed 0 pays the host-side step loop's batch_max_length + 1 round trips once per size bucket,
                  --mixed 1 once per page set (d2t_decode_attn_beam_batch_ragged).
                  --beam 0: greedy is_test forwards, pipelined on --chains chains.  --mixed 0: one launch of the one-block-
                  per-row step loop per size bucket, as before Model.attn_decode_group existed; --mixed 1: the buckets'
                  rows share a launch until the group holds --group batches or --group-rows rows (Model.attn_decode_group /
                  attn_decode_group_rows, d2t_decode_attn_greedy_submit_ragged).

  --device-beam 1   (with --head attnv2 --beam K) Model.attn_beam_device: the search's bookkeeping stays on the device, one
                    captured graph per search instead of a host round trip per step;
  --submit 1        (with --head attnv2 --beam K) Model.beam_search_batch_async: a page set's search is submitted and its
                    results are read after the NEXT page set's encoders have been issued, which then run beside the search;
  --end-bias B, --max-length L   the generator's [s] bias and batch_max_length of the attnv2 stack (default: the config's):
                    with a bias at which searches end after a few tens of steps the host loop stops at once while the
                    device-side graph still pays its empty launches up to L + 1.

Prints one JSON line: formulas/s end to end (uint8 pages -> LaTeX strings)."""
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
from doc2tex_amd.postprocess import LabelDecoder
from doc2tex_amd.preprocess import Preprocessor

SYMBOLS = ["\\frac", "{", "}", "x", "y", "a", "b", "1", "2", "^", "_", "\\mathrm", "\\operatorname", "*", "\\alpha", "+", "=",
           "(", ")", "\\,", "d", "\\hspace", "\\mathbf", "\\left", "\\right", ".", "~", "\\\\", "&", "e", "\\sum", "\\int", "|"]
BUCKETS = {(96, 384), (128, 512), (160, 640)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="page sets timed")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--per-size", type=int, default=8, help="pages per crop size in a page set")
    ap.add_argument("--mixed", type=int, default=0, choices=[0, 1])
    ap.add_argument("--group", type=int, default=6, help="batches per decode step loop")
    ap.add_argument("--group-rows", type=int, default=384, help="--mixed 1: row budget of a group")
    ap.add_argument("--chains", type=int, default=3)
    ap.add_argument("--page-sets", type=int, default=4, help="distinct page sets cycled through")
    ap.add_argument("--beam", type=int, default=0, help="beam width; 0 = greedy decoding through the decode groups")
    ap.add_argument("--head", default="tfm", choices=["tfm", "attnv2"], help="prediction head on C4's encoder")
    ap.add_argument("--device-beam", type=int, default=0, choices=[0, 1], help="attnv2 beam search: bookkeeping on the device")
    ap.add_argument("--submit", type=int, default=0, choices=[0, 1], help="attnv2 beam search: submitted, read one page set later")
    ap.add_argument("--end-bias", type=float, default=None, help="attnv2: bias of the generator's [s] logit")
    ap.add_argument("--max-length", type=int, default=None, help="attnv2: batch_max_length")
    args = ap.parse_args()
    if (args.device_beam or args.submit) and not (args.head == "attnv2" and args.beam):
        ap.error("--device-beam / --submit belong to --head attnv2 --beam K")
    if (args.end_bias is not None or args.max_length) and args.head != "attnv2":
        ap.error("--end-bias / --max-length belong to --head attnv2")
    dev = torch.device("cuda", 0)
    cfg = synth.make_config("C4", device=str(dev), beam_size=1)  # (C4 asks for width 5; the searches here take --beam, forward() decodes greedily)
    if args.head == "attnv2":
        cfg["Prediction"] = {"name": "Attnv2", "params": {
            "seqmodel": "TFM", "input_size": 256, "hidden_size": 256, "kernel_size": 2, "kernel_dim": 128, "embed_target": True,
            "enc_init": True, "attn_type": "coverage", "method": "concat", "teacher_forcing": 1.0, "droprate": 0.2}}
        if args.max_length:
            cfg["batch_max_length"] = args.max_length
    model = Model(cfg)
    tmpl = {k: v for k, v in model.state_dict().items() if not k.endswith("image_positional_encoder.pe")}
    model.load_state_dict(synth.synth_state_dict(tmpl, end_bias=args.end_bias or 0.0), strict=False)
    model.eval().to(dev)
    model.pipelined, model.decode_chains, model.decode_group, model.reserved_blocks = True, args.chains, args.group, 0
    if args.mixed:
        model.decode_group_mixed, model.decode_group_rows = True, args.group_rows
    model.attn_beam_device = bool(args.device_beam)
    if args.head == "attnv2" and not args.beam and args.mixed:
        model.attn_decode_group, model.attn_decode_group_rows = args.group, args.group_rows
    opt = {"imgH": None, "imgW": None, "max_dimension": cfg["max_dimension"], "min_dimension": [32, 32], "mean": 0.5,
           "std": 0.5, "rgb": False, "pad": False, "device": str(dev)}
    pre = Preprocessor(opt, "demo")
    attn = args.head == "attnv2"
    vocab = [SYMBOLS[i % len(SYMBOLS)] + ("" if i < len(SYMBOLS) else f"_{i}") for i in range(synth.VOCAB - (3 if attn else 4))]
    dec = LabelDecoder(vocab, head="Attn" if attn else "TFM")
    rng = np.random.default_rng(3)
    n = args.per_size

    def page_set(s):
        # scanned pages that are scaled down onto 160x640, and crops that already have one of the two smaller sizes
        pages = [synth.synth_formula_image(int(rng.integers(380, 396)), int(rng.integers(1580, 1601)), 9000 + s * 64 + i) for i in range(n)]
        pages += [synth.synth_formula_image(128, 512, 9100 + s * 64 + i) for i in range(n)]
        pages += [synth.synth_formula_image(96, 384, 9200 + s * 64 + i) for i in range(n)]
        order = rng.permutation(len(pages))
        return [pages[i] for i in order]

    sets = [page_set(s) for s in range(args.page_sets)]
    go = torch.full((3 * n, 1), 1, dtype=torch.long, device=dev)
    side = torch.cuda.Stream(dev)
    L = (cfg["batch_max_length"] if attn else cfg["Prediction"]["params"]["max_seq_len"]) + 1
    ring = [torch.empty((3 * n, L), dtype=torch.int64).pin_memory() for _ in range(64)]
    state = {"done": 0, "t_post": 0.0, "seq": 0, "sample": "", "lens": 0, "searches": 0, "search_steps": 0}
    submitted = []  # --submit 1: the handles of the page set whose search is still running
    waiting, pending = [], []  # forwards whose decode may not be launched yet; copies in flight (pinned slot, rows, event)

    def copy_out(force):
        ready = [w for w in waiting if force or w[1].ticket is not None]
        if not ready:
            return
        if force:
            model.synchronize(host_sync=False)  # launches an incomplete group
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for tokens, handle in ready:
                handle.wait()  # the side stream waits for exactly that decode
                slot = ring[state["seq"] % len(ring)]
                state["seq"] += 1
                slot[:tokens.shape[0]].copy_(tokens, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending.append((slot, tokens.shape[0], ev))
        for w in ready:
            waiting.remove(w)

    def consume(block):
        while pending and (block or pending[0][2].query()):
            slot, rows, ev = pending.pop(0)
            ev.synchronize()
            t = time.perf_counter()
            latex = dec.to_latex(slot[:rows], "word", postprocess=True)
            state["t_post"] += time.perf_counter() - t
            state["done"] += len(latex)
            state["sample"] = latex[0]

    def emit(found):
        tokens = torch.zeros((len(found), L), dtype=torch.int64)  # PAD behind every hypothesis
        for r, (seq, *_) in enumerate(found):
            tokens[r, :seq.shape[1]] = seq[0]
            state["lens"] += seq.shape[1]
        t = time.perf_counter()
        latex = dec.to_latex(tokens, "word", postprocess=True)
        state["t_post"] += time.perf_counter() - t
        state["done"] += len(latex)
        state["sample"] = latex[0]

    def drain():
        found = []
        for h in submitted:
            found += h.result()
            state["searches"] += 1
            state["search_steps"] += h.steps()
        submitted.clear()
        if found:
            emit(found)

    def step(i):
        tensors, errors = pre.batch(sets[i % len(sets)])
        assert all(e is None for e in errors)
        buckets = {}
        for t in tensors:
            buckets.setdefault(t._base.data_ptr(), t._base)
        assert len(buckets) == 3 and {tuple(x.shape[2:]) for x in buckets.values()} == BUCKETS, [x.shape for x in buckets.values()]
        if args.beam and args.submit:
            with torch.no_grad():  # this page set's encoders are issued while the previous page set's search runs
                if args.mixed:
                    handles = [model.beam_search_batch_async(list(buckets.values()), args.beam)]
                else:
                    handles = [model.beam_search_batch_async(x, args.beam) for x in buckets.values()]
            drain()
            submitted.extend(handles)
            return
        if args.beam:
            with torch.no_grad():
                if args.mixed:
                    found = model.beam_search_batch(list(buckets.values()), args.beam)
                else:
                    found = [r for x in buckets.values() for r in model.beam_search_batch(x, args.beam)]
            emit(found)
            return
        for x in buckets.values():
            with torch.no_grad():
                tokens, _, extra = model(x, go[:x.shape[0]], is_train=False, is_test=attn)  # (the Attn heads serve with the exit)
            waiting.append((tokens, extra["decode"]))
        copy_out(False)
        consume(False)

    for i in range(args.warmup):
        step(i)
    drain()
    copy_out(True)
    consume(True)
    torch.cuda.synchronize(dev)
    state.update(done=0, t_post=0.0, lens=0, searches=0, search_steps=0)
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(args.warmup + i)
    drain()
    copy_out(True)
    consume(True)
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    assert state["done"] == 3 * n * args.steps, (state["done"], 3 * n * args.steps)
    print(json.dumps({"metric": "formulas/s end to end on mixed-size pages (uint8 pages -> LaTeX strings)",
                      "value": round(state["done"] / el, 1), "unit": "formulas/s", "mixed": args.mixed, "steps": args.steps,
                      "per_size": n, "group": args.group, "group_rows": args.group_rows, "chains": args.chains, "beam": args.beam, "head": args.head, "ms_per_page_set": round(el / args.steps * 1e3, 2),
                      "postprocess_ms_per_page_set": round(state["t_post"] / args.steps * 1e3, 2),
                      "sizes": sorted(BUCKETS), "sample_latex_chars": len(state["sample"]),
                      "device_beam": args.device_beam, "submit": args.submit, "end_bias": args.end_bias, "max_length": L - 1,
                      "mean_result_len": round(state["lens"] / max(state["done"], 1), 1) if args.beam else None,
                      "mean_search_steps": round(state["search_steps"] / state["searches"], 1) if state["searches"] else None}))


if __name__ == "__main__":
    main()
