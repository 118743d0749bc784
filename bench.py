#!/usr/bin/env python3
"""Headline benchmark: formulas/s, greedy decode of 128x512 crops (BASELINE.json
configs[2]: HybridViT encoder + 6-layer transformer decoder, B=64 per GPU, all
151 decode steps), one process per GPU.

  python bench.py --gpus 1 --steps 5 --warmup 2
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A "step" = one pass of the hot path (Model.forward: encode + KV-cached greedy
decode) over one batch of synthetic crops already resident in HBM.  Data-parallel
weak scaling: every rank decodes its own batch, no data-path collective
(SURVEY.md 8e); the only collectives are the timing barrier / max-reduce.

--precision bf16x3 (default): convolutions on the bf16 matrix cores with every fp32 operand split into
two bf16 (3 MFMAs per product, fp32 accumulate; tokens bit-exact, logits within 1e-3: tests/); --precision
fp32: exact fp32 MFMA everywhere.

Rank 0 prints ONE JSON line with the contract fields plus
  roofline     dominant kernel (the 512->512 3x3 conv @16x129 as implicit GEMM)
               timed live with HIP events inside the timed region (d2t_profile_*)
A plain run does only that: set up, warm up, time the K steps, print the line.

--full adds everything else the line can carry, each measured outside the headline's timed region:
  parity       the timed configuration's first rows against the CPU oracle
  cpu_baseline the CPU oracle in reference-faithful mode (no KV cache, unfused BN),
               timed on this box's host cores on a bounded sample (rank 0, N=1 only)
  secondary    transfer-inclusive rate, the other arithmetics, C0 / C1 / C3 / C4
  stem_hbm     HBM traffic of the network's front from the committed PMC pass

--dump-outputs DIR writes what the last timed step returned (rank 0) as DIR/tokens.npy (float64) and
DIR/logits.npy (float32); inputs and weights are seeded, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

from doc2tex_amd import Model, synth

# MI355X_MICROARCH.md "Chip-level parameters": dense matrix-core peaks
PEAK_F32_MFMA_TFLOPS = 157.3   # v_mfma_f32_32x32x2_f32 (fp32 in / fp32 accumulate)
PEAK_BF16_MFMA_TFLOPS = 2500.0  # v_mfma_f32_32x32x16_bf16, dense


def decoder_flops(L, M, d=256, ff=1024, n=6, V=500):
    """KV-cached algorithmic decoder FLOPs for L generated tokens."""
    per_tok = n * (2 * d * 3 * d + 3 * 2 * d * d + 4 * d * ff) + 2 * d * V
    attn = sum(n * 4 * d * (l + 1 + M) for l in range(L))
    return L * per_tok + attn + n * 2 * M * d * 2 * d


def host_cores():
    """CPU cores this process may actually use (affinity mask and cgroup quota), not the host total."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 64))


def pmc_traffic(precision):
    """HBM bytes per launch of the dominant kernel from the committed PMC passes
    (profiles/rNN_pmc_dominant_kernel_<precision>.json: FETCH_SIZE x2 gfx950 correction + WRITE_SIZE), or None."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_dominant_kernel_{precision}.json")))
    if not files:
        return None, None
    with open(files[-1]) as f:
        pm = json.load(f)
    global _PMC
    _PMC = pm
    return pm.get("hbm_bytes_per_launch"), os.path.relpath(files[-1], ROOT)


_PMC = {}


def train_pmc_traffic(precision, gemm):
    """HBM bytes per launch of the training step's dominant forward / data-gradient convolution from the latest committed PMC
    pass of the training bench (profiles/rNN_pmc_train_dominant_<precision>.json, tools/profile_train_pmc.sh), or None."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_train_dominant_{precision}.json")))
    if not files:
        return None, None
    with open(files[-1]) as f:
        pm = json.load(f)
    if list(pm.get("gemm_MNK", [])) != list(gemm):
        return None, None
    return pm.get("hbm_bytes_per_launch"), os.path.relpath(files[-1], ROOT)


def stem_hbm():
    """HBM traffic and rate of the HBM-bound front of the network (conv0_1 stem, conv0_2, first max-pool) from the latest
    committed PMC pass (profiles/rNN_pmc_stem.json: FETCH_SIZE x 2 + WRITE_SIZE per launch, tools/pmc_aggregate.py), or None."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_stem.json")))
    if not files:
        return None
    with open(files[-1]) as f:
        d = json.load(f)
    d["source"] = os.path.relpath(files[-1], ROOT)
    return d


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, arrays):
    """Write {name: tensor} as dirname/<name>.npy: integer arrays as float64 (exact), the rest as float32.  If the arrays
    exceed DUMP_LIMIT_BYTES together, the same fixed, seeded sample of leading-axis rows is taken from each of them (its
    row indices go to rows.npy)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    out = {}
    for k, t in arrays.items():
        a = t.detach().cpu().numpy()
        out[k] = a.astype(np.float64 if np.issubdtype(a.dtype, np.integer) else np.float32)
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT_BYTES:
        n = min(a.shape[0] for a in out.values())
        keep = max(1, int(n * DUMP_LIMIT_BYTES // total))
        rows = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
        out = {k: a[rows] for k, a in out.items()}
        out["rows"] = rows.astype(np.float64)
    for k, a in out.items():
        np.save(os.path.join(dirname, f"{k}.npy"), a)
    log(f"outputs written to {dirname}: " + ", ".join(f"{k} {list(a.shape)} {a.dtype}" for k, a in out.items()))


def cpu_baseline(cfg_name, H, W, max_len, sample_b, passes=3):
    """The CPU oracle timed on the host cores (bounded sample, 1 warm-up + `passes` timed passes, median), in both modes:
    reference-faithful (what the reference's own CPU path does: unfused conv+BN+ReLU, full-prefix re-decode without a KV
    cache) -> `cpu_baseline`; and cached (BN folded, KV cache, cross K/V projected once: the algorithm the engine runs) ->
    `cpu_baseline_cached`, so that the GPU/CPU ratio splits into an algorithmic and a hardware factor."""
    import statistics
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import oracle_state_dict
    from oracle import restatement as R

    with open(os.path.join(ROOT, "tests", "golden", "manifests.json")) as f:
        man = json.load(f)
    cores = host_cores()
    torch.set_num_threads(cores)
    cfg, sd = oracle_state_dict(cfg_name, man[cfg_name], max_len)
    img = synth.synth_images(sample_b, H, W, seed=1000)
    text = torch.full((sample_b, 1), R.GO, dtype=torch.long)
    out = []
    answers = None
    for faithful in (True, False):
        log(f"cpu baseline ({'faithful' if faithful else 'cached'} mode): {sample_b} crops on {cores} threads, 1 + {passes} passes ...")
        times = []
        with torch.no_grad():
            for i in range(passes + 1):
                t0 = time.perf_counter()
                answers = R.forward(cfg, sd, img, text, is_test=False, faithful=faithful)[:2]
                if i:  # pass 0 warms the thread pool / allocator
                    times.append(time.perf_counter() - t0)
        dt = statistics.median(times)
        mode = ("faithful mode (no KV cache, unfused BN: op-for-op the reference's CPU path)" if faithful else
                "cached mode (BN folded, KV cache, cross K/V projected once: the engine's algorithm)")
        out.append({
            "value": round(sample_b / dt, 4), "unit": "formulas/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{sample_b} crops {H}x{W}, {max_len + 1} greedy steps, oracle/restatement.py {mode}; median of "
                      f"{passes} timed passes after 1 warm-up = {dt:.2f} s (all: {', '.join(f'{t:.2f}' for t in times)})",
        })
    return out[0], out[1], answers  # answers: the oracle's (tokens, logits) for the sample crops (the bench line's parity check)


def train_bench(args, rank, world, dev, dist, emit=True):
    """BASELINE configs[3]: HybridViT + TFM-6 training step, CE loss on synthetic labels, per-GPU batch 32, data-parallel
    with the gradient all-reduce of doc2tex_amd.dist.GradSync.  One step = forward + loss + backward + clip + AdamW.
    emit=False: return the line (rank 0) instead of printing it and leave the process group alone (secondary.train_c3)."""
    from doc2tex_amd.dist import GradSync
    name = "C3"
    H, W = synth.crop_shape(name)
    B = (args.batch if emit else 0) or synth.batch_size(name)
    cfg = synth.make_config(name, device=str(dev))
    L = cfg["Prediction"]["params"]["max_seq_len"]
    model = Model(cfg)
    tmpl = {k: v for k, v in model.state_dict().items() if not k.endswith("image_positional_encoder.pe")}
    model.load_state_dict(synth.synth_state_dict(tmpl), strict=False)
    model.to(dev).train()
    tprec = args.precision if args.precision in ("fp32", "bf16x3") else "bf16x3"  # (the training step has no fp16x2 form)
    model.conv_precision = tprec
    if world > 1:
        model.grad_sync = GradSync()
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    img = synth.synth_images(B, H, W, seed=3000 + rank).to(dev)
    text = synth.synth_labels(B, max_len=L, seed=3000 + rank).to(dev)
    from doc2tex_amd.loss import create_criterion
    crit = create_criterion("entropy", {"ignore_index": 0, "reduction": "none"})  # fused log-softmax + NLL (d2t_ce_*)

    def step():
        _, preds, _ = model(img, text[:, :-1])
        loss = crit(preds.view(-1, preds.shape[-1]), text[:, 1:].contiguous().view(-1)).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
        opt.step()
        model.zero_grad()
        return loss

    parity = None
    if rank == 0 and tprec in ("fp32", "bf16x3"):
        # the bench line proves its training arithmetic: the REFERENCE's training step on the c3_train_step fixture (B = 4,
        # same weights -- nothing has been trained yet) gives this loss; tools/make_golden.py wrote it from the reference
        import numpy as np
        with open(os.path.join(ROOT, "tests", "golden", "cases.json")) as f:
            fx = next(c for c in json.load(f)["train_step"] if c["case"] == "c3_train_step")
        ftext = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "c3_train_step.npz"))["text"]).to(dev)
        fimg = synth.synth_images(fx["B"], fx["H"], fx["W"], seed=fx["iseed"]).to(dev)
        with torch.no_grad():
            _, fp, _ = model(fimg, ftext[:, :-1])
            floss = float(crit(fp.view(-1, fp.shape[-1]), ftext[:, 1:].contiguous().view(-1)).mean())
        rel = abs(floss - fx["loss"]) / max(1.0, abs(fx["loss"]))
        parity = {"fixture": "tests/golden/c3_train_step (the reference's own loss, B = 4, 128x512, 151-token labels)",
                  "loss": round(floss, 7), "reference_loss": fx["loss"], "rel_err": float(f"{rel:.2e}"), "tolerance": 1e-4,
                  "ok": bool(rel <= 1e-4)}
        del fp, fimg, ftext
    for _ in range(args.warmup):
        loss = step()
    torch.cuda.synchronize(dev)
    eng = model.engine(finalize=False)
    eng.profile(True)  # HIP events around every forward / data-gradient GEMM launch of the timed steps
    if dist:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize(dev)
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    eng.profile(False)
    recs = [r for r in eng.profile_read(16384) if r[3] > 0 and r[0] > 0]
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        # roofline of the step's dominant GEMM shape (forward convolutions and their data gradients share shapes and kernel):
        # algorithmic 2*M*N*K per launch / average launch time, against the dense peak of the MFMA type in use
        by_shape = {}
        for M_, N_, K_, ms in recs:
            by_shape.setdefault((M_, N_, K_), []).append(ms)
        roofline = None
        if by_shape:
            dom = max(by_shape, key=lambda q: sum(by_shape[q]))
            dom_ms = sum(by_shape[dom]) / len(by_shape[dom])
            flop = 2.0 * dom[0] * dom[1] * dom[2]
            bf = tprec == "bf16x3"
            peak = PEAK_BF16_MFMA_TFLOPS if bf else PEAK_F32_MFMA_TFLOPS
            ach = flop / (dom_ms * 1e-3) / 1e12
            total_ms = sum(sum(v) for v in by_shape.values())
            traffic, traffic_src = train_pmc_traffic(tprec, dom)
            roofline = {"bound": "mfma", "kernel": "forward / data-gradient convolution GEMM (split-bf16, LDS-DMA kernels on split-record copies of the inputs)" if bf
                        else "forward / data-gradient convolution GEMM (fp32 MFMA)",
                        "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": traffic,
                        "traffic_unit": "HBM bytes per launch", "traffic_source": traffic_src,
                        "gemm_MNK": list(dom), "avg_launch_ms": round(dom_ms, 4), "launches_timed": len(by_shape[dom]),
                        "gemm_ms_per_step": round(total_ms / args.steps, 2),
                        "note": "GEMM launches timed with HIP events (weight-gradient kernels, BatchNorm / attention / element-wise "
                                "kernels, CE, clip and AdamW make up the rest of the step)"}
        line = {
            "metric": "formulas/s (training step, 128x512 crops, CE loss)", "value": round(B * world * args.steps / elapsed, 2),
            "unit": "formulas/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16x3" if tprec == "bf16x3" else "f32", "data": "synthetic",
            "config": {"workload": f"C3: HybridViT + TFM-6 training step, {H}x{W} crops, {L + 1}-token labels, "
                                   "forward + CE + backward + clip + AdamW",
                       "per_gpu_batch": B, "global_batch": B * world,
                       "parallelism": f"dp{world} (per-rank batches, gradient all-reduce-mean in 64 MB buckets over RCCL)"},
            "roofline": roofline, "criterion": "fused CE (d2t_ce_forward / d2t_ce_backward)",
            "loss": round(float(loss), 4), "parity": parity}
        if parity is not None and not parity["ok"]:
            line["value"] = None  # a number without its parity is not a measurement
        if not emit:
            del model, opt
            torch.cuda.empty_cache()
            return line
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"loss": loss})
        print(json.dumps(line), flush=True)
    if dist and emit:
        dist.destroy_process_group()
    return None


def serving_bench(args, name, rank, world, dev, dist, secondary_runs=True, steps=None, warmup=None):
    """Greedy serving of one BASELINE config (C2 = the headline, C1): returns (line, out) on rank 0 -- the contract fields
    with `roofline` (and, with secondary_runs, `secondary.incl_transfers` / `secondary.fp32`) and the (tokens, logits) of
    the first timed measurement's last step -- and (None, None) on the other ranks."""
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    group = args.group if args.group > 0 else (4 if name == "C1" else 6)
    H, W = synth.crop_shape(name)
    B = args.batch or synth.batch_size(name)
    cfg = synth.make_config(name, device=str(dev))
    L = cfg["Prediction"]["params"]["max_seq_len"]
    model = Model(cfg)
    tmpl = {k: v for k, v in model.state_dict().items() if not k.endswith("image_positional_encoder.pe")}
    model.load_state_dict(synth.synth_state_dict(tmpl, end_bias=args.end_bias), strict=False)
    model.eval().to(dev)
    if args.precision:
        model.conv_precision = args.precision
    if args.mixed_units is not None:
        model.mixed_units = args.mixed_units
    precision = model.effective_conv_precision()  # the Model's default for this stack unless --precision says otherwise
    early = args.end_bias != 0.0
    model.pipelined = not args.no_pipeline and not early
    model.decode_chains = args.chains
    model.decode_group = group
    model.reserved_blocks = args.reserve  # decode of batch i overlaps the encoder of batch i+1
    model.reserved_cus = args.reserve_cus
    if args.conv_kernel:
        model.conv_kernel = args.conv_kernel
    host_img = synth.synth_images(B, H, W, seed=1000 + rank).pin_memory()  # each rank its own shard
    img = host_img.to(dev)
    text = torch.full((B, 1), 1, dtype=torch.long, device=dev)
    T = None

    def step(x=None):
        with torch.no_grad():
            return model(img if x is None else x, text, is_train=False, is_test=early)

    primed = []  # the decode graphs depend on the decode buffers only (not on the arithmetic mode or the input tensor)

    def prime():
        """Capture every decode launch configuration the timed region can need before anything is timed: a group that
        synchronize() finds incomplete is decoded at its own row count, on either decode chain (largest group first: the
        engine's buffers only grow, so the addresses the smaller graphs capture stay valid)."""
        if model.pipelined and not primed:
            primed.append(True)
            for n in range(max(1, group), 0, -1):
                for _ in range(2 * max(1, args.chains)):
                    for _ in range(n):
                        step()
                    model.synchronize()

    def timed(steps, warmup, with_transfers=False):
        """W untimed warm-up steps, then exactly `steps` timed ones bracketed by barrier + synchronize on both sides.
        with_transfers: every step first copies its batch from pinned host memory (H2D on a copy stream, two device
        buffers, ordered by events) and the region ends with the D2H of every batch's token ids."""
        prime()
        bufs, copy_stream, free_ev = None, None, None
        if with_transfers:
            bufs = [torch.empty_like(img), torch.empty_like(img)]
            copy_stream = torch.cuda.Stream(device=dev)
            free_ev = [torch.cuda.Event(), torch.cuda.Event()]
            for e in free_ev:
                e.record()

        def h2d(i):
            """H2D of batch i into buffer i & 1 on the copy stream, once the forward that last read that buffer (batch
            i - 2) has consumed it; returns the event the forward of batch i waits for."""
            k = i & 1
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(free_ev[k])
                bufs[k].copy_(host_img, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record()
            return ready

        def fed_step(i, n, toks, pending):
            """One step of the transfer-inclusive loop, fed the way a loader feeds it: the forward of batch i waits for
            its copy, and the copy of batch i + 1 is issued BEFORE that forward is enqueued, so it has a whole forward to
            land in.  Returns (out, the next batch's event)."""
            k = i & 1
            torch.cuda.current_stream(dev).wait_event(pending[0] if pending else h2d(i))
            nxt = [h2d(i + 1)] if i + 1 < n else None
            out = step(bufs[k])
            free_ev[k].record()
            toks.append(out[0])
            return out, nxt

        def drain(toks):
            model.synchronize()  # every batch fully decoded
            return torch.stack(toks).to("cpu", non_blocking=True) if toks else None  # D2H of every batch's token ids

        wtoks = []
        pending = None
        for i in range(warmup):  # the warm-up takes the same path as the timed steps (copy stream, pinned staging, D2H)
            if with_transfers:
                out, pending = fed_step(i, warmup, wtoks, pending)
            else:
                out = step()
        drain(wtoks)
        del wtoks
        eng = model.engine()
        torch.cuda.synchronize(dev)
        eng.profile(not with_transfers)
        toks = []
        marks = [] if with_transfers else [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                                           for _ in range(steps)]
        if dist:
            dist.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(steps):
            if with_transfers:
                out, pending = fed_step(i, steps, toks, pending)  # the first copy is issued (and waited for) inside the region
            else:
                if i < len(marks):
                    marks[i][0].record()
                out = step()
                if i < len(marks):
                    marks[i][1].record()
        host_tok = drain(toks)
        torch.cuda.synchronize(dev)
        if dist:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        eng.profile(False)
        recs = eng.profile_read() if not with_transfers else []
        if dist:
            t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        assert early or out[0].shape == (B, L + 1), out[0].shape
        if with_transfers:
            assert host_tok.shape[0] == steps
        if marks and rank == 0:  # time the caller's stream spends on one forward (encoder + cross K/V + waits for a K/V slot)
            per = [a.elapsed_time(b) for a, b in marks]
            gaps = [marks[i][1].elapsed_time(marks[i + 1][0]) for i in range(len(marks) - 1)]
            log(f"caller stream: forward {sum(per) / len(per):.2f} ms avg (max {max(per):.2f}), gap between forwards "
                f"{sum(gaps) / max(1, len(gaps)):.2f} ms avg")
        return elapsed, recs, out

    def roofline_of(recs, precision, steps):
        """Dominant kernel = the most expensive GEMM shape of the timed region, timed live with HIP events around every
        launch on the launch stream (d2t_profile_*)."""
        by_shape = {}
        for M_, N_, K_, ms in recs:
            if ms > 0 and M_ > 0:
                by_shape.setdefault((M_, N_, K_), []).append(ms)
        total_ms = sum(sum(v) for v in by_shape.values())
        total_flop = sum(2.0 * m * n * k * len(v) for (m, n, k), v in by_shape.items())
        dom = max(by_shape, key=lambda q: sum(by_shape[q]))
        dom_ms = sum(by_shape[dom]) / len(by_shape[dom])
        dom_flop = 2.0 * dom[0] * dom[1] * dom[2]
        achieved = dom_flop / (dom_ms * 1e-3) / 1e12
        traffic, traffic_src = pmc_traffic(precision)
        f16 = precision == "fp16x2"
        mixed = precision == "mixed"  # split-bf16 with the two-MFMA fp16 arithmetic in `mixed_units` of the 512 -> 512 units
        bf = precision == "bf16x3" or f16 or mixed  # (16-bit matrix-core operands: the bf16 / fp16 dense peak)
        peak = PEAK_BF16_MFMA_TFLOPS if bf else PEAK_F32_MFMA_TFLOPS
        roofline = {
            "bound": "mfma",
            "kernel": ("fp16x2 implicit-GEMM convolution (fp16 records x fp16 hi / lo weights), pipelined 256x128 kernel on "
                       "v_mfma_f32_16x16x32_f16" if f16 else
                       f"implicit-GEMM convolution, pipelined 256x128 kernel on 16x16x32 MFMAs: the launches of this shape in the "
                       f"two-MFMA fp16 arithmetic ({model.mixed_units} of the 8 plain 512->512 units) and in split-bf16 together" if mixed else
                       _PMC.get("kernel_short") or ("split-bf16 implicit-GEMM convolution, pipelined 256x128 kernel on v_mfma_f32_16x16x32_bf16" if bf
                                                      else "conv_mfma_kernel<128,128>")) +
                      (" (512->512 3x3 conv @16x129 as implicit GEMM)" if tuple(dom) == (132096, 512, 4608)
                       else f" (the most expensive GEMM shape of the timed region, M x N x K = {dom[0]} x {dom[1]} x {dom[2]})"),
            "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_unit": "HBM bytes per launch",
            "traffic_source": traffic_src,
            "peak_dtype": ("fp16 dense MFMA" if f16 else "bf16 dense MFMA") if bf else "fp32 MFMA",
            "gemm_MNK": list(dom), "flop_per_launch": dom_flop, "avg_launch_ms": round(dom_ms, 4),
            "launches_timed": len(by_shape[dom]),
            "share_of_gemm_time": round(sum(by_shape[dom]) / total_ms, 4),
            "all_encoder_gemms": {"achieved": round(total_flop / (total_ms * 1e-3) / 1e12, 2),
                                  "ms_per_step": round(total_ms / steps, 3)},
        }
        if tuple(dom) != (132096, 512, 4608):  # the committed counter passes describe the headline shape only
            roofline["traffic"], roofline["traffic_source"] = None, None
        elif _PMC.get("mfma_busy_frac") is not None:  # from the same committed PMC pass (kernel alone), not measured live
            roofline["mfma_busy_frac_pmc"] = round(_PMC["mfma_busy_frac"], 4)
            roofline["kernel_alone_ms_rocprof"] = round(_PMC.get("kernel_trace_avg_ms", 0.0), 4)
        if bf and not mixed:  # every algorithmic product costs three bf16 MFMA products (hi*hi + hi*lo + lo*hi), or two fp16 ones (x*lo + x*hi)
            per = 2 if f16 else 3
            roofline["mfma_issued_tflops"] = round(per * achieved, 2)
            roofline["mfma_issued_frac"] = round(per * achieved / peak, 4)
        if os.environ.get("D2T_BENCH_SHAPES"):  # per-shape table of the timed region (in situ: beside the decode streams)
            for shp, v in sorted(by_shape.items(), key=lambda kv: -sum(kv[1])):
                log(f"  GEMM {shp}: {len(v) // max(1, steps)} launches/step, avg {sum(v) / len(v) * 1e3:.0f} us, "
                    f"{sum(v) / steps:.2f} ms/step, {2.0 * shp[0] * shp[1] * shp[2] / (sum(v) / len(v) * 1e-3) / 1e12:.0f} TFLOP/s")
        loops = [(N_, K_, ms) for M_, N_, K_, ms in recs if M_ == -1 and ms > 0]
        if loops:  # the decode step loops that ran beside the encoders (HIP events on the decode streams)
            roofline["decode_loops"] = {"count": len(loops), "rows": loops[0][0], "steps": loops[0][1],
                                        "avg_ms": round(sum(l[2] for l in loops) / len(loops), 2),
                                        "max_ms": round(max(l[2] for l in loops), 2)}
        return roofline

    elapsed, recs, out = timed(steps, warmup)
    first_out = (out[0], out[1])
    if rank == 0:
        log(f"{name}: timed {steps} steps in {elapsed:.3f} s")
    # secondary measurements of the SAME workload (rank-symmetric, so that the collectives inside timed() match up):
    #   incl. transfers -- H2D of every batch and D2H of its token ids inside the timed region (SURVEY 8d's metric definition)
    #   fp32            -- the exact-fp32 arithmetic mode (--precision fp32), fewer steps
    secondary = {}
    if not early and secondary_runs:
        e2, _, o2 = timed(steps, warmup, with_transfers=True)
        # SURVEY 8d quotes the metric with the H2D of the batch and the D2H of the ids inside the region; the task's bench contract
        # asks for `value` with inputs resident in HBM.  Both are in the line: `value` = resident, this = SURVEY 8d's definition.
        secondary["incl_transfers"] = {
            "value": round(world * B * steps / e2, 2), "unit": "formulas/s", "ms_per_step": round(e2 / steps * 1e3, 3),
            "metric_definition": "SURVEY.md 8d (PCIe-inclusive): the rate a caller holding host buffers sees; `value` is the "
                                 "HBM-resident rate the bench contract asks for",
            "what": f"as `value`, plus per step the H2D copy of the batch ({host_img.numel() * 4 / 1e6:.1f} MB from pinned host "
                    "memory, on a copy stream) and, before the region ends, the D2H copy of every batch's token ids",
            "_out": (o2[0], o2[1])}  # (its last batch is checked against the oracle like the headline's: main())
        if precision in ("bf16x3", "fp16x2", "mixed"):
            k3 = max(4, steps // 4)
            model.conv_precision = "fp32"
            e3, r3, o3 = timed(k3, 2)
            model.conv_precision = precision
            if rank == 0:
                secondary["fp32"] = {
                    "value": round(world * B * k3 / e3, 2), "unit": "formulas/s", "ms_per_step": round(e3 / k3 * 1e3, 3),
                    "steps": k3, "dtype": "f32",
                    "what": "same workload and serving configuration with exact fp32 arithmetic on the fp32-input MFMA "
                            "(v_mfma_f32_32x32x2_f32) everywhere",
                    "roofline": roofline_of(r3, "fp32", k3), "_out": (o3[0], o3[1])}
            # the other 16-bit arithmetics beside the headline's, each with its own roofline and its own parity
            others = ["bf16x3"] if precision in ("fp16x2", "mixed") else (["mixed", "fp16x2"] if name in ("C2", "C4") else [])
            what = {"bf16x3": "split-bf16 arithmetic (three bf16 MFMAs per product): the default",
                    "fp16x2": "the backbone's feature maps as fp16 records and its convolutions as x16 * w_lo + x16 * w_hi (two MFMAs "
                              "per product instead of three) in EVERY split-record layer: 5x margin to the logits bar (opt-in; it is "
                              "also what a forward under the caller's torch.autocast runs -- the reference's --amp, api/infer.py:120-124, "
                              "whose own fp16 path sits 3e-3 from its fp32 logits on this config)",
                    "mixed": f"split-bf16 with the two-MFMA fp16 arithmetic in the first {model.mixed_units} of the backbone's eight plain "
                             "512->512 units only, fp16 hi|lo records between them (opt-in; >= 10x margin to the logits bar on this "
                             "config: DESIGN.md section 3)"}
            for other in others:
                model.conv_precision = other
                e4, r4, o4 = timed(steps, 2)
                model.conv_precision = precision
                if rank == 0:
                    secondary[other] = {
                        "value": round(world * B * steps / e4, 2), "unit": "formulas/s", "ms_per_step": round(e4 / steps * 1e3, 3),
                        "steps": steps, "dtype": other if other != "mixed" else f"bf16x3+fp16x2({model.mixed_units}u)",
                        "what": "same workload and serving configuration, " + what[other],
                        "roofline": roofline_of(r4, other, steps),
                        "_out": (o4[0], o4[1])}

    if rank == 0:
        T = model.engine().encoder_shape(H, W)[0]
        bf = precision == "bf16x3"
        roofline = roofline_of(recs, precision, steps)
        formulas = world * B * steps
        ms_step = elapsed / steps * 1e3
        enc_flops = {"C2": 205.28e9, "C1": 50.79e9}.get(name, 0.0)
        algo = enc_flops + decoder_flops(L + 1, T, d=cfg["Prediction"]["params"]["d_model"],
                                         ff=cfg["Prediction"]["params"]["dim_feedforward"],
                                         n=cfg["Prediction"]["params"]["num_decoder_layers"])
        result = {
            "metric": ("formulas/s (greedy decode, 128x512 crops)" if name == "C2" else f"formulas/s ({name})") +
                      (" -- early exit (is_test), synchronous" if early else ""),
            "value": round(formulas / elapsed, 2), "unit": "formulas/s", "n_gpus": world, "steps": steps,
            "warmup": warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16x3" if bf else ("fp16x2" if precision == "fp16x2" else
                                          f"bf16x3+fp16x2({model.mixed_units}u)" if precision == "mixed" else "f32"), "data": "synthetic",
            "config": {"workload": f"{name}: HybridViT(ResNet-512, patch 2x2, depth 6) + TFM-6 greedy, "
                                   f"{H}x{W} crops, {L + 1} decode steps (no early exit)" if name == "C2" else name,
                       "per_gpu_batch": B, "global_batch": B * world, "vocab": synth.VOCAB, "memory_tokens": T,
                       "parallelism": f"dp{world} (batch-sharded, no collective)",
                       "pipelined": bool(model.pipelined), "reserved_blocks": model.reserved_blocks if model.pipelined else 0,
                       "conv_kernel": model.conv_kernel, "reserved_cus": model.reserved_cus if model.pipelined else 0,
                       "decode_chains": model.decode_chains if model.pipelined else 1,
                       "decode_group": model.decode_group if model.pipelined else 1},
            **({"early_exit": {"end_bias": args.end_bias, "decode_steps_run": int(out[0].shape[1])}} if early else {}),
            "algorithmic_gflop_per_formula": round(algo / 1e9, 2),
            "e2e_tflops": round(algo * formulas / elapsed / 1e12, 2),
            "roofline": roofline,
        }
        if secondary:
            result["secondary"] = secondary
        result["_shape"] = (H, W, L, B)
        model.synchronize()
        return result, first_out
    model.synchronize()
    return None, None


def other_configs(args, dev):
    """The other BASELINE configs on one GPU, measured after the headline and outside its timed region (world == 1):
    C1 (configs[1]) greedy serving, C3's per-GPU training step (configs[3]) and C4's beam-5 decode (configs[4])."""
    import copy
    import gc
    out = {}
    gc.collect()  # the headline's model and engine context (its buffers, streams and graphs) go first
    torch.cuda.empty_cache()
    a = copy.copy(args)
    a.batch, a.group = 0, 0
    line, o1 = serving_bench(a, "C1", 0, 1, dev, None, secondary_runs=False, steps=max(40, args.steps), warmup=4)
    out["c1"] = {k: line[k] for k in ("value", "unit", "ms_per_step", "steps", "dtype", "config", "roofline")}
    if not args.no_cpu_baseline:
        out["c1"]["parity"] = oracle_parity("C1", o1, 4, seed=1000)
        if not out["c1"]["parity"]["ok"]:
            out["c1"]["value"] = None
    torch.cuda.empty_cache()
    out["c0"] = c0_bench(dev, cpu=not args.no_cpu_baseline)
    torch.cuda.empty_cache()
    a = copy.copy(args)
    a.steps, a.warmup = max(4, args.steps // 4), 2
    line = train_bench(a, 0, 1, dev, None, emit=False)
    out["train_c3"] = {k: line[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "dtype", "config", "roofline", "loss", "parity")}
    torch.cuda.empty_cache()
    out["c4_beam5"] = beam_bench(dev)
    torch.cuda.empty_cache()
    return out


def oracle_parity(name, outs, n, seed):
    """Rows 0 .. n-1 of a timed batch (crops synth_images(B, ..., seed)) against oracle/restatement.py (KV-cached mode)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import oracle_state_dict
    from oracle import restatement as R
    with open(os.path.join(ROOT, "tests", "golden", "manifests.json")) as f:
        man = json.load(f)
    H, W = synth.crop_shape(name)
    cfg, sd = oracle_state_dict(name, man[name], synth.MAX_LEN)
    img = synth.synth_images(synth.batch_size(name), H, W, seed=seed)[:n]
    text = torch.full((n, 1), R.GO, dtype=torch.long)
    torch.set_num_threads(host_cores())
    with torch.no_grad():
        otok, olog = R.forward(cfg, sd, img, text, is_test=False, faithful=False)[:2]
    tok, lg = outs[0][:n].cpu(), outs[1][:n].cpu()
    exact = bool(torch.equal(tok, otok))
    dl = float((lg - olog).abs().max())
    return {"rows": n, "tokens_exact": exact, "max_abs_dlogit": float(f"{dl:.3e}"), "tolerance": 1e-3, "ok": bool(exact and dl <= 1e-3),
            "what": f"rows 0..{n - 1} of the last timed batch against oracle/restatement.py (KV-cached mode) on the same crops and weights"}


def c0_bench(dev, steps=30, cpu=True):
    """BASELINE configs[0]: CNN (VGG) + BiLSTM + LSTM-attention decoder, batch 4, 32x320 crops, 151 greedy steps -- the
    reference's CPU-runnable case.  GPU: one synchronous Model.forward per step; CPU: the faithful oracle on the SAME crops."""
    import statistics
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import oracle_state_dict
    from oracle import restatement as R
    name = "C0"
    H, W = synth.crop_shape(name)
    B = synth.batch_size(name)
    cfg = synth.make_config(name, device=str(dev))
    m = Model(cfg)
    m.load_state_dict(synth.synth_state_dict({k: v for k, v in m.state_dict().items()}), strict=False)
    m = m.to(dev).eval()
    himg = synth.synth_images(B, H, W, seed=1000)
    img = himg.to(dev)
    text = torch.full((B, 1), 1, dtype=torch.long, device=dev)  # (ignored by the LSTM-attention decoder at inference)
    with torch.no_grad():
        for _ in range(3):
            o = m(img, text, is_train=False)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            o = m(img, text, is_train=False)
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / steps
    res = {"value": round(B / dt, 2), "unit": "formulas/s", "ms_per_step": round(dt * 1e3, 3), "steps": steps, "dtype": m.effective_conv_precision(),
           "config": {"workload": f"C0: VGG + BiLSTM + LSTM-attention decoder, {H}x{W} crops, {o[0].shape[1]} greedy steps, synchronous forward",
                      "per_gpu_batch": B}}
    if cpu:
        with open(os.path.join(ROOT, "tests", "golden", "manifests.json")) as f:
            man = json.load(f)
        ocfg, sd = oracle_state_dict(name, man[name], synth.MAX_LEN)
        torch.set_num_threads(host_cores())
        times = []
        with torch.no_grad():
            for i in range(4):
                t0 = time.perf_counter()
                otok, olog = R.forward(ocfg, sd, himg, text.cpu(), is_test=False, faithful=True)[:2]
                if i:
                    times.append(time.perf_counter() - t0)
        cdt = statistics.median(times)
        res["cpu_baseline"] = {"value": round(B / cdt, 3), "unit": "formulas/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": f"the same {B} crops, oracle/restatement.py faithful mode (op-for-op the reference's CPU path), "
                                         f"median of 3 timed passes after 1 warm-up = {cdt:.2f} s"}
        exact = bool(torch.equal(o[0].cpu(), otok))
        dl = float((o[1].cpu() - olog).abs().max())
        res["parity"] = {"rows": B, "tokens_exact": exact, "max_abs_dlogit": float(f"{dl:.3e}"), "tolerance": 1e-3, "ok": bool(exact and dl <= 1e-3)}
        res["speedup_vs_cpu"] = round(res["value"] / res["cpu_baseline"]["value"], 1)
        if not res["parity"]["ok"]:
            res["value"] = None
    del m
    return res


def beam_bench(dev, n=128, beam=5, per_sample=8):
    """BASELINE configs[4] per-GPU work: the C2 model under max_dimension [160, 640], beam width 5, one bucket (160x640) of
    n crops: the batched API (Model.beam_search_batch: encoder on the whole batch, all hypotheses in one step loop) and the
    reference-shaped call (one sample per forward, tfm.py:146-148) on the first `per_sample` crops."""
    cfg = synth.make_config("C4", device=str(dev), beam_size=beam)
    H, W = synth.crop_shape("C4")
    m = Model(cfg)
    m.load_state_dict(synth.synth_state_dict({k: v for k, v in m.state_dict().items()}), strict=False)
    m = m.to(dev).eval()
    img = synth.synth_images(n, H, W, seed=11)
    # row 0 of the timed batch is the crop of the reference fixture c4_beam5_160_full (same weights, beam 5, 151 steps): the
    # reference's own sequence and score for it ride in the timed region
    with open(os.path.join(ROOT, "tests", "golden", "cases.json")) as f:
        fx = next(c for c in json.load(f)["beam"] if c["case"] == "c4_beam5_160_full")
    img[:1] = synth.synth_images(1, fx["H"], fx["W"], seed=fx["iseed"])
    img = img.to(dev)
    go = torch.ones(1, 1, dtype=torch.long, device=dev)
    with torch.no_grad():
        m.beam_search_batch(img, beam)  # warm-up (buffers, graphs)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        seqs = m.beam_search_batch(img, beam)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        seq0, score0 = seqs[0]
        same = seq0[0].tolist() == fx["seq"]
        dscore = abs(float(score0) - float(fx["score"]))
        parity = {"fixture": "tests/golden c4_beam5_160_full (the reference's forward_beam on this crop)", "row": 0,
                  "sequence_exact": bool(same), "abs_dscore": float(f"{dscore:.3e}"), "tolerance": max(1e-3, 2e-5 * len(fx["seq"])),
                  "ok": bool(same and dscore <= max(1e-3, 2e-5 * len(fx["seq"])))}
        m(img[:1], go, is_train=False, is_test=True)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for i in range(per_sample):
            m(img[i:i + 1], go, is_train=False, is_test=True)
        torch.cuda.synchronize(dev)
        ds = time.perf_counter() - t1
    # the same batch with the [s] bias raised (as the early-exit fixtures: +1.8): with the seeded weights [s] then enters the top
    # five at the first step -- one hypothesis per sample completes there and wins on score / length, the other four rows run on
    # (the synthetic logits hardly depend on the crop: up to +1.75 nothing completes, from +1.8 this happens for every sample),
    # so the completed-hypothesis bookkeeping and the shrinking row set run inside a timed region
    m2 = Model(synth.make_config("C4", device=str(dev), beam_size=beam))
    m2.load_state_dict(synth.synth_state_dict({k: v for k, v in m2.state_dict().items()}, end_bias=1.8), strict=False)
    m2 = m2.to(dev).eval()
    with torch.no_grad():
        m2.beam_search_batch(img, beam)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        seqs_e = m2.beam_search_batch(img, beam)
        torch.cuda.synchronize(dev)
        de = time.perf_counter() - t2
    lens_e = sorted(int(q.shape[1]) for q, _ in seqs_e)
    del m2
    return {"value": round(n / dt, 2) if parity["ok"] else None, "unit": "formulas/s", "ms_per_batch": round(dt * 1e3, 2), "dtype": m.effective_conv_precision(),
            "parity": parity,
            "with_end_bias": {"end_bias": 1.8, "value": round(n / de, 2), "unit": "formulas/s", "ms_per_batch": round(de * 1e3, 2),
                              "sequence_lengths": {"min": lens_e[0], "median": lens_e[len(lens_e) // 2], "max": lens_e[-1],
                                                   "completed_before_the_last_step": sum(1 for v in lens_e if v < lens_e[-1])}},
            "config": {"workload": f"C4: HybridViT + TFM-6, beam width {beam}, {H}x{W} crops (max_dimension [160, 640]), one bucket "
                                   f"per batch, up to {cfg['Prediction']['params']['max_seq_len'] + 1} steps, batched API",
                       "per_gpu_batch": n},
            "sequence_lengths": sorted(set(int(q.shape[1]) for q, _ in seqs)),
            "per_sample_api": {"value": round(per_sample / ds, 2), "unit": "formulas/s", "samples": per_sample,
                               "what": "Model.forward on one crop at a time (encoder + beam search per call), as the reference's "
                                       "forward_beam requires"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--config", default="C2", help="C2 (headline) or C1")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: the config's)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--mixed-units", type=int, default=None,
                    help="--precision mixed: how many of the backbone's eight plain 512->512 units run the two-MFMA fp16 arithmetic")
    ap.add_argument("--precision", default=None, choices=["fp32", "bf16x3", "fp16x2", "mixed"],
                    help="convolution arithmetic: exact fp32 MFMA, split-bf16 (3 bf16 MFMAs per product), or fp16 feature maps x fp16 "
                         "hi / lo weights in the backbone (2 MFMAs per product; opt-in, DESIGN.md section 3).  Default: the Model's "
                         "own default (bf16x3); the other 16-bit arithmetic runs beside it under `secondary`")
    ap.add_argument("--reserve", type=int, default=0,
                    help="pipelined mode: block slots the persistent convolution leaves free for the decode stream")
    ap.add_argument("--conv-kernel", default=None, choices=["classic", "pipelined16"],
                    help="split-bf16 convolution kernel: 256x128 tile with loader waves, one block per CU / 128x128, two per CU")
    ap.add_argument("--reserve-cus", type=int, default=0,
                    help="pipelined mode: compute units the pipelined convolution kernel's grid leaves to the decode streams")
    ap.add_argument("--chains", type=int, default=3, choices=[1, 2, 3, 4],
                    help="pipelined mode: decode loops in flight side by side")
    ap.add_argument("--group", type=int, default=0,
                    help="pipelined mode: decode the rows of this many consecutive batches in one step loop "
                         "(default: 6 for C2 -- the loop's duration hardly depends on the row count and it runs in the "
                         "gaps the convolutions leave, so larger groups mean fewer loops beside the encoders; 4 for C1)")
    ap.add_argument("--end-bias", type=float, default=0.0,
                    help="secondary run (SURVEY 8d): raise the [s] logit bias of the synthetic weights by this much so that "
                         "rows terminate, and decode with is_test=True (the reference's early exit: a batch stops at the "
                         "first step at which every row has ended); synchronous, not pipelined")
    ap.add_argument("--train", action="store_true",
                    help="secondary mode (BASELINE configs[3]): time the training step of config C3 -- forward under "
                         "module.train(), CE, backward in the HIP engine, bucketed RCCL gradient all-reduce when more than "
                         "one rank runs, clip, AdamW -- and print its own JSON line instead of the headline metric")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="finish each batch's decode before the next batch's encoder starts")
    ap.add_argument("--cpu-sample", type=int, default=8,
                    help="crops in the CPU-baseline sample (1 warm-up + 3 timed passes in each of the two oracle modes: ~30 s)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the secondary measurements (transfer-inclusive rate, exact-fp32 mode)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the oracle parity check, the CPU baseline, the secondary "
                         "measurements and the other configurations (off: only what the headline figure needs)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()
    if not args.full:
        args.no_cpu_baseline, args.no_secondary = True, True

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` without a launcher: start one fresh rank process per GPU ourselves (before anything here
        # has touched the GPU -- never re-exec a process that initialised HIP) and exit with the worst of their codes.
        # Rank 0 prints the JSON line to the stdout the children inherit.
        import socket
        import subprocess
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        procs = []
        for r in range(args.gpus):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
        # poll: the first rank that exits non-zero takes its siblings with it (they would otherwise sit in a barrier or a
        # collective until the caller's limit), and the launcher exits non-zero
        codes = [None] * len(procs)
        bad = None
        while any(c is None for c in codes) and bad is None:
            for i, q in enumerate(procs):
                if codes[i] is None:
                    codes[i] = q.poll()
                    if codes[i] not in (None, 0):
                        bad = i
            if bad is None:
                time.sleep(0.2)
        if bad is not None:
            log(f"rank {bad} exited with code {codes[bad]}: terminating the other ranks")
            for i, q in enumerate(procs):
                if codes[i] is None:
                    q.terminate()
            for i, q in enumerate(procs):
                if codes[i] is None:
                    try:
                        codes[i] = q.wait(timeout=20)
                    except subprocess.TimeoutExpired:
                        q.kill()
                        codes[i] = q.wait()
            sys.exit(abs(codes[bad]) or 1)
        sys.exit(0)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        args.gpus = world
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1 or "RANK" in os.environ:  # under torch.distributed.run (also with one rank)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    if args.train:
        train_bench(args, rank, world, dev, dist)
        return
    name = args.config
    early = args.end_bias != 0.0
    result, out = serving_bench(args, name, rank, world, dev, dist, secondary_runs=not args.no_secondary)
    if rank == 0:
        H, W, L, B = result.pop("_shape")
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"tokens": out[0], "logits": out[1]})
        if args.full:
            stem = stem_hbm()
            if stem:
                result["stem_hbm"] = stem
        parity_ok = True
        if world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"], result["cpu_baseline_cached"], answers = cpu_baseline(name, H, W, L, args.cpu_sample)
            f, c_ = result["cpu_baseline"]["value"], result["cpu_baseline_cached"]["value"]
            result["speedup_vs_cpu"] = round(result["value"] / f, 1)
            # the ratio splits into what the algorithm buys on the same CPU (KV cache, folded BN) and what the GPU buys
            result["speedup_split"] = {"algorithm_on_cpu": round(c_ / f, 2), "hardware_vs_cached_cpu": round(result["value"] / c_, 1)}
            if not early and args.batch in (0, B) and args.cpu_sample <= B:
                # the bench line proves its own answers: the CPU sample IS the first rows of the timed batch (same seed), so
                # the tokens / logits the TIMED configuration produced for them are checked against the oracle's
                n = args.cpu_sample
                tok, lg = out[0][:n].cpu(), out[1][:n].cpu()
                exact = bool(torch.equal(tok, answers[0]))
                dl = float((lg - answers[1]).abs().max())
                parity_ok = exact and dl <= 1e-3
                result["parity"] = {"rows": n, "tokens_exact": exact, "max_abs_dlogit": float(f"{dl:.3e}"), "tolerance": 1e-3,
                                    "what": f"rows 0..{n - 1} of the last batch of the timed region (pipelined, decode groups of "
                                            f"{result['config']['decode_group']}) against oracle/restatement.py (KV-cached mode) on the "
                                            "same crops and weights"}
        for leg in result.get("secondary", {}).values():  # the other 16-bit runs prove their answers the same way (or carry none)
            if not isinstance(leg, dict) or "_out" not in leg:
                continue
            o4 = leg.pop("_out")
            if "parity" in result:
                n = args.cpu_sample
                exact = bool(torch.equal(o4[0][:n].cpu(), answers[0]))
                dl = float((o4[1][:n].cpu() - answers[1]).abs().max())
                leg["parity"] = {"rows": n, "tokens_exact": exact, "max_abs_dlogit": float(f"{dl:.3e}"), "tolerance": 1e-3,
                                 "all_rows_equal_the_headline_tokens": bool(torch.equal(o4[0].cpu(), out[0].cpu()))}
                if not (exact and dl <= 1e-3):
                    leg["value"] = None  # a number without its parity is not a measurement
        if world == 1 and name == "C2" and not early and not args.no_secondary:
            result.setdefault("secondary", {}).update(other_configs(args, dev))
        print(json.dumps(result), flush=True)
        if not parity_ok:
            log("PARITY FAILURE: the timed configuration's answers differ from the oracle's")
            sys.exit(3)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
