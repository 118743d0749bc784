"""Cost of the LSTM-attention heads' vocabulary size.  usage: attn_vocab_cost.py [V ...]   (default 500 1024 4096 16384)

Decoder wall time on the shipped config/test.yaml geometry (HybridViT + Attnv2, one 448 x 960 crop = 1695 tokens,
batch_max_length 500, all 501 steps): greedy at B = 1 and B = 8, beam 5 on one crop; and a TS0-sized training step
(48 x 64 crops, B = 8, 24-token labels, forward + backward).  The sizes are measured in alternation (two rounds), medians
of the second round's repeats.  V <= 1024 runs the one-class-per-thread decode kernel, larger V the wide one; each row and
step reads all of the generator (1 MiB per 1024 classes)."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from doc2tex_amd import Model, synth  # noqa: E402

H, W, L, BEAM = 448, 960, 500, 5
VS = [int(a) for a in sys.argv[1:]] or [500, 1024, 4096, 16384]


def _load(cfg):
    m = Model(cfg)
    m.load_state_dict(synth.synth_state_dict(m.state_dict(), learned_pos=synth.learned_pos_embed(cfg)))
    return m.cuda()


def _time(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[1:]) * 1e3


def _setup(V):
    cfg = synth.make_config("S0", device="cuda", max_seq_len=L)
    cfg["max_dimension"] = [H, W]
    cfg["num_class"] = V
    g = _load(cfg).eval()
    bcfg = dict(cfg, beam_size=BEAM)
    b = Model(bcfg)
    b.load_state_dict(g.state_dict())
    b = b.cuda().eval()
    tcfg = synth.make_config("TS0", device="cuda", max_seq_len=24)
    tcfg["num_class"] = V
    tr = _load(tcfg)
    tr.conv_precision = "fp32"
    img = synth.synth_images(8, H, W, seed=77).cuda()
    with torch.no_grad():
        mem = {B: g.forward_encoder(img[:B])[0] for B in (1, 8)}
    timg = synth.synth_images(8, 48, 64, seed=78).cuda()
    gen = torch.Generator().manual_seed(79)
    text = torch.zeros(8, 26, dtype=torch.long)
    text[:, 1:25] = torch.randint(2, V, (8, 24), generator=gen)
    text[:, 25] = 1
    return g, b, tr, mem, timg, text.cuda()


def _run(V, s):
    g, b, tr, mem, timg, text = s
    out = {}
    with torch.no_grad():
        for B in (1, 8):
            t = torch.zeros(B, L + 1, dtype=torch.long, device="cuda")
            out[f"greedy B={B}"] = _time(lambda: g.forward_decoder(mem[B], t, is_train=False, is_test=False), 4)
        t1 = torch.zeros(1, L + 1, dtype=torch.long, device="cuda")
        out["beam 5"] = _time(lambda: b.forward_decoder(mem[1], t1, is_train=False, is_test=True), 3)

    def step():
        tr.train()
        tr.zero_grad()
        _, preds, _ = tr(timg, text[:, :-1])
        loss = torch.nn.functional.cross_entropy(preds.reshape(-1, V), text[:, 1:].reshape(-1), ignore_index=0)
        loss.backward()

    out["train TS0 B=8"] = _time(step, 6)
    return out


setups = {V: _setup(V) for V in VS}
res = {}
for rnd in range(2):
    for V in VS:
        r = _run(V, setups[V])
        if rnd == 1:
            res[V] = r
for V in VS:
    r = res[V]
    per = {k: v / (L + 1) for k, v in r.items() if not k.startswith("train")}
    print(f"V={V:6d}: " + ", ".join(f"{k} {v:.1f} ms ({per[k] * 1e3:.0f} us/step)" if k in per else f"{k} {v:.1f} ms"
                                    for k, v in r.items()), flush=True)
