"""Cost of the ViT self-attention maps (forward hooks on attn_drop): Model.forward_encoder with no hook, with block 0 hooked
and with every block hooked, timed with device events after warm-up.  Geometries: C2 (128 x 512 crops, 261 tokens) at
B = 64 -- 139 MB of maps per hooked block -- and the shipped 448 x 960 crop (1695 tokens) at B = 1 -- 92 MB per block.
usage: vit_attn_maps_cost.py [reps]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from doc2tex_amd import Model, synth  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def timed(m, img):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    with torch.no_grad():
        for _ in range(3):
            m.forward_encoder(img)
        for _ in range(REPS):
            ev[0].record()
            m.forward_encoder(img)
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ts)


for label, H, W, B in [("C2", 128, 512, 64), ("shipped", 448, 960, 1)]:
    cfg = synth.make_config("C2", device="cuda", max_seq_len=4)
    cfg["max_dimension"] = [H, W]
    m = Model(cfg)
    m.load_state_dict(synth.synth_state_dict({k: v for k, v in m.state_dict().items()}), strict=False)
    m = m.cuda().eval()
    img = synth.synth_images(B, H, W, seed=5).cuda()
    drops = [blk.attn.attn_drop for blk in m.seqmodeler.SequenceModeling.blocks]
    T = m.engine().encoder_shape(H, W)[0]
    mb = B * 8 * T * T * 4 / 1e6
    res = {}
    for mode in ("off", "one", "all", "off"):
        hooked = {"off": [], "one": drops[:1], "all": drops}[mode]
        handles = [d.register_forward_hook(lambda *_: None) for d in hooked]
        res.setdefault(mode, []).append(timed(m, img))
        for h in handles:
            h.remove()
    off, one, full = min(res["off"]), res["one"][0], res["all"][0]
    print(f"{label} B={B} T={T}: {mb:.0f} MB of maps per block; encoder {off:.3f} ms maps off, {one:.3f} ms one block hooked "
          f"(+{one - off:.3f}), {full:.3f} ms all {len(drops)} hooked (+{(full - off) / len(drops):.3f} per block)", flush=True)
