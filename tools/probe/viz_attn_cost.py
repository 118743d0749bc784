"""Wall time of the shipped config/test.yaml beam search (HybridViT + Attnv2, one 448 x 960 crop = 1694 keys,
batch_max_length 500, beam_size 5) with the decoder alignment maps off and on (viz_attn).  usage: viz_attn_cost.py [end_bias]
end_bias 0.0 runs all 501 steps, 0.3 completes after a few."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from doc2tex_amd import Model, synth  # noqa: E402

H, W, L, beam = 448, 960, 500, 5
for eb in [float(a) for a in sys.argv[1:]] or [0.0, 0.3]:
    cfg = synth.make_config("S0", device="cuda", max_seq_len=L, beam_size=beam)
    cfg["max_dimension"] = [H, W]
    m = Model(cfg)
    m.load_state_dict(synth.synth_state_dict({k: v for k, v in m.state_dict().items()}, end_bias=eb), strict=False)
    m = m.cuda().eval()
    img = synth.synth_images(1, H, W, seed=77).cuda()
    text = torch.zeros(1, L + 1, dtype=torch.long, device="cuda")
    res = {}
    with torch.no_grad():
        for viz in (False, True, False, True):
            m.predicter.Prediction.viz_attn = viz
            ts = []
            for _ in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seq, score, add = m(img, text, is_train=False)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            res.setdefault(viz, []).extend(ts[1:])
    print(f"end_bias {eb}: {seq.shape[1]} tokens; maps off median {statistics.median(res[False]) * 1e3:.1f} ms, "
          f"maps on median {statistics.median(res[True]) * 1e3:.1f} ms (n = {len(res[True])} each)", flush=True)
