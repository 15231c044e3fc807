"""Time diverse beam search against plain beam search in the reference scripts' mode: the selected regions of 1 synthetic image x 4
beams, fp16 autocast, max_length 300, early stopping ('bench' weights).  The language model is timed alone (the detector runs once,
outside the window): host wall time around a synchronised call, `--runs` calls per mode after one full-length warm-up each, the modes
alternating inside one process.  --modes: plain = generate(num_beams=4); g1 / g2 / g4 = group_beam_search with that many groups
(penalty 0.5).  Prints one line per mode: median and min .. max ms per call, steps, ms per step."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgrg_amd  # noqa: E402
from rgrg_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="plain,g2,g4")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--max-length", type=int, default=300)
ap.add_argument("--tag", default="")
args = ap.parse_args()

m = rgrg_amd.ReportGenerationModel(True)
m.load_state_dict(synth.make_state_dict(0, "bench"))
m.to("cuda:0").eval()
lm = m.language_model
img = synth.make_images(1, 1234).cuda()
with torch.no_grad():
    _, _, top_feats, cd = m.object_detector(img)
    _, feats = m.binary_classifier_region_selection(top_feats, cd, return_loss=False)
S, nb, L = feats.shape[0], 4, args.max_length


def call(mode):
    if mode == "plain":
        return lm.generate(feats, max_length=L, num_beams=nb, early_stopping=True)
    return lm.group_beam_search(feats, L, nb, int(mode[1:]), 0.5, early_stopping=True)


modes = args.modes.split(",")
times = {k: [] for k in modes}
steps = {}
with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
    for k in modes:   # warm-up: every graph of the timed window is captured
        call(k)
    torch.cuda.synchronize()
    for _ in range(args.runs):
        for k in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call(k)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
            steps[k] = out.shape[1] - 1
for k in modes:
    t = times[k]
    med = statistics.median(t)
    print(f"GROUPBEAMBENCH{args.tag} mode={k} regions={S} rows={S * nb} runs={len(t)} median_ms={med:.1f} min_ms={min(t):.1f} max_ms={max(t):.1f} "
          f"steps={steps[k]} ms_per_step={med / steps[k]:.4f}", flush=True)
