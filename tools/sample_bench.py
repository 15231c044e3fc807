"""Cost of a sampling decode step against a greedy one, and of the sample kernel alone.
Usage: python tools/sample_bench.py [--max-length 128] [--runs 3] [--out FILE.md]
For 29 rows in fp32 and 928 rows under bf16 autocast: `LanguageModel.generate` and `LanguageModel.sample` (temperature 1, top_k 50,
top_p 0.9) alternate, `--runs` timed calls each after one warm-up of each; ms per step = call time / (max_length - 1) (the bench
weights never emit EOS, so every call runs all steps; the prefill is inside both).  Then rgrg_sample_logits_f32 alone on
[S, 50272] logits with HIP events, per parameter set, against its floor: one read of S * V * 4 bytes at the 8 TB/s HBM peak.
Prints one JSON line; --out writes the same numbers as a markdown table."""
import argparse
import contextlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgrg_amd  # noqa: E402
from rgrg_amd import synth  # noqa: E402

V, LD, HBM_PEAK = 50257, 50272, 8.0e12


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-length", type=int, default=128)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    model = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    model.load_state_dict(synth.make_state_dict(0, "bench"))
    model.to("cuda:0").eval()
    lm, eng = model.language_model, model.engine()
    steps = args.max_length - 1
    res = {"max_length": args.max_length, "runs": args.runs, "steps": [], "kernel": []}
    for S, dtype in ((29, "f32"), (928, "bf16")):
        feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(99)).to("cuda:0")
        ctx = torch.autocast("cuda", dtype=torch.bfloat16) if dtype == "bf16" else contextlib.nullcontext()
        greedy = lambda: lm.generate(feats, max_length=args.max_length)   # noqa: E731
        sample = lambda: lm.sample(feats, max_length=args.max_length, top_k=50, top_p=0.9, seed=1)   # noqa: E731
        with ctx:
            greedy(), sample()
            g, s = [], []
            for _ in range(args.runs):
                g.append(timed(greedy) / steps)
                s.append(timed(sample) / steps)
        res["steps"].append({"rows": S, "dtype": dtype, "greedy_ms_per_step": g, "sample_ms_per_step": s,
                             "sample_over_greedy": sorted(s)[len(s) // 2] / sorted(g)[len(g) // 2]})
        logits = torch.randn((S, LD), generator=torch.Generator().manual_seed(5)).mul_(3.0).to("cuda:0")
        for name, (T, k, p) in (("no filter", (1.0, 0, 1.0)), ("top_k 50", (1.0, 50, 1.0)), ("top_p 0.9", (1.0, 0, 0.9)),
                                ("top_k 50 + top_p 0.9", (1.0, 50, 0.9)), ("top_k 1", (1.0, 1, 1.0))):
            call = lambda: eng.sample_logits(logits, T, k, p, 7, ld=LD, vocab=V)   # noqa: E731
            call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            iters = 20
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / iters
            floor_us = S * V * 4 / HBM_PEAK * 1e6
            res["kernel"].append({"rows": S, "params": name, "us_per_launch": us, "floor_us": floor_us, "fraction_of_hbm_peak": floor_us / us})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("| rows | dtype | greedy ms / step (runs) | sample ms / step (runs) | sample / greedy (medians) |\n|---|---|---|---|---|\n")
            for r in res["steps"]:
                f.write(f"| {r['rows']} | {r['dtype']} | {', '.join(f'{v:.3f}' for v in r['greedy_ms_per_step'])} | "
                        f"{', '.join(f'{v:.3f}' for v in r['sample_ms_per_step'])} | {r['sample_over_greedy']:.3f} |\n")
            f.write("\n| rows | parameters | us per launch (incl. launch gaps) | floor us (S V 4 B at 8 TB/s) | fraction of peak |\n|---|---|---|---|---|\n")
            for r in res["kernel"]:
                f.write(f"| {r['rows']} | {r['params']} | {r['us_per_launch']:.1f} | {r['floor_us']:.1f} | {r['fraction_of_hbm_peak']:.3f} |\n")


if __name__ == "__main__":
    main()
