"""Beam search from a prompt: what the shared prompt pass costs, and that a BOS prompt runs at the speed of generate(num_beams).
Usage: python tools/prompt_beam_bench.py [--runs 5] [--new-tokens 8] [--out FILE.md]
29 items x 4 beams under fp16 autocast (the scripts' mode; 'bench' weights: no row emits EOS), T = 4, 16, 64 prompt tokens:
  (a) LanguageModel.beam_search - a call that ends with the first ranking (max_length = T + 1: image slot, ONE prompt pass over
      29 x T token rows into cache row s * 4, lm_head over 116 rows, ranking) and a call that generates --new-tokens tokens;
  (g) LanguageModel.greedy_search at the same S and T, ending with its first token (max_length = T + 1): the prompt pass of the
      parent commit, unchanged.  Expanding the prompts - one pass per beam row - would cost num_beams times (g).
  BOS: a [29,1] prompt of BOS with a mask of ones against generate(num_beams=4) at the same max_length, alternating in one process,
      and generate against itself (the spread that repeating the same call shows).
One warm-up of each, then --runs timed calls each (alternating), medians.  Prints one JSON line; --out writes a markdown table."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgrg_amd  # noqa: E402
from rgrg_amd import synth  # noqa: E402

DEV = "cuda:0"
S, NB, BOS = 29, 4, 50256


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--new-tokens", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    model = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    model.load_state_dict(synth.make_state_dict(0, "bench"))
    model.to(DEV).eval()
    lm = model.language_model
    n = args.new_tokens
    scorer = SimpleNamespace(num_beams=NB, _beam_hyps=[None] * S, length_penalty=1.0, do_early_stopping=False, num_beam_hyps_to_keep=1,
                             num_beam_groups=1)
    auto = lambda: torch.autocast("cuda", dtype=torch.float16)   # noqa: E731
    rows = []
    for T in (4, 16, 64):
        g = torch.Generator().manual_seed(1000 * S + T)
        ids = torch.randint(0, 50000, (S, T), generator=g).to(DEV)
        mask = torch.ones((S, T), dtype=torch.int64, device=DEV)
        feats = torch.randn((S, 1024), generator=g).to(DEV)
        ids_x, mask_x = ids.repeat_interleave(NB, 0), mask.repeat_interleave(NB, 0)

        def beam(new):
            with auto():
                return lm.beam_search(ids_x, feats, T + new, scorer, attention_mask=mask_x, use_cache=True)

        def greedy():
            with auto():
                return lm.greedy_search(ids, feats, T + 1, attention_mask=mask, use_cache=True)

        beam(1), beam(n), greedy()
        t = {"beam_first": [], "beam_all": [], "greedy_first": []}
        for _ in range(args.runs):
            t["beam_first"].append(timed(lambda: beam(1)))
            t["greedy_first"].append(timed(greedy))
            t["beam_all"].append(timed(lambda: beam(n)))
        med = {k: statistics.median(v) for k, v in t.items()}
        rows.append({"T": T, "new_tokens": n, **{k + "_ms": med[k] for k in med}, "beam_over_greedy": med["beam_first"] / med["greedy_first"],
                     "spread": {k: [min(v), max(v)] for k, v in t.items()}})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    # a BOS prompt of ones replays the captured steps of generate(num_beams=4)
    L = 1 + n
    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(7)).to(DEV)
    bos = torch.full((S * NB, 1), BOS, dtype=torch.int64, device=DEV)
    ones = torch.ones_like(bos)

    def gen():
        with auto():
            return lm.generate(feats, max_length=L, num_beams=NB)

    def bos_beam():
        with auto():
            return lm.beam_search(bos, feats, L, scorer, attention_mask=ones, use_cache=True)

    same = bool(torch.equal(gen(), bos_beam()))
    t = {"generate": [], "bos_prompt": [], "generate_again": []}
    for _ in range(args.runs):
        t["generate"].append(timed(gen))
        t["bos_prompt"].append(timed(bos_beam))
        t["generate_again"].append(timed(gen))
    bos_res = {"max_length": L, "same_ids": same, **{k + "_ms": statistics.median(v) for k, v in t.items()},
               "spread": {k: [min(v), max(v)] for k, v in t.items()}}
    res = {"runs": args.runs, "new_tokens": n, "items": S, "num_beams": NB, "device": torch.cuda.get_device_name(0), "cases": rows, "bos": bos_res}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Beam search from a prompt: one prompt pass per region\n\n"
                    f"`python tools/prompt_beam_bench.py --runs {args.runs} --new-tokens {n}` on {res['device']}; 'bench' weights, {S} items x "
                    f"{NB} beams under fp16 autocast, medians of {args.runs} calls after one warm-up each, host wall time around a "
                    "synchronised call, ms.  'beam first' = `LanguageModel.beam_search` ending with the first ranking (max_length = T + 1: "
                    f"image slot, one prompt pass over {S} x T token rows, lm_head over {S * NB} rows, ranking, the scorer on the host); "
                    f"'beam all' = {n} generated tokens; 'greedy first' = `LanguageModel.greedy_search` at the same S and T ending with its "
                    "first token (the prompt pass of the parent commit).  Expanding the prompts would cost about num_beams x 'greedy "
                    "first'; the last column is beam first / greedy first.\n\n"
                    "| T | beam first | greedy first | beam / greedy | beam all |\n|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['T']} | {r['beam_first_ms']:.1f} | {r['greedy_first_ms']:.1f} | {r['beam_over_greedy']:.2f} | {r['beam_all_ms']:.1f} |\n")
            f.write("\nmin .. max of the timed calls, ms:\n\n")
            for r in rows:
                f.write(f"- T = {r['T']}: " + ", ".join(f"{k} {v[0]:.1f} .. {v[1]:.1f}" for k, v in r["spread"].items()) + "\n")
            f.write(f"\n## A BOS prompt against generate(num_beams={NB})\n\nmax_length {L}, alternating in one process; the BOS call replays the "
                    f"captured beam steps of `generate` (same ids: {same}).\n\n| call | median | min .. max |\n|---|---|---|\n")
            for k in ("generate", "bos_prompt", "generate_again"):
                f.write(f"| {k} | {bos_res[k + '_ms']:.1f} | {bos_res['spread'][k][0]:.1f} .. {bos_res['spread'][k][1]:.1f} |\n")


if __name__ == "__main__":
    main()
