"""Prompted greedy search: the batched prompt pass against feeding the prompt through forward(use_cache=True).
Usage: python tools/prompt_bench.py [--runs 5] [--new-tokens 8] [--out FILE.md]
For T = 4, 16, 64 prompt tokens at 29 rows in fp32 and at 928 rows under bf16 autocast ('bench' weights: no row emits EOS):
  (a) LanguageModel.greedy_search - time of a call that stops after the first generated token (max_length = T + 1: image slot,
      prompt pass, lm_head + arg-max over S rows) and of a call that generates --new-tokens tokens;
  (b) the same prompt through LanguageModel.forward(use_cache=True) - T single-position steps, [S,T,V] logits - then arg-max on the
      host and single-token forward(past_key_values=...) steps: the only way to condition on a prefix before; fp32 whatever the
      autocast state.
One warm-up of each, then --runs timed calls each (alternating), medians.  Prints one JSON line; --out writes a markdown table."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgrg_amd  # noqa: E402
from rgrg_amd import synth  # noqa: E402

DEV = "cuda:0"


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
    rows = []
    for S, dtype in ((29, "f32"), (928, "bf16")):
        for T in (4, 16, 64):
            g = torch.Generator().manual_seed(1000 * S + T)
            ids = torch.randint(0, 50000, (S, T), generator=g).to(DEV)
            mask = torch.ones((S, T), dtype=torch.int64, device=DEV)
            feats = torch.randn((S, 1024), generator=g).to(DEV)
            ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if dtype == "bf16" else contextlib.nullcontext

            def batched(new):
                with ctx():
                    return lm.greedy_search(ids, feats, T + new, attention_mask=mask, use_cache=True)

            def stepwise(new):
                with torch.no_grad():
                    logits, past = lm(ids, mask, feats, return_loss=False, use_cache=True)
                    tok = logits[:, -1].argmax(-1, keepdim=True)
                    del logits
                    am = mask
                    for _ in range(new - 1):
                        am = torch.cat([am, am.new_ones((S, 1))], dim=1)
                        logits, past = lm(tok, am, feats, return_loss=False, past_key_values=past, use_cache=True)
                        tok = logits[:, -1].argmax(-1, keepdim=True)
                return tok

            batched(1), batched(n), stepwise(1), stepwise(n)
            t = {"a_first": [], "a_all": [], "b_first": [], "b_all": []}
            for _ in range(args.runs):
                t["a_first"].append(timed(lambda: batched(1)))
                t["b_first"].append(timed(lambda: stepwise(1)))
                t["a_all"].append(timed(lambda: batched(n)))
                t["b_all"].append(timed(lambda: stepwise(n)))
            med = {k: statistics.median(v) for k, v in t.items()}
            rows.append({"rows": S, "dtype": dtype, "T": T, "new_tokens": n, **{k + "_ms": med[k] for k in med},
                         "first_speedup": med["b_first"] / med["a_first"], "all_speedup": med["b_all"] / med["a_all"],
                         "spread": {k: [min(v), max(v)] for k, v in t.items()}})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    res = {"runs": args.runs, "new_tokens": n, "device": torch.cuda.get_device_name(0), "cases": rows}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Prompted greedy search: batched prompt pass against forward(use_cache=True)\n\n"
                    f"`python tools/prompt_bench.py --runs {args.runs} --new-tokens {n}` on {res['device']}; 'bench' weights, medians of "
                    f"{args.runs} calls after one warm-up each, host wall time around a synchronised call, ms.  (a) = "
                    "`LanguageModel.greedy_search` (one batched pass over the S x T prompt rows into the decode cache; bf16 autocast at 928 "
                    "rows); (b) = the prompt through `forward(use_cache=True)` (T single-position steps, fp32 in both configurations) and "
                    "single-token `forward(past_key_values=...)` steps.  'first' = a call that ends with the first generated token, "
                    f"'all' = {n} generated tokens.\n\n"
                    "| rows | mode of (a) | T | (a) first | (b) first | (b)/(a) | (a) all | (b) all | (b)/(a) |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['rows']} | {r['dtype']} | {r['T']} | {r['a_first_ms']:.1f} | {r['b_first_ms']:.1f} | {r['first_speedup']:.2f} | "
                        f"{r['a_all_ms']:.1f} | {r['b_all_ms']:.1f} | {r['all_speedup']:.2f} |\n")
            f.write("\nmin .. max of the timed calls, ms:\n\n")
            for r in rows:
                f.write(f"- {r['rows']} rows, T = {r['T']}: " + ", ".join(f"{k} {v[0]:.1f} .. {v[1]:.1f}" for k, v in r["spread"].items()) + "\n")


if __name__ == "__main__":
    main()
