"""Timings behind profiles/rolling_prompt.md: what prompts in a rolling session cost.  Synthetic weights, random
feature rows and prompts from a seed; every window ends in a device synchronise (``advance`` waits; submits are followed by one).
  --mode step     ms per step of a session WITHOUT prompts (max_prompt_length is not passed at all, so the same file measures a tree
                  from before prompts): ``--rows`` decoder rows kept full from a stream of 8 x rows sentences, ``--steps`` steps per
                  window, ``--windows`` windows after one warm-up window.
  --mode submit   ms of ``submit(feats, prompt_ids)`` for ``--count`` prompts of ``--prompt`` tokens (enqueue time, and the time
                  until the device has finished the submit), against the same submit without prompts, and of the first step
                  behind it - the step whose hand-out ran in the submit, so its own refill launch finds an empty list - against
                  a later step.
  --mode stream   steps and wall time for ``--count`` sentences through ``--rows`` rows with ``--prompt``-token prompts, beside
                  the same sentences without prompts, at ``--max-length`` for both (the prompt counts).
One JSON line per configuration."""
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


def mode_step(args, lm):
    R, L = args.rows, args.max_length
    g = torch.Generator().manual_seed(3)
    feats = torch.randn((8 * R, 1024), generator=g).to(DEV)
    with lm.open_rolling(L, rows=R, capacity=8 * R) as ses:
        ses.submit(feats)
        ses.advance(args.steps)
        ms = []
        for _ in range(args.windows):
            ses.collect()
            room = ses.capacity - (ses.submitted - ses.watermark)
            if room >= R:      # keep the rows full: refill the ring outside the timed window
                ses.submit(feats[:room])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            launched = ses.advance(args.steps)
            ms.append((time.perf_counter() - t0) * 1e3 / max(launched, 1))
            assert launched == args.steps and ses.unfinished >= R, "the stream ran dry inside the timed windows"
        return {"rows": R, "steps_per_window": args.steps, "ms_per_step_median": statistics.median(ms), "ms_per_step_min": min(ms),
                "ms_per_step_max": max(ms), "windows": len(ms)}


def mode_submit(args, lm):
    R, L, m, P = args.rows, args.max_length, args.count, args.prompt
    g = torch.Generator().manual_seed(5)
    feats = torch.randn((m, 1024), generator=g).to(DEV)
    prompts = torch.randint(0, 50000, (m, P), generator=g)
    out = {"rows": R, "count": m, "prompt_tokens": P}
    for key, kw in (("plain", {}), ("prompted", dict(prompt_ids=prompts))):
        enq, done, first, later = [], [], [], []
        for _ in range(args.windows + 1):
            with lm.open_rolling(L, rows=R, capacity=m, max_prompt_length=P) as ses:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ses.submit(feats, **kw)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                ses.advance(1)
                t3 = time.perf_counter()
                ses.advance(1)
                ses.advance(1)
                t4 = time.perf_counter()
                ses.advance(1)
                t5 = time.perf_counter()
                enq.append((t1 - t0) * 1e3); done.append((t2 - t0) * 1e3); first.append((t3 - t2) * 1e3); later.append((t5 - t4) * 1e3)
        for name, v in (("submit_enqueue_ms", enq), ("submit_done_ms", done), ("first_step_ms", first), ("later_step_ms", later)):
            out[f"{key}_{name}"] = statistics.median(v[1:])      # (the first round is the warm-up: graph capture, work space)
    return out


def mode_stream(args, lm):
    R, L, S, P = args.rows, args.max_length, args.count, args.prompt
    g = torch.Generator().manual_seed(7)
    feats = torch.randn((S, 1024), generator=g).to(DEV)
    prompts = torch.randint(0, 50000, (S, P), generator=g)
    out = {"rows": R, "sequences": S, "prompt_tokens": P, "max_length": L}
    for key, kw in (("plain", {}), ("prompted", dict(prompt_ids=prompts))):
        ms, steps, toks = [], 0, 0
        for _ in range(args.windows + 1):
            with lm.open_rolling(L, rows=R, capacity=S, max_prompt_length=P) as ses:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ses.submit(feats, **kw)
                ses.advance()
                ms.append((time.perf_counter() - t0) * 1e3)
                steps = ses.steps
                toks = sum(it[1].shape[0] for it in ses.collect())
        out[f"{key}_ms"] = statistics.median(ms[1:])
        out[f"{key}_steps"] = steps
        out[f"{key}_tokens"] = toks
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "submit", "stream"), required=True)
    ap.add_argument("--rows", type=int, default=70)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="bf16")
    ap.add_argument("--weights", choices=("bench", "ragged"), default="bench")
    ap.add_argument("--max-length", type=int, default=40)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--count", type=int, default=50)
    ap.add_argument("--prompt", type=int, default=8)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rolling_prompt_bench: no GPU (a timing needs one; there is no CPU fallback)")
    model = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    model.load_state_dict(synth.make_state_dict(0, args.weights))
    model.to(DEV).eval()
    ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if args.dtype == "bf16" else contextlib.nullcontext
    with torch.no_grad(), ctx():
        res = {"step": mode_step, "submit": mode_submit, "stream": mode_stream}[args.mode](args, model.language_model)
    res.update(mode=args.mode, dtype=args.dtype, weights=args.weights, tag=args.tag, data="synthetic weights, random feature rows")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
