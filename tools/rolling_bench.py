"""The decoder alone on the bench's region rows, lock step against rolling batch (no detector in the timed part), like
tools/decode_only.py: the feature rows the detector and the selection produce for the bench's 32 synthetic images, repeated
``--repeat`` times as one stream of sequences, decoded under bf16 autocast at ``--max-length`` either by ``LanguageModel.generate``
- one call per repeat, every call in lock step over all its rows (``--mode generate``, which also runs on a tree without
``generate_rolling``) - or by ONE ``LanguageModel.generate_rolling`` call over the stream on ``--rows`` decoder rows (``--mode
rolling``; several ``--rows`` values = several configurations in one process).
Sampling: ``--mode sample`` is ONE ``LanguageModel.sample`` call over the batch with ``--hypotheses`` n sequences per row (lock step over
rows x n; runs on a tree without ``sample_rolling``), ``--mode sample-rolling`` ONE ``LanguageModel.sample_rolling`` call per
``--rows`` value over the same rows and n, under ``--temperature / --top-k / --top-p / --seed``; ``--repeat`` is not used.
Beam search: ``--beams N`` (N > 1, early stopping on) turns ``--mode generate`` into one ``LanguageModel.generate(num_beams=N)`` call per
repeat (lock step over regions x N rows; runs on a tree without ``beam_search_rolling``) and ``--mode rolling`` into ONE
``LanguageModel.beam_search_rolling`` call over the stream of regions per ``--rows`` value (decoder rows: rows // N slots); the JSON
line then carries regions, regions per second and the K/V cache the decoder holds instead of the token figures.  With
``--prefill`` the rolling mode also times, at max_length 2 (one decode step per row hand-out), the call on the unrepeated rows
against the call on the rows repeated n-fold with one hypothesis each: the difference is the prefill the shared image rows save.
Sessions (``--session``): ``--session all`` is ONE rolling session per ``--rows`` value with the whole stream submitted
before the first step (set it against ``--mode rolling`` on the same arguments: the same schedule); ``--session arrivals`` splits the
unrepeated rows into ``--submits`` submits that arrive ``--gap`` steps apart into one session on ``--rows`` rows (timed with
``advance(gap)`` between them; a second pass with ``advance(1)`` gives, per submit, the steps from its arrival to its last sentence);
``--session arrivals-generate`` / ``arrivals-rolling`` are what a tree without sessions offers for the same arrivals - one
``generate()`` / one ``generate_rolling`` per arrival, a call starting when the one before it has returned (they use nothing newer
than ``generate_rolling``, so this file also runs them on such a tree).  ``--requests``: every submit of ``--session
all`` / ``arrivals`` carries request parameters that change no result (the session's max_length, EOS as a stop token).
Usage: python tools/rolling_bench.py --mode rolling --rows 128 256 464 928 [--repeat 4] [--weights bench|ragged] [--runs 3]
Prints one JSON line per configuration: sequences, length histogram, steps executed, the longest sequence's steps, sum of the
steps every sequence needs / rows, ms per call (median of --runs after one warm-up), ms per step, generated tokens per second."""
import argparse
import collections
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

EOS = 50256


def lengths(ids):
    """Tokens of every row, BOS and EOS included (PAD = EOS: the first EOS behind the BOS ends the row)."""
    body = ids[:, 1:]
    is_eos = body == EOS
    first = torch.where(is_eos.any(dim=1), is_eos.float().argmax(dim=1) + 1, torch.full((ids.shape[0],), body.shape[1], device=ids.device))
    return (first + 1).cpu()


def timed(fn, runs):
    fn()   # warm-up: decoder, graph capture, work space
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms), ms


def run_session(args, model, lm, batch, stream, L, report):
    def table(items, total):
        out = torch.full((total, L), EOS, dtype=torch.int64)
        for q, ids in items:
            out[q, :ids.shape[0]] = ids.cpu()
        return out

    req = dict(max_length=L, stop_token_ids=[EOS]) if args.requests else {}   # values that change no result: the request path alone
    if args.session == "all":
        for R in args.rows:
            S = int(stream.shape[0])
            state = {}

            def run():
                with lm.open_rolling(L, rows=R, capacity=S) as ses:   # (open and close are part of the call: the rings are allocated)
                    ses.submit(stream, **req)
                    ses.advance()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    items = ses.collect()
                    state.update(steps=ses.steps, items=items, collect_ms=(time.perf_counter() - t0) * 1e3)
            _, ms, all_ms = timed(run, args.runs)
            lens = lengths(table(state["items"], S))
            report({"rows": R, "work_steps_per_row": round(int((lens - 1).sum()) / R, 2), "collect_ms_included": round(state["collect_ms"], 3)},
                   lens, int(state["steps"]), ms, all_ms)
        return
    chunks = [c.contiguous() for c in torch.chunk(batch, args.submits)]
    total, gap = int(batch.shape[0]), args.gap
    first = [sum(int(c.shape[0]) for c in chunks[:i]) for i in range(len(chunks))]
    for R in (args.rows if args.session != "arrivals-generate" else [0]):
        if args.session == "arrivals":
            def run(step=gap, latency=None):
                items, clock = [], 0
                with lm.open_rolling(L, rows=R, capacity=total) as ses:
                    def tick(k):
                        nonlocal clock
                        for _ in range(0, k, step):
                            clock += ses.advance(min(step, k))
                            got = ses.collect()
                            items.extend(got)
                            if latency is not None:
                                for q, _ids in got:
                                    i = max(j for j in range(len(first)) if first[j] <= q)
                                    latency[i] = max(latency[i], clock - i * gap)
                    for c in chunks:
                        ses.submit(c, **req)
                        tick(gap)
                    while ses.unfinished:
                        tick(gap if latency is None else 1)
                    return items, ses.steps
            (items, steps), ms, all_ms = timed(run, args.runs)
            lat = [0] * len(chunks)
            run(step=1, latency=lat)
            report({"rows": R, "sequences": total, "repeat": 1, "submits": len(chunks), "gap_steps": gap,
                    "steps_from_arrival_to_last_sentence": lat},
                   lengths(table(items, total)), int(steps), ms, all_ms)
        else:
            def run():
                outs, steps = [], []
                for c in chunks:
                    if args.session == "arrivals-generate":
                        outs.append(lm.generate(c, max_length=L))
                        steps.append(int(outs[-1].shape[1]) - 1)
                    else:
                        outs.append(lm.generate_rolling(c, L, rows=min(R, int(c.shape[0]))))
                        steps.append(int(model.engine().last_rolling_steps))
                return outs, steps
            (outs, steps), ms, all_ms = timed(run, args.runs)
            lat, end = [], 0
            for i, k in enumerate(steps):   # a call starts when its rows have arrived and the call before it has returned
                end = max(i * gap, end) + k
                lat.append(end - i * gap)
            report({"rows": R or "the arrival's rows", "sequences": total, "repeat": 1, "submits": len(chunks), "gap_steps": gap,
                    "steps_from_arrival_to_last_sentence": lat,
                    "steps_are": "steps of calls on different row counts: not of one duration"},
                   torch.cat([lengths(o) for o in outs]), sum(steps), ms, all_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("generate", "rolling", "sample", "sample-rolling"))
    ap.add_argument("--session", choices=("all", "arrivals", "arrivals-generate", "arrivals-rolling"))
    ap.add_argument("--submits", type=int, default=8)
    ap.add_argument("--gap", type=int, default=8)
    ap.add_argument("--requests", action="store_true", help="--session all / arrivals: every submit carries request parameters (DESIGN.md 7.18)")
    ap.add_argument("--rows", type=int, nargs="*", default=[128, 256, 464, 928])
    ap.add_argument("--repeat", type=int, default=4)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--max-length", type=int, default=128)
    ap.add_argument("--weights", choices=("bench", "ragged"), default="bench")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="bf16")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--hypotheses", type=int, default=4)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--prefill", action="store_true")
    ap.add_argument("--beams", type=int, default=0)
    args = ap.parse_args()
    if (args.mode is None) == (args.session is None):
        ap.error("give either --mode or --session")
    if args.session:
        args.mode = "session-" + args.session
    model = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    model.load_state_dict(synth.make_state_dict(0, args.weights))
    model.to("cuda:0").eval()
    lm = model.language_model
    images = synth.make_images(args.images, 1234).to("cuda:0")
    ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if args.dtype == "bf16" else contextlib.nullcontext
    with torch.no_grad(), ctx():
        _, _, top, cd = model.object_detector(images)
        _, batch = model.binary_classifier_region_selection(top, cd, return_loss=False)
    batch = batch.float().contiguous()
    stream = batch.repeat(args.repeat, 1).contiguous()
    L = args.max_length
    sampling = args.mode.startswith("sample")
    draw = dict(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, seed=args.seed)
    if sampling:
        stream = batch
    base = {"mode": args.mode, "weights": args.weights, "dtype": args.dtype, "max_length": L, "sequences": int(stream.shape[0]),
            "rows_per_image_batch": int(batch.shape[0]), "repeat": args.repeat, "data": "synthetic weights and images"}
    if args.session:
        base["requests"] = bool(args.requests)
    if sampling:
        base.update(draw, hypotheses=args.hypotheses, sequences=int(batch.shape[0]) * args.hypotheses, repeat=1)

    def report(extra, lens, steps, ms, all_ms):
        tokens = int((lens - 1).sum())
        hist = collections.Counter(lens.tolist())
        print(json.dumps(dict(base, **extra, length_histogram={str(k): hist[k] for k in sorted(hist)}, steps=steps,
                              longest_steps=int(lens.max()) - 1, tokens=tokens, ms=round(ms, 3), ms_runs=[round(m, 3) for m in all_ms],
                              ms_per_step=round(ms / max(steps, 1), 4), tokens_per_s=round(tokens / ms * 1e3, 1))), flush=True)

    def report_beams(extra, regions, steps, ms, all_ms):
        cap_s, cap_l = model.engine()._decoder_caps
        cache = model.engine().n_layer * 2 * cap_s * 16 * (cap_l + 1) * 64 * 4
        print(json.dumps(dict(base, **extra, beams=args.beams, regions=regions, steps=steps, ms=round(ms, 3),
                              ms_runs=[round(m, 3) for m in all_ms], ms_per_step=round(ms / max(steps, 1), 4),
                              regions_per_s=round(regions / ms * 1e3, 1), kv_cache_rows=cap_s, kv_cache_mib=round(cache / 2 ** 20, 1))),
              flush=True)

    if args.session:
        with torch.no_grad(), ctx():
            run_session(args, model, lm, batch, stream, L, report)
        return

    if args.beams > 1 and not sampling:
        nb = args.beams
        with torch.no_grad(), ctx():
            if args.mode == "generate":
                outs, ms, all_ms = timed(lambda: [lm.generate(batch, max_length=L, num_beams=nb, early_stopping=True)
                                                  for _ in range(args.repeat)], args.runs)
                # lock step runs until the slowest region is done: the output width is min(longest hypothesis + 1, max_length), so
                # width - 1 counts the iterations exactly when a region ran to max_length and is a lower bound otherwise
                report_beams({"rows": int(batch.shape[0]) * nb, "steps_are": "output width - 1 per call"}, int(stream.shape[0]),
                             sum(int(o.shape[1]) - 1 for o in outs), ms, all_ms)
            else:
                for R in args.rows:
                    _, ms, all_ms = timed(lambda: lm.beam_search_rolling(stream, L, nb, rows=R, early_stopping=True), args.runs)
                    report_beams({"rows": R, "slots": min(R // nb, int(stream.shape[0]))}, int(stream.shape[0]),
                                 int(model.engine().last_rolling_steps), ms, all_ms)
        return

    with torch.no_grad(), ctx():
        if args.mode == "generate":
            def run():
                return [lm.generate(batch, max_length=L) for _ in range(args.repeat)]
            outs, ms, all_ms = timed(run, args.runs)
            lens = torch.cat([lengths(o) for o in outs])
            report({"rows": int(batch.shape[0])}, lens, sum(int(o.shape[1]) - 1 for o in outs), ms, all_ms)
        elif args.mode == "sample":
            ids, ms, all_ms = timed(lambda: lm.sample(batch, L, num_return_sequences=args.hypotheses, **draw), args.runs)
            report({"rows": int(ids.shape[0])}, lengths(ids), int(ids.shape[1]) - 1, ms, all_ms)
        elif args.mode == "sample-rolling":
            n = args.hypotheses
            for R in args.rows:
                ids, ms, all_ms = timed(lambda: lm.sample_rolling(batch, L, rows=R, num_return_sequences=n, **draw), args.runs)
                lens = lengths(ids)
                steps = int(model.engine().last_rolling_steps)
                extra = {"rows": R, "work_steps_per_row": round(int((lens - 1).sum()) / R, 2)}
                if args.prefill:
                    rows_n = batch.repeat_interleave(n, 0).contiguous()
                    _, shared, _ = timed(lambda: lm.sample_rolling(batch, 2, rows=R, num_return_sequences=n, **draw), 5)
                    _, repeated, _ = timed(lambda: lm.sample_rolling(rows_n, 2, rows=R, num_return_sequences=1, **draw), 5)
                    extra.update(ms_max_length_2_shared_rows=round(shared, 3), ms_max_length_2_rows_repeated=round(repeated, 3))
                report(extra, lens, steps, ms, all_ms)
        else:
            for R in args.rows:
                ids, ms, all_ms = timed(lambda: lm.generate_rolling(stream, L, rows=R), args.runs)
                lens = lengths(ids)
                steps = int(model.engine().last_rolling_steps)
                report({"rows": R, "work_steps_per_row": round(int((lens - 1).sum()) / R, 2)}, lens, steps, ms, all_ms)


if __name__ == "__main__":
    main()
