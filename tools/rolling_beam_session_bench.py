"""Rolling beam sessions on one GPU, SYNTHETIC weights and images (``ragged``: its length distribution is not that
of a trained model).  The scripts' mode: 4 beams, early stopping, fp16 autocast.  One JSON line per measurement; every number is
the median of ``--runs`` timed calls after one warm-up call, and a comparison takes fresh processes that alternate between the two
sides (profiles/rolling_beam_session.md).

  --what oneshot   ONE ``beam_search_rolling`` call over the selected regions of ``--images`` images on ``--rows`` rows.  Uses nothing
                   this change adds, so it also runs on the parent tree.
  --what session   the same regions through one session: open (capacity = all regions), submit everything, ``advance()``,
                   ``collect()``, close - all inside the timed call.  The same schedule as ``oneshot``.
  --what wait      what a tree without beam sessions offers a study that arrives while another is being decoded: the call in
                   flight, ``generate_rolling_beam(A)``, drains, then ``generate_rolling_beam(B)``.  Times both calls; with B arriving
                   when A's call is at the fraction ``--arrive`` of its steps, B's result is there (1 - arrive) * ms_A + ms_B later.
                   Also runs on the parent tree.
  --what arrival   ``ReportGenerationModel.open_rolling(num_beams=4)``: A is submitted, ``advance`` runs ``--arrive`` of the steps A alone
                   takes, B is submitted, and ``advance(--poll)`` / ``collect()`` alternate until B's ticket is delivered: the time from
                   B's submit (its detector pass included, as in ``wait``) to its result, and the steps that took."""
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


def timed(fn, runs):
    fn()   # warm-up: decoder, graph capture, work space
    torch.cuda.synchronize()
    out, ms = None, []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms), [round(m, 3) for m in ms]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=("oneshot", "session", "wait", "arrival"), required=True)
    ap.add_argument("--images", type=int, default=8, help="oneshot / session: images whose selected regions are decoded")
    ap.add_argument("--rows", type=int, default=116)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--max-length", type=int, default=128)
    ap.add_argument("--dtype", choices=("f32", "f16", "bf16"), default="f16")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arrive", type=float, default=0.5)
    ap.add_argument("--poll", type=int, default=4)
    args = ap.parse_args()
    model = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    model.load_state_dict(synth.make_state_dict(0, "ragged"))
    model.to("cuda:0").eval()
    lm = model.language_model
    nb, L, R = args.beams, args.max_length, args.rows
    ctx = ((lambda: torch.autocast("cuda", dtype={"f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]))
           if args.dtype != "f32" else contextlib.nullcontext)
    base = {"what": args.what, "beams": nb, "rows": R, "max_length": L, "dtype": args.dtype, "data": "synthetic weights and images (ragged)"}

    def out(**kw):
        print(json.dumps(dict(base, **kw)), flush=True)

    with torch.no_grad(), ctx():
        if args.what in ("oneshot", "session"):
            images = synth.make_images(args.images, 1234).to("cuda:0")
            _, _, top, cd = model.object_detector(images)
            _, feats = model.binary_classifier_region_selection(top, cd, return_loss=False)
            feats = feats.float().contiguous()
            S = int(feats.shape[0])
            if args.what == "oneshot":
                ids, ms, all_ms = timed(lambda: lm.beam_search_rolling(feats, L, nb, rows=R, early_stopping=True), args.runs)
                steps, collect_ms = int(model.engine().last_rolling_steps), None
            else:
                state = {}

                def run():
                    with lm.open_rolling(L, rows=R, capacity=S, num_beams=nb, early_stopping=True) as ses:
                        ses.submit(feats)
                        ses.advance()
                        t0 = time.perf_counter()
                        items = ses.collect()
                        state.update(steps=ses.steps, collect_ms=(time.perf_counter() - t0) * 1e3)
                    return items
                items, ms, all_ms = timed(run, args.runs)
                assert [q for q, _ in items] == list(range(S))
                steps, collect_ms = state["steps"], round(state["collect_ms"], 3)
                width = max(v.shape[1] for _, v in items)
                ids = torch.full((S, width), 50256, dtype=torch.int64)
                for q, v in items:
                    ids[q, :v.shape[1]] = v[0].cpu()
            out(regions=S, steps=steps, ms=round(ms, 3), ms_runs=all_ms, ms_per_step=round(ms / max(steps, 1), 4),
                collect_ms_included=collect_ms, ids_checksum=int(ids.cpu().sum()), width=int(ids.shape[1]))
            return
        a, b = synth.make_images(2, 1234).to("cuda:0").split(1)
        kw = dict(num_beams=nb, early_stopping=True)
        if args.what == "wait":
            res_a, ms_a, runs_a = timed(lambda: model.generate_rolling_beam(a, L, nb, rows=R, early_stopping=True), args.runs)
            steps_a = int(model.engine().last_rolling_steps)
            res_b, ms_b, runs_b = timed(lambda: model.generate_rolling_beam(b, L, nb, rows=R, early_stopping=True), args.runs)
            steps_b = int(model.engine().last_rolling_steps)
            out(regions_a=int(res_a[0].shape[0]), regions_b=int(res_b[0].shape[0]), steps_a=steps_a, steps_b=steps_b, ms_a=round(ms_a, 3),
                ms_a_runs=runs_a, ms_b=round(ms_b, 3), ms_b_runs=runs_b, arrive=args.arrive,
                ms_from_arrival_to_result_b=round((1 - args.arrive) * ms_a + ms_b, 3),
                steps_from_arrival_to_result_b=steps_a - int(args.arrive * steps_a) + steps_b)
            return
        with model.open_rolling(L, rows=R, **kw) as ses:   # the steps A takes alone
            ses.submit(a)
            ses.advance()
            steps_a = ses.session.steps
        half = int(args.arrive * steps_a)
        state = {}

        def run():
            with model.open_rolling(L, rows=R, **kw) as ses:
                ses.submit(a)
                ses.advance(half)
                done = dict(ses.collect())
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tb = ses.submit(b)
                at = ses.session.steps
                while tb not in done:
                    ses.advance(args.poll)
                    done.update(ses.collect())
                torch.cuda.synchronize()
                state.update(ms=(time.perf_counter() - t0) * 1e3, steps=ses.session.steps - at)
                ses.advance()
                done.update(ses.collect())
            state.setdefault("all", []).append(round(state["ms"], 3))
            return done
        done, _, _ = timed(run, args.runs)
        runs_b = state["all"][1:]   # (the first entry is the warm-up)
        out(regions_a=int(done[0][0].shape[0]), regions_b=int(done[1][0].shape[0]), steps_a_alone=steps_a, arrive=args.arrive,
            b_submitted_after_steps=half, poll=args.poll, ms_from_arrival_to_result_b=round(statistics.median(runs_b), 3),
            ms_runs=runs_b, steps_from_arrival_to_result_b=state["steps"])


if __name__ == "__main__":
    main()
