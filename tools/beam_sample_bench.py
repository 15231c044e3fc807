"""The beam-sampling ranking beside the plain beam ranking it stands in for, in the same process, and the whole beam-sampling call
beside plain beam search.  Writes profiles/beam_sample.md.

  python tools/beam_sample_bench.py           the driver: both measurements below as child processes under their own time limit,
                                              one after the other; stops at the first child that fails
  python tools/beam_sample_bench.py rank      on the same random logits [rows][50272]: rgrg_debug_beam_sample_rank (row + item
                                              kernel, one call) and rgrg_debug_beam_row_topk + rgrg_debug_beam_merge (one call each),
                                              at 116 rows (29 items x 4 beams) and 464 rows (29 x 16); HIP events around each call,
                                              minimum and median of 40 calls after 5
  python tools/beam_sample_bench.py step      29 items x 4 beams = 116 rows under fp16 autocast, max_length 32: whole
                                              LanguageModel.beam_sample and generate(num_beams=4) calls (graph replays, host scorer
                                              included), ms per call over 5 calls after 2, divided by the steps the call ran

The plain beam step is untouched by beam sampling, so the plain figures of this process are the parent's.  Each child prints one
JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
V, LD, ITEMS = 50257, 50272, 29
PARAMS = (("T=1, no filter", 1.0, 0, 1.0), ("T=0.8, top_k=50, top_p=0.95", 0.8, 50, 0.95), ("T=1, top_p=0.9", 1.0, 0, 0.9))


def rank():
    import torch
    from rgrg_amd import _hip
    lib = _hip.load()
    dev = torch.device("cuda", 0)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(call):
        us = []
        for it in range(45):
            ev0.record()
            _hip.check(call(), "ranking launch")
            ev1.record()
            torch.cuda.synchronize()
            if it >= 5:
                us.append(ev0.elapsed_time(ev1) * 1e3)
        return {"min": min(us), "median": statistics.median(us)}

    out = {}
    for nb in (4, 16):
        R, K = ITEMS * nb, 2 * nb
        g = torch.Generator(device=dev).manual_seed(nb)
        logits = torch.randn((R, LD), device=dev, generator=g) * 3.0
        bs = -torch.rand((R,), device=dev, generator=g) * 5.0
        f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        i = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        rmax, rls, tv, tt, sc, ot, ob = f(R), f(R), f(R, 32), i(R, 32), f(ITEMS, K), i(ITEMS, K), i(ITEMS, K)
        rk, rs, rt, scratch = f(R, 32), f(R, 32), i(R, 32), f(ITEMS, nb * K)
        p = lambda t: t.data_ptr()  # noqa: E731
        res = {"plain_row_topk": timed(lambda: lib.rgrg_debug_beam_row_topk(p(logits), LD, V, R, K, p(rmax), p(rls), p(tv), p(tt), None)),
               "plain_merge": timed(lambda: lib.rgrg_debug_beam_merge(p(rmax), p(rls), p(tv), p(tt), p(bs), ITEMS, nb, V, p(scratch), p(sc),
                                                                      p(ot), p(ob), None))}
        for name, T, k, tp in PARAMS:
            res[name] = timed(lambda: lib.rgrg_debug_beam_sample_rank(p(logits), LD, V, ITEMS, nb, p(bs), T, k, tp, 7, 3, 0, p(sc), p(ot), p(ob),
                                                                      p(rk), p(rs), p(rt), None))
        out[str(R)] = res
    print(json.dumps({"rank": out}))


def step():
    import torch
    import rgrg_amd
    from rgrg_amd import synth
    model = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    model.load_state_dict(synth.make_state_dict(0, "bench"))
    model.to("cuda:0").eval()
    lm = model.language_model
    feats = torch.randn((ITEMS, 1024), generator=torch.Generator().manual_seed(99)).to("cuda:0")
    L = 32
    calls = {"plain beam search": lambda: lm.generate(feats, max_length=L, num_beams=4)}
    for name, T, k, tp in PARAMS:
        calls["beam sampling, " + name] = (lambda T=T, k=k, tp=tp: lm.beam_sample(feats, L, 4, temperature=T, top_k=k, top_p=tp, seed=5))
    out = {}
    with torch.autocast("cuda", dtype=torch.float16):
        for name, call in calls.items():
            for _ in range(2):
                ids = call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                ids = call()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / 5
            steps = ids.shape[1] - 1 if ids.shape[1] < L else L - 1   # the loop ran until the longest hypothesis ended, or to max_length
            out[name] = {"ms_per_call": ms, "steps": steps, "ms_per_step": ms / steps}
    print(json.dumps({"step": out}))


def driver(limit, out_path):
    runs = {}
    for what in ("rank", "step"):
        res = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), what], capture_output=True, text=True)
        if res.returncode != 0:   # a fault, an abort or the time limit: nothing else is started
            sys.stderr.write(res.stderr[-3000:])
            sys.exit(f"beam_sample_bench {what} ended with status {res.returncode}: stopping")
        runs[what] = json.loads(res.stdout.strip().splitlines()[-1])[what]
    L = ["# Beam-sampling ranking beside the plain beam ranking; whole calls beside plain beam search", "",
         "`python tools/beam_sample_bench.py` on one MI355X.  The plain beam step is untouched by beam sampling: its figures here are the parent's.", "",
         "## The ranking alone, random logits [rows][50272], us per call: minimum (median) of 40", "",
         "| ranking | 116 rows (29 x 4 beams) | 464 rows (29 x 16 beams) |", "|---|---|---|"]
    names = list(runs["rank"]["116"])
    for n in names:
        cell = lambda R: f"{runs['rank'][R][n]['min']:.1f} ({runs['rank'][R][n]['median']:.1f})"  # noqa: E731
        label = {"plain_row_topk": "plain: beam_row_topk_kernel", "plain_merge": "plain: beam_merge_kernel"}.get(n, "beam sampling (row + item kernel), " + n)
        L.append(f"| {label} | {cell('116')} | {cell('464')} |")
    L += ["", "## Whole calls, 116 rows, fp16 autocast, max_length 32 (graph replays, host scorer included)", "",
          "| call | ms per call | steps | ms per step |", "|---|---|---|---|"]
    for n, r in runs["step"].items():
        L.append(f"| {n} | {r['ms_per_call']:.2f} | {r['steps']} | {r['ms_per_step']:.3f} |")
    text = "\n".join(L) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", choices=("rank", "step"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "beam_sample.md"))
    a = ap.parse_args()
    {"rank": rank, "step": step, None: lambda: driver(a.limit, a.out)}[a.what]()
