"""The e4m3 K/V cache against the 16-bit cache it replaces, in the same process: the decode-attention kernel alone and the whole
many-sequence decode step.  Writes profiles/kv8_step.md.

  python tools/kv8_bench.py                 the driver: every measurement below as a child process under its own time limit, one
                                            after the other, `--repeats` times each; stops at the first child that fails
  python tools/kv8_bench.py kernel          both debug hooks (rgrg_debug_attn_decode kv16 / rgrg_debug_attn_decode_kv8) at S x H =
                                            928 x 16 over 2 .. 129 keys; 8 cache sets in rotation (4 GB / 2 GB: nothing stays in
                                            the 256 MiB last-level cache between launches, as in the step's 24 layers)
  python tools/kv8_bench.py step            928 rows under bf16 autocast: rgrg_decoder_trace_step at 65 and 129 keys (eager step,
                                            first launch to the arg-max's end) and whole generate() calls of 128 tokens (graph
                                            replays), for the bf16 and for the e4m3 cache

Each child prints one JSON line.  HBM fraction = K/V bytes of a launch / time / 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
S, H, SLOTS, SETS = 928, 16, 132, 8
KEYS = (2, 17, 33, 65, 97, 129)
HBM = 8.0e12


def _fit(xs, ys):
    n = len(xs)
    mx, my = sum(xs) / n, sum(ys) / n
    b = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    return my - b * mx, b


def kernel():
    import torch
    from rgrg_amd import _hip
    lib = _hip.load()
    dev = torch.device("cuda", 0)
    D = H * 64
    g = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn((S, 3 * D), device=dev, generator=g)
    out16 = torch.empty((S, D), dtype=torch.int16, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    n = S * H * SLOTS * 64
    planes16 = [(torch.randn(n, device=dev, generator=g).to(torch.bfloat16), torch.randn(n, device=dev, generator=g).to(torch.bfloat16)) for _ in range(SETS)]
    planes8 = [(k.float().to(torch.float8_e4m3fn), v.float().to(torch.float8_e4m3fn)) for k, v in planes16]
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(fmt8, nkeys, iters):
        step.fill_(nkeys - 2)
        planes = planes8 if fmt8 else planes16
        for it in range(-SETS, iters):
            if it == 0:
                ev0.record()
            k, v = planes[it % SETS]
            if fmt8:
                rc = lib.rgrg_debug_attn_decode_kv8(qkv.data_ptr(), 3 * D, k.data_ptr(), v.data_ptr(), step.data_ptr(), None, out16.data_ptr(),
                                                    S, H, SLOTS, None, None, 0, 0, None)
            else:
                rc = lib.rgrg_debug_attn_decode(qkv.data_ptr(), 3 * D, k.data_ptr(), v.data_ptr(), step.data_ptr(), None, out16.data_ptr(),
                                                S, H, SLOTS, None, None, 1, 0, 0, 0, 0, None)
            _hip.check(rc, "attention launch")
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) * 1e3 / iters   # us per launch

    res = {"bf16": {}, "e4m3": {}}
    for nkeys in KEYS:
        for name, fmt8 in (("bf16", False), ("e4m3", True), ("bf16", False), ("e4m3", True)):   # interleaved: clocks and thermals shared
            res[name].setdefault(nkeys, []).append(run(fmt8, nkeys, 48))
    out = {}
    for name, esz in (("bf16", 2), ("e4m3", 1)):
        us = {k: min(v) for k, v in res[name].items()}
        a, b = _fit(list(us), list(us.values()))
        out[name] = {"us": us, "intercept_us": a, "slope_us_per_key": b,
                     "hbm_fraction": {k: S * H * k * 64 * esz * 2 / (t * 1e-6) / HBM for k, t in us.items()}}
    print(json.dumps({"kernel": out}))


def step():
    import torch
    import rgrg_amd
    from rgrg_amd import _hip, synth
    model = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    model.load_state_dict(synth.make_state_dict(0, "bench"))
    model.to("cuda:0").eval()
    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(99)).to("cuda:0")
    lib = _hip.load()
    lm = model.language_model
    out = {}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for name in ("bf16", "e4m3", "bf16", "e4m3"):
            lm.set_kv_cache_dtype("fp8_e4m3" if name == "e4m3" else None)
            lm.generate(feats, max_length=130)   # the decoder in this format, 131 slots
            torch.cuda.synchronize()
            eng = lm.engine()
            assert eng.kv_format_in_use(S) == (3 if name == "e4m3" else 1)
            r = out.setdefault(name, {"step_us": {65: [], 129: []}, "generate_ms_per_step": []})
            for nkeys in (65, 129):
                recs, n = (C.c_float * (3 * 4096))(), C.c_int(0)
                _hip.check(lib.rgrg_decoder_trace_step(eng._decoder, S, nkeys, 5, recs, 4096, C.byref(n)), "rgrg_decoder_trace_step")
                r["step_us"][nkeys].append(max(recs[3 * i + 2] for i in range(n.value)) * 1e3)
            lm.generate(feats, max_length=128)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                lm.generate(feats, max_length=128)
            torch.cuda.synchronize()
            r["generate_ms_per_step"].append((time.perf_counter() - t0) * 1e3 / 3 / 127)
    lm.set_kv_cache_dtype(None)
    print(json.dumps({"step": out}))


def _spread(v, nd=2):
    return f"{statistics.median(v):.{nd}f} ({min(v):.{nd}f} - {max(v):.{nd}f})"


def driver(repeats, limit, out_path):
    runs = {"kernel": [], "step": []}
    for what in ("kernel", "step"):
        for _ in range(repeats):
            res = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), what], capture_output=True, text=True)
            if res.returncode != 0:   # a fault, an abort or the time limit: nothing else is started
                sys.stderr.write(res.stderr[-3000:])
                sys.exit(f"kv8_bench {what} ended with status {res.returncode}: stopping")
            runs[what].append(json.loads(res.stdout.strip().splitlines()[-1])[what])
    L = ["# e4m3 K/V cache against the bf16 cache: kernel alone and whole decode step", "",
         f"`python tools/kv8_bench.py --repeats {repeats}` on one MI355X; every figure: median (min - max) over {repeats} processes.", "",
         f"## Kernel alone, S x H = {S} x {H}, out16, {SETS} cache sets in rotation", "",
         "| keys | bf16 us | e4m3 us | bf16 HBM fraction | e4m3 HBM fraction |", "|---|---|---|---|---|"]
    K = runs["kernel"]
    for k in KEYS:
        g = lambda f, q: _spread([r[f][q][str(k)] for r in K])  # noqa: E731
        L.append(f"| {k} | {g('bf16', 'us')} | {g('e4m3', 'us')} | {g('bf16', 'hbm_fraction')} | {g('e4m3', 'hbm_fraction')} |")
    L += ["", "| fit over the key counts | bf16 | e4m3 |", "|---|---|---|"]
    for q, label in (("intercept_us", "intercept, us"), ("slope_us_per_key", "slope, us per key")):
        L.append(f"| {label} | {_spread([r['bf16'][q] for r in K], 4)} | {_spread([r['e4m3'][q] for r in K], 4)} |")
    sl16, sl8 = [r["bf16"]["slope_us_per_key"] for r in K], [r["e4m3"]["slope_us_per_key"] for r in K]
    L += ["", f"Slope: e4m3 {statistics.median(sl8):.4f} us per key (max {max(sl8):.4f}), bf16 {statistics.median(sl16):.4f} (min {min(sl16):.4f}): "
          + ("lower by more than the run-to-run spread." if max(sl8) < min(sl16) else "NOT lower by more than the run-to-run spread."), "",
          f"## Whole step, {S} rows, bf16 autocast", "",
          "| | bf16 cache | e4m3 cache |", "|---|---|---|"]
    T = runs["step"]
    flat = lambda f, get: [x for r in T for x in get(r[f])]  # noqa: E731
    for nk in ("65", "129"):
        L.append(f"| eager step at {nk} keys, ms | {_spread([x / 1e3 for x in flat('bf16', lambda r: r['step_us'][nk])])} | "
                 f"{_spread([x / 1e3 for x in flat('e4m3', lambda r: r['step_us'][nk])])} |")
    L.append(f"| generate() of 128 tokens, ms per step (graph replays) | {_spread(flat('bf16', lambda r: r['generate_ms_per_step']))} | "
             f"{_spread(flat('e4m3', lambda r: r['generate_ms_per_step']))} |")
    text = "\n".join(L) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", choices=("kernel", "step"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kv8_step.md"))
    a = ap.parse_args()
    {"kernel": kernel, "step": step, None: lambda: driver(a.repeats, a.limit, a.out)}[a.what]()
