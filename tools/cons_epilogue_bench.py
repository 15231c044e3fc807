"""A/B of the consumer epilogues of the LDS-DMA GEMM (rgrg_amd/csrc/gemm_bf16.hip, RGRG_CONS_EPI) in ONE process: c_fc (Y16, gelu_new,
N = 4096) and c_attn with the K/V-cache epilogue (N = 3072) of the many-sequence decode step, K = 1024, through the launcher the decoder
uses.  The switch is read per launch, so the modes alternate on the same buffers: 0 = run-time activation switch, 1 = the
instantiation with the compile-time activation (64 x 64 tile; c_fc over 923 rows runs on 128 x 64 and has no such instantiation).
Cold weights (a ring of copies larger than the caches, as in a decode step), HIP events around `--launches` launches, `--rounds`
rounds, median per launch in us.

    python tools/cons_epilogue_bench.py --rows 231,923 --modes 0,1
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgrg_amd import _hip  # noqa: E402

K, H, T_SLOTS = 1024, 16, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="231,923")
    ap.add_argument("--modes", default="0,1")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--copies-mb", type=int, default=600)
    ap.add_argument("--fp16", type=int, default=0)
    args = ap.parse_args()
    lib = _hip.load()
    dev = torch.device("cuda", 0)
    t16 = torch.float16 if args.fp16 else torch.bfloat16
    modes = [int(m) for m in args.modes.split(",")]
    for M in (int(r) for r in args.rows.split(",")):
        g = torch.Generator().manual_seed(M)
        x = torch.randn(M, K, generator=g)
        a = x.to(t16).view(torch.int16).to(dev)
        blocks = x.view(M, 16, 64)
        stats = torch.stack((blocks.sum(-1), (blocks * blocks).sum(-1)), dim=-1).contiguous().to(dev)
        for name, N in (("c_fc", 4096), ("c_attn", 3 * H * 64)):
            ncopy = max(2, -(-args.copies_mb * 1_000_000 // (N * K * 2)))
            w = (torch.randn(N, K, generator=g) / K ** 0.5).to(t16).view(torch.int16).to(dev)
            ring = w.unsqueeze(0).repeat(ncopy, 1, 1).contiguous()
            colsum = w.view(t16).float().sum(-1).contiguous()
            shift = (torch.randn(N, generator=g) * 0.1).to(dev)
            y16 = torch.zeros(M, N, dtype=torch.int16, device=dev)
            y = torch.zeros(M, N, device=dev)
            kc = torch.zeros(M, H, T_SLOTS, 64, dtype=torch.int16, device=dev)
            vc = torch.zeros_like(kc)
            step = torch.zeros(1, dtype=torch.int32, device=dev)
            state = {"i": 0}

            def launch():
                wp = ring[state["i"] % ncopy].data_ptr()
                state["i"] += 1
                if name == "c_fc":
                    rc = lib.rgrg_debug_linear_bf16_ln_kp(a.data_ptr(), wp, shift.data_ptr(), None, None, y16.data_ptr(), None, None, stats.data_ptr(),
                                                          colsum.data_ptr(), M, N, K, N, 2, args.fp16, 0, None)
                else:
                    rc = lib.rgrg_debug_linear_bf16_ln_kv(a.data_ptr(), wp, shift.data_ptr(), y.data_ptr(), stats.data_ptr(), colsum.data_ptr(),
                                                          kc.data_ptr(), vc.data_ptr(), step.data_ptr(), M, H, T_SLOTS, K, N, args.fp16, None)
                _hip.check(rc, name)

            res = {m: [] for m in modes}
            took = {}
            for _ in range(args.rounds):
                for m in modes:
                    os.environ["RGRG_CONS_EPI"] = str(m)
                    for _ in range(10):
                        launch()
                    before = lib.rgrg_debug_cons_epilogue_launches()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.launches):
                        launch()
                    e1.record()
                    torch.cuda.synchronize()
                    took[m] = lib.rgrg_debug_cons_epilogue_launches() - before
                    res[m].append(e0.elapsed_time(e1) * 1000.0 / args.launches)
            print(json.dumps({"launch": name, "M": M, "N": N, "fp16": args.fp16,
                              "us": {str(m): [round(v, 2) for v in res[m]] for m in modes},
                              "median_us": {str(m): round(statistics.median(res[m]), 2) for m in modes},
                              "launches_on_compile_time_epilogue": {str(m): took[m] for m in modes}}), flush=True)


if __name__ == "__main__":
    main()
