"""Quality cost of the e4m3 K/V cache on the synthetic 'bench' weights, CPU only, from the oracle alone: 14 seeded feature rows are
decoded greedily for 128 tokens by the fp32 oracle, then ONE teacher-forced pass over those histories with each
cache: bf16 (oracle/language_model.py), e4m3 rounded directly from fp32 (tests/kv8_reference.py, what the HIP path computes) and
e4m3 rounded through bf16 first (the other evaluation a reader might call legitimate: their distance is the spread between two
e4m3 evaluations).  Writes profiles/kv8_parity.md.  Usage: python tools/kv8_parity.py [--rows 14] [--length 128]"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import kv8_reference as K8  # noqa: E402
from oracle import language_model as o_lm  # noqa: E402
from rgrg_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=14)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kv8_parity.md"))
    a = ap.parse_args()
    torch.set_num_threads(min(8, os.cpu_count() or 8))
    sd = synth.make_state_dict(0, "bench")
    feats = torch.randn((a.rows, 1024), generator=torch.Generator().manual_seed(43))
    L = ["# e4m3 K/V cache against the bf16 cache: the oracle's own figures (synthetic 'bench' weights)", "",
         f"`python tools/kv8_parity.py`: {a.rows} seeded feature rows, {a.length} tokens, greedy histories of the fp32 oracle, one",
         "teacher-forced pass per cache.  CPU only; no HIP code runs.  Quality on a real checkpoint is unmeasured: this tree has only",
         "synthetic weights.", "",
         "| autocast type | arg-max agreement e4m3 vs 16-bit cache | max logit difference / logit range (last position) | "
         "arg-max agreement e4m3 direct vs e4m3 through the 16-bit type | max logit difference / range of those two |", "|---|---|---|---|---|"]
    ids = o_lm.greedy_generate(sd, feats, a.length)
    for mode, name in ((True, "bf16"), (2, "fp16")):
        t16 = o_lm.teacher_forced_trace(sd, ids, feats, bf16=mode)
        with K8.e4m3_cache_oracle():
            t8 = o_lm.teacher_forced_trace(sd, ids, feats, bf16=mode)
        with K8.e4m3_cache_oracle(via16=True):
            t8v = o_lm.teacher_forced_trace(sd, ids, feats, bf16=mode)
        rng = t16["last_logits"].abs().max().item()
        ag = lambda x, y: (x["top_idx"][:, :, 0] == y["top_idx"][:, :, 0]).float().mean().item()  # noqa: E731
        df = lambda x, y: (x["last_logits"] - y["last_logits"]).abs().max().item() / rng  # noqa: E731
        L.append(f"| {name} | {ag(t8, t16):.4f} | {df(t8, t16):.5f} | {ag(t8, t8v):.4f} | {df(t8, t8v):.5f} |")
        print(L[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
