"""Golden fixture for ``LanguageModel.beam_search`` with a PROMPT: the REAL reference's loop (language_model.py:529-607 on the
restated HF-4.19.2 BeamSearchScorer, positions from ``prepare_inputs_for_generation`` :498-520) on the seeded synthetic weights, run
in the build container, with the CPU loop of tests/prompt_beam_reference.py checked against it BIT FOR BIT (exit status 1 otherwise).
Data only: prompts, masks, features, returned sequences, meta.

  ones_s3_t4_b4         S=3, T=4, 4 beams, mask of ones, max_length 10
  leftpad_s3_t5_b4      S=3, T=5, 4 beams, left padding of 0 / 1 / 3 slots, early stopping, max_length 11
  padded_s2_t4_b3_k2    S=2, T=4, 3 beams, left padding of 2 / 0 slots, num_return_sequences = 2, max_length 9
  allfinish_s3_t3_b4    wte[EOS] scaled by 1.05 (prompt_reference.eos_boosted): every item finishes early
  one_iter_s3_t4_b4     max_length = T + 1: one iteration, the first ranking alone
  max_length_T          what the real reference does at max_length = T (recorded like the ``no_mask`` case of lm_prompt_greedy.pt)

Ties: over every step and unfinished item, the smallest difference between adjacent entries of the top 2 * num_beams + 1 candidate
scores must be at least 2e-3 - the project's own bound on fp32 logits against the oracle, so a swapped ranking would need an error
the other tests already forbid.  Seeds are walked upward from SEED0 until it is.  An item's prompt and features are drawn from the
item's OWN seed (items of a batch do not interact in beam search), so the walk runs item by item on the CPU loop - the joint event
"every gap of every item of a case" is too rare on these weights (about 0.035 between neighbours in one row's top candidates) to
be met by one seed per case.  The gap that is accepted and recorded is that of the whole case, computed once more on the batch.

    python tests/golden/make_golden_lm_prompt_beam.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

import ref_harness  # noqa: E402
import prompt_beam_reference as pbr  # noqa: E402
import prompt_reference as pr  # noqa: E402
from rgrg_amd import synth  # noqa: E402

EOS = 50256
SEED0 = 400
MIN_GAP = 2e-3
MAX_SEEDS = 20000

#        name                  S  T  beams pads        early  keep max_length weights             steps
CASES = [("ones_s3_t4_b4",      3, 4, 4,    None,       False, 1,   10,        "ragged",           True),
         ("leftpad_s3_t5_b4",   3, 5, 4,    (0, 1, 3),  True,  1,   11,        "ragged",           True),
         ("padded_s2_t4_b3_k2", 2, 4, 3,    (2, 0),     False, 2,   9,         "ragged",           True),
         ("allfinish_s3_t3_b4", 3, 3, 4,    None,       False, 1,   11,        "ragged_eos_x1.05", False),
         ("one_iter_s3_t4_b4",  3, 4, 4,    (0, 2, 0),  False, 1,   5,         "ragged",           False)]


def item(seed, T, pad):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 50000, (1, T), generator=g)
    mask = torch.ones((1, T), dtype=torch.int64)
    mask[0, :pad] = 0
    ids[0, :pad] = EOS
    return ids, mask, torch.randn((1, 1024), generator=g)


def reference_beam_search(lm, ids, mask, feats, max_length, nb, early, keep):
    from transformers.generation_beam_search import BeamSearchScorer
    S = ids.shape[0]
    scorer = BeamSearchScorer(batch_size=S, num_beams=nb, device=ids.device, length_penalty=1.0, do_early_stopping=early,
                              num_beam_hyps_to_keep=keep)
    with torch.no_grad():
        return lm.beam_search(pbr.expand(ids, nb), feats, max_length, scorer, attention_mask=pbr.expand(mask, nb), use_cache=True)


def main():
    model = ref_harness.reference_model()
    sd = synth.make_state_dict(0, "ragged")
    sd_eos = pr.eos_boosted(sd, 1.05)
    lm = model.language_model
    cases, ok_all, loaded, seed = {}, True, None, SEED0
    for name, S, T, nb, pads, early, keep, max_length, weights, steps in CASES:
        w = sd_eos if weights != "ragged" else sd
        if loaded is not w:
            model.load_state_dict(synth.to_reference_state_dict(w), strict=True)
            loaded = w
        while True:
            parts, seeds = [], []
            for i in range(S):
                for _ in range(MAX_SEEDS):
                    it = item(seed, T, (pads or (0,) * S)[i])
                    seed += 1
                    one = pbr.beam_search(w, *it, max_length, nb, early, keep, return_gap=True, stop_below=MIN_GAP)[0]
                    # ... and, where the case is about the steps behind the prompt, the item's best hypothesis continues the prompt
                    # by at least one token that is not EOS (an item that finishes at once exercises the first ranking only)
                    if one is not None and (not steps or bool((one[0, T:] != EOS).any())):
                        break
                else:
                    print(f"{name}: item {i}: no seed in {MAX_SEEDS} with a gap of {MIN_GAP}")
                    return 1
                parts.append(it)
                seeds.append(seed - 1)
                print(f"{name}: item {i}: seed {seed - 1}", flush=True)
            ids, mask, feats = (torch.cat([p[k] for p in parts]) for k in range(3))
            o_seq, gap = pbr.beam_search(w, ids, mask, feats, max_length, nb, early, keep, return_gap=True)
            if gap >= MIN_GAP:   # (the batch may round differently from the single items)
                break
            print(f"{name}: the batch has a gap of {gap:.2e}: walking on")
        seq = reference_beam_search(lm, ids, mask, feats, max_length, nb, early, keep)
        ok = o_seq.shape == seq.shape and bool(torch.equal(o_seq, seq))
        ok_all &= ok
        print(f"{name}: seeds {seeds} gap {gap:.4f} L = {seq.shape[1]} generated {seq[:, T:].tolist()} oracle == reference: {ok}")
        cases[name] = dict(input_ids=ids, attention_mask=mask, feats=feats, max_length=max_length, num_beams=nb, early_stopping=early,
                           num_return_sequences=keep, weights=weights, sequences=seq.clone(), seeds=seeds, gap=gap)
    # max_length = T: what the real reference does (its loop runs one iteration before it looks at max_length)
    c = cases["ones_s3_t4_b4"]
    model.load_state_dict(synth.to_reference_state_dict(sd), strict=True)
    T = c["input_ids"].shape[1]
    try:
        seq = reference_beam_search(lm, c["input_ids"], c["attention_mask"], c["feats"], T, c["num_beams"], False, 1)
        at_T = {"raised": None, "shape": tuple(seq.shape)}
    except Exception as e:  # noqa: BLE001
        at_T = {"raised": {"type": type(e).__name__, "message": str(e)}, "shape": None}
    print("beam_search at max_length = T:", at_T)
    out = {"meta": {"torch": str(torch.__version__), "reference": "ttanida/rgrg", "weights_seed": 0, "profile": "ragged", "eos_boost": 1.05,
                    "seed0": SEED0, "min_gap": MIN_GAP, "seeds": {k: v["seeds"] for k, v in cases.items()},
                    "gaps": {k: v["gap"] for k, v in cases.items()}, "oracle_matches_reference": bool(ok_all)},
           "cases": cases, "max_length_T": {"case": "ones_s3_t4_b4", **at_T}}
    torch.save(out, os.path.join(HERE, "lm_prompt_beam.pt"))
    print("saved lm_prompt_beam.pt; oracle matches reference bit for bit:", ok_all)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
