"""Golden fixture for ``LanguageModel.greedy_search`` with a PROMPT: the REAL reference's loop (language_model.py:609-652, positions
from ``prepare_inputs_for_generation`` :498-520) on the seeded synthetic weights, run in the build container, with the oracle loop
of tests/prompt_reference.py checked against it.  Data only: prompts, masks, features, returned ids, and the logits of the last
prompt position (a strided probe of every row, one full row).

  (i)   S=3, T=4, mask of ones                      (ii)  S=4, T=5, left padding of 0, 1, 2, 3 slots
  (iii) case (ii) WITHOUT attention_mask: the reference cannot run it - the exception it raises is recorded
  (iv)  an EOS in the middle of the prompt          (v)   T = max_length: one generated token
  (vi)  wte[EOS] scaled by 1.05 (prompt_reference.eos_boosted): every row emits EOS within two tokens - PAD behind EOS, early exit

    python tests/golden/make_golden_lm_prompt.py
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
import prompt_reference as pr  # noqa: E402
from rgrg_amd import synth  # noqa: E402

EOS = 50256
PROBE = 97


def main():
    model = ref_harness.reference_model()
    sd = synth.make_state_dict(0, "ragged")
    sd_eos = pr.eos_boosted(sd, 1.05)
    lm = model.language_model
    g = torch.Generator().manual_seed(71)

    def prompt(S, T, pads=None):
        ids = torch.randint(0, 50000, (S, T), generator=g)
        mask = torch.ones((S, T), dtype=torch.int64)
        for s, p in enumerate(pads or ()):
            mask[s, :p] = 0
            ids[s, :p] = EOS
        return ids, mask, torch.randn((S, 1024), generator=g)

    cases = {}
    ids, mask, feats = prompt(3, 4)
    cases["ones_s3_t4"] = dict(input_ids=ids, attention_mask=mask, feats=feats, max_length=10, weights="ragged")
    ids, mask, feats = prompt(4, 5, (0, 1, 2, 3))
    cases["leftpad_s4_t5"] = dict(input_ids=ids, attention_mask=mask, feats=feats, max_length=11, weights="ragged")
    ids, mask, feats = prompt(3, 4)
    ids[:, 1] = EOS
    ids[0, 2] = EOS
    cases["eos_inside_s3_t4"] = dict(input_ids=ids, attention_mask=mask, feats=feats, max_length=9, weights="ragged")
    ids, mask, feats = prompt(3, 4)
    cases["one_token_s3_t4"] = dict(input_ids=ids, attention_mask=mask, feats=feats, max_length=4, weights="ragged")
    ids, mask, feats = prompt(4, 3)
    cases["allfinish_s4_t3"] = dict(input_ids=ids, attention_mask=mask, feats=feats, max_length=11, weights="ragged_eos_x1.05")

    ok_all = True
    loaded = None
    for name, c in cases.items():
        w = sd_eos if c["weights"] != "ragged" else sd
        if loaded is not w:
            model.load_state_dict(synth.to_reference_state_dict(w), strict=True)
            loaded = w
        ids, mask, feats = c["input_ids"], c["attention_mask"], c["feats"]
        with torch.no_grad():
            out = lm.greedy_search(ids.clone(), feats, c["max_length"], attention_mask=mask.clone(), use_cache=True)
            logits, _ = lm(ids.clone(), mask.clone(), feats, return_loss=False, position_ids=pr.positions_from_mask(mask), use_cache=True)
        last = logits[:, -1]
        o_ids, o_last, _ = pr.greedy_search(w, ids, feats, c["max_length"], mask, return_prompt_pass=True)
        ok = o_ids.shape == out.shape and bool(torch.equal(o_ids, out)) and (o_last - last).abs().max().item() <= 2e-4
        ok_all &= ok
        top2 = last.topk(2, -1).values
        print(f"{name}: L' = {out.shape[1]} ids {out[:, ids.shape[1]:].tolist()} first-token top-2 gap {(top2[:, 0] - top2[:, 1]).min().item():.4f} "
              f"oracle |dlogits| {(o_last - last).abs().max().item():.2e} ok={ok}")
        c.update(output_ids=out.clone(), last_logits_probe=last[:, ::PROBE].clone(), logits_absmax=last.abs().max().item())
        if name == "leftpad_s4_t5":
            c["last_logits_row3"] = last[3].clone()
    # (iii): the reference without a mask
    c = cases["leftpad_s4_t5"]
    model.load_state_dict(synth.to_reference_state_dict(sd), strict=True)
    try:
        with torch.no_grad():
            lm.greedy_search(c["input_ids"].clone(), c["feats"], c["max_length"], use_cache=True)
        raised = None
    except Exception as e:  # noqa: BLE001
        raised = {"type": type(e).__name__, "message": str(e)}
    print("greedy_search without attention_mask:", raised)
    out = {"meta": {"torch": str(torch.__version__), "reference": "ttanida/rgrg", "weights_seed": 0, "profile": "ragged",
                    "eos_boost": 1.05, "probe_stride": PROBE, "oracle_matches_reference": bool(ok_all)},
           "cases": cases, "no_mask": {"case": "leftpad_s4_t5", "raised": raised}}
    torch.save(out, os.path.join(HERE, "lm_prompt_greedy.pt"))
    print("saved lm_prompt_greedy.pt; oracle matches reference:", ok_all)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
