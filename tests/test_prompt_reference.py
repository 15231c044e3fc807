"""Prompted greedy search without a GPU: the oracle loop of tests/prompt_reference.py reproduces the REAL reference's
``greedy_search`` on every case of tests/golden/lm_prompt_greedy.pt bit for bit, the public method exists with the reference's
parameter names, and the header and the ctypes binding still agree with the new entries."""
import inspect
import os
import re

import pytest
import torch

import prompt_reference as pr
from conftest import REPO, load_golden, synth_sd
from rgrg_amd import _hip


@pytest.fixture(scope="module")
def fx():
    return load_golden("lm_prompt_greedy.pt")


CASES = ["ones_s3_t4", "leftpad_s4_t5", "eos_inside_s3_t4", "one_token_s3_t4", "allfinish_s4_t3"]


@pytest.mark.parametrize("case", CASES)
def test_oracle_loop_reproduces_the_reference(fx, case):
    assert fx["meta"]["oracle_matches_reference"] and sorted(fx["cases"]) == sorted(CASES)
    c = fx["cases"][case]
    sd = synth_sd("ragged")
    if c["weights"] != "ragged":
        sd = pr.eos_boosted(sd, fx["meta"]["eos_boost"])
    ids, last, past = pr.greedy_search(sd, c["input_ids"], c["feats"], c["max_length"], c["attention_mask"], return_prompt_pass=True)
    T = c["input_ids"].shape[1]
    assert torch.equal(ids, c["output_ids"]) and torch.equal(ids[:, :T], c["input_ids"])
    assert ids.shape[1] == max(T + 1, min(c["max_length"], ids.shape[1]))
    assert (last[:, ::fx["meta"]["probe_stride"]] - c["last_logits_probe"]).abs().max().item() <= 2e-4
    assert past[0][0].shape == (ids.shape[0], 16, T + 1, 64)


def test_fixture_shape_of_every_case(fx):
    c = fx["cases"]
    assert c["leftpad_s4_t5"]["attention_mask"].sum(1).tolist() == [5, 4, 3, 2]
    assert (c["eos_inside_s3_t4"]["input_ids"][:, 1] == pr.EOS).all() and c["eos_inside_s3_t4"]["output_ids"].shape[1] > 5
    assert c["one_token_s3_t4"]["output_ids"].shape[1] == 5 and c["one_token_s3_t4"]["max_length"] == 4
    fin = c["allfinish_s4_t3"]["output_ids"]
    assert fin.shape[1] < c["allfinish_s4_t3"]["max_length"] and ((fin[:, 3:] == pr.EOS).sum(1) >= 1).all()
    assert all(v["output_ids"].shape[1] - v["input_ids"].shape[1] <= 8 for v in c.values())
    # case (iii): without a mask the reference's own loop raises - there are no ids to record
    assert fx["no_mask"]["raised"]["type"] == "AttributeError"


def test_greedy_search_has_the_reference_signature():
    import rgrg_amd
    lm = rgrg_amd.LanguageModel
    sig = inspect.signature(lm.greedy_search)
    assert list(sig.parameters) == ["self", "input_ids", "image_hidden_states", "max_length", "model_kwargs"]
    assert sig.parameters["model_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(rgrg_amd.ReportGenerationModel.generate_from_prompts).parameters) == [
        "self", "images", "region_prompts", "region_prompt_mask", "max_length"]
    from rgrg_amd.engine import HipEngine
    assert "greedy_decode_prompted" in vars(HipEngine)


def test_greedy_search_argument_errors_need_no_gpu():
    import rgrg_amd
    lm = rgrg_amd.LanguageModel()
    ids, feats = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 1024))
    am = torch.ones((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError):
        lm.greedy_search(ids, feats, 8, attention_mask=am, use_cache=False)
    with pytest.raises(TypeError):
        lm.greedy_search(ids, feats, 8, attention_mask=am, past=None)
    with pytest.raises(AttributeError):
        lm.greedy_search(ids, feats, 8, use_cache=True)
    with pytest.raises(RuntimeError):      # CPU tensors: no fallback
        lm.greedy_search(ids, feats, 8, attention_mask=am, use_cache=True)


def test_header_declares_the_new_entries_like_the_binding():
    with open(os.path.join(REPO, "include", "rgrg_hip.h")) as f:
        header = f.read()
    for name in ("rgrg_decoder_generate_prompted", "rgrg_debug_attn_decode_first", "rgrg_debug_resid_dropout_ln16", "rgrg_debug_ln_backward",
                 "rgrg_debug_ce_rows", "rgrg_debug_ce_finalize", "rgrg_debug_ce_backward", "rgrg_debug_gelu", "rgrg_debug_dropout_add"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_hip.SIGNATURES[name][1]), name
    declared = set(re.findall(r"\b(rgrg_[a-z0-9_]+)\s*\(", header))
    assert set(_hip.SIGNATURES) <= declared
    assert _hip.ABI_VERSION == 28   # 26 brought the prompted entries, 27 the hooks of the training pass's row kernels, 28 those of the skinny GEMMs
