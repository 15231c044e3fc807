"""CPU side of beam search and sampling from a prompt: the fixture of the REAL reference's ``beam_search`` against the CPU loop of
tests/prompt_beam_reference.py, a BOS prompt against ``oracle.language_model.beam_generate``, the public signatures, the argument
errors that need no GPU, the header against the binding, and the sensitivity of the kernel test's inputs."""
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import attn_reference as R
import prompt_beam_reference as pbr
import prompt_reference as pr
import rgrg_amd
from conftest import REPO, load_golden, synth_sd
from oracle import language_model as o_lm
from rgrg_amd import _hip

EOS = 50256
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def fx():
    return load_golden("lm_prompt_beam.pt")


@pytest.fixture(scope="module")
def model():
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.eval()
    return m


def _weights(c, fx):
    return synth_sd("ragged") if c["weights"] == "ragged" else pr.eos_boosted(synth_sd("ragged"), fx["meta"]["eos_boost"])


CASES = ["ones_s3_t4_b4", "leftpad_s3_t5_b4", "padded_s2_t4_b3_k2", "allfinish_s3_t3_b4", "one_iter_s3_t4_b4"]


@pytest.mark.parametrize("case", CASES)
def test_fixture_equals_the_cpu_loop(fx, case):
    c = fx["cases"][case]
    assert fx["meta"]["oracle_matches_reference"] and c["gap"] >= fx["meta"]["min_gap"] == 2e-3
    seq, gap = pbr.beam_search(_weights(c, fx), c["input_ids"], c["attention_mask"], c["feats"], c["max_length"], c["num_beams"],
                               c["early_stopping"], c["num_return_sequences"], return_gap=True)
    assert torch.equal(seq, c["sequences"]), (seq.tolist(), c["sequences"].tolist())
    assert gap == pytest.approx(c["gap"], rel=1e-3)
    T = c["input_ids"].shape[1]
    keep = c["num_return_sequences"]
    assert torch.equal(seq[:, :T], c["input_ids"].repeat_interleave(keep, dim=0))       # the prompt comes back in front
    assert seq.shape[0] == c["input_ids"].shape[0] * keep and T + 1 <= seq.shape[1] <= c["max_length"]


def test_fixture_cases_are_what_they_claim(fx):
    c = fx["cases"]
    assert (c["ones_s3_t4_b4"]["attention_mask"] == 1).all() and c["ones_s3_t4_b4"]["max_length"] == 10
    assert (c["leftpad_s3_t5_b4"]["attention_mask"] == 0).sum(1).tolist() == [0, 1, 3] and c["leftpad_s3_t5_b4"]["early_stopping"]
    assert c["padded_s2_t4_b3_k2"]["num_beams"] == 3 and c["padded_s2_t4_b3_k2"]["num_return_sequences"] == 2
    assert (c["padded_s2_t4_b3_k2"]["attention_mask"] == 0).any()
    a = c["allfinish_s3_t3_b4"]
    assert a["sequences"].shape[1] < a["max_length"]                                     # every item finished early
    o = c["one_iter_s3_t4_b4"]
    assert o["max_length"] == o["input_ids"].shape[1] + 1 and o["sequences"].shape[1] == o["max_length"]
    assert fx["max_length_T"]["case"] == "ones_s3_t4_b4"


def test_bos_prompt_of_ones_equals_beam_generate():
    sd = synth_sd("ragged")
    feats = torch.randn((2, 1024), generator=torch.Generator().manual_seed(5))
    bos = torch.full((2, 1), EOS, dtype=torch.int64)
    ref = o_lm.beam_generate(sd, feats, 6, 3, early_stopping=False, num_return_sequences=2)
    got = pbr.beam_search(sd, bos, torch.ones_like(bos), feats, 6, 3, False, 2)
    assert torch.equal(got, ref)


def test_signatures(model):
    lm = model.language_model
    assert list(inspect.signature(lm.beam_search).parameters) == ["input_ids", "image_hidden_states", "max_length", "beam_scorer",
                                                                   "model_kwargs"]
    assert inspect.signature(lm.beam_search).parameters["model_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    s = inspect.signature(lm.sample_from_prompt)
    assert list(s.parameters) == ["input_ids", "image_hidden_states", "max_length", "attention_mask", "temperature", "top_k", "top_p",
                                  "num_return_sequences", "seed", "return_logprobs"]
    assert s.parameters["max_length"].default is None and s.parameters["attention_mask"].kind is inspect.Parameter.KEYWORD_ONLY
    assert s.parameters["attention_mask"].default is inspect.Parameter.empty
    assert (s.parameters["temperature"].default, s.parameters["top_k"].default, s.parameters["top_p"].default) == (1.0, 0, 1.0)
    b = inspect.signature(model.beam_search_from_prompts)
    assert list(b.parameters) == ["images", "region_prompts", "region_prompt_mask", "max_length", "num_beams", "early_stopping",
                                  "num_return_sequences"]
    assert b.parameters["early_stopping"].default is False and b.parameters["num_return_sequences"].default == 1
    p = inspect.signature(model.sample_from_prompts)
    assert list(p.parameters) == ["images", "region_prompts", "region_prompt_mask", "max_length", "temperature", "top_k", "top_p",
                                  "num_return_sequences", "seed", "return_logprobs"]
    assert p.parameters["max_length"].default is None and p.parameters["temperature"].kind is inspect.Parameter.KEYWORD_ONLY
    eng = rgrg_amd.engine.HipEngine
    assert hasattr(eng, "beam_search_prompted") and hasattr(eng, "sample_decode_prompted")
    assert "not updated" in lm.beam_search.__doc__.lower()


def _scorer(S, nb, groups=1):
    return SimpleNamespace(num_beams=nb, _beam_hyps=[None] * S, length_penalty=1.0, do_early_stopping=False, num_beam_hyps_to_keep=1,
                           num_beam_groups=groups)


def test_argument_errors_without_a_gpu(model):
    lm = model.language_model
    ids = torch.zeros((8, 3), dtype=torch.int64)
    am = torch.ones((8, 3), dtype=torch.int64)
    f = torch.zeros((2, 1024))
    with pytest.raises(AttributeError):                                    # the mask is required, as in the reference's forward
        lm.beam_search(ids, f, 8, _scorer(2, 4), use_cache=True)
    with pytest.raises(ValueError, match="use_cache"):
        lm.beam_search(ids, f, 8, _scorer(2, 4), attention_mask=am, use_cache=False)
    with pytest.raises(TypeError, match="position_ids"):
        lm.beam_search(ids, f, 8, _scorer(2, 4), attention_mask=am, position_ids=None)
    with pytest.raises(ValueError, match="num_beam_groups"):
        lm.beam_search(ids, f, 8, _scorer(2, 4, groups=2), attention_mask=am)
    with pytest.raises(ValueError, match=r"Batch dimension of 'input_ids' should be 12, but is 8\."):   # the reference's message
        lm.beam_search(ids, f, 8, _scorer(3, 4), attention_mask=am)
    with pytest.raises(ValueError, match="max_length"):
        lm.beam_search(ids, f, 3, _scorer(2, 4), attention_mask=am)         # max_length = T
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.beam_search(ids, f, 8, _scorer(2, 4), attention_mask=am)
    with pytest.raises(ValueError, match="temperature"):
        lm.sample_from_prompt(ids, torch.zeros((8, 1024)), 8, attention_mask=am, temperature=0.0)
    with pytest.raises(ValueError, match="top_p"):
        lm.sample_from_prompt(ids, torch.zeros((8, 1024)), 8, attention_mask=am, top_p=0.0)
    with pytest.raises(AttributeError):
        lm.sample_from_prompt(ids, torch.zeros((8, 1024)), 8, attention_mask=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.sample_from_prompt(ids, torch.zeros((8, 1024)), 8, attention_mask=am)
    images = torch.zeros((1, 1, 512, 512))
    rp, rm = torch.zeros((1, 29, 3), dtype=torch.int64), torch.ones((1, 29, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="num_beams"):
        model.beam_search_from_prompts(images, rp, rm, 8, 1)
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.beam_search_from_prompts(images, rp, rm, 8, 2, num_return_sequences=3)
    with pytest.raises(ValueError, match="max_length"):
        model.beam_search_from_prompts(images, rp, rm, 3, 2)
    with pytest.raises(ValueError, match="region_prompts"):
        model.beam_search_from_prompts(images, rp[:, :5], rm[:, :5], 8, 2)
    with pytest.raises(ValueError, match="top_k"):
        model.sample_from_prompts(images, rp, rm, 8, top_k=-1)
    with pytest.raises(ValueError, match="region_prompt_mask"):
        model.sample_from_prompts(images, rp, rm[:, :, :2], 8)


def _header_args(name):
    text = open(os.path.join(REPO, "include", "rgrg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/rgrg_hip.h"
    kinds = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        if "*" in a:
            kinds.append("int*" if re.match(r"^int\s*\*\s*out_len$", a) else "ptr")
        else:
            kinds.append(a.rsplit(" ", 1)[0])
    return kinds


@pytest.mark.parametrize("name", ["rgrg_decoder_beam_search_prompted", "rgrg_decoder_sample_prompted", "rgrg_debug_attn_decode_beam_first"])
def test_header_declares_the_entries_as_the_binding_does(name):
    import ctypes as C
    to_kind = {C.c_void_p: "ptr", C.c_int: "int", C.c_float: "float", C.c_uint64: "uint64_t", C.POINTER(C.c_int): "int*"}
    res, args = _hip.SIGNATURES[name]
    assert res is C.c_int
    assert [to_kind[a] for a in args] == _header_args(name)


def test_abi_version_of_library_and_binding_agree():
    """The new entries are additions: no existing signature changed, and the version the existing tests pin stays."""
    text = open(os.path.join(REPO, "rgrg_amd", "csrc", "runtime.hip")).read()
    assert f"return {_hip.ABI_VERSION};" in text


@pytest.mark.parametrize("kv16", [None, 0, 1])
@pytest.mark.parametrize("nkeys", pbr.BEAM_FIRST_NKEYS)
def test_kernel_test_inputs_are_sensitive(nkeys, kv16):
    """On the inputs of tests/test_gpu_prompt_beam.py::test_attn_decode_beam_first, a kernel that dropped ``first`` (no slot masked)
    or ``src`` (every slot read from the row's own cache row) would be caught: the float64 reference moves by more than 10x the
    comparison bound in every row with first > 0, and in every row that reaches an unmasked slot through a foreign ancestor."""
    d, first, kmask = pbr.beam_first_inputs(nkeys, kv16)
    S, slot = d["S"], d["step"] + 1
    r64 = pbr.beam_first_reference(d, kmask, F64, kv16)[0]
    r32 = pbr.beam_first_reference(d, kmask, F32, kv16)[0]
    bound = R.bound(r64, r32)["bound"]
    no_first = pbr.beam_first_reference(d, None, F64, kv16)[0]
    no_src = pbr.beam_first_reference(d, kmask, F64, kv16, src=None)[0]
    visible = torch.ones((S, slot), dtype=torch.bool)                        # slots 0 .. step (slot step + 1 is the new token's)
    for s in range(S):
        visible[s, 1:1 + int(first[s])] = False
    foreign = ((d["src"][:, :slot].long() != torch.arange(S)[:, None]) & visible).any(1)
    assert (first > 0).any() or nkeys == 2
    assert foreign.any() or nkeys == 2
    for s in range(S):
        if first[s] > 0:
            assert (no_first[s] - r64[s]).abs().max().item() > 10 * bound, (s, int(first[s]))
        if foreign[s]:
            assert (no_src[s] - r64[s]).abs().max().item() > 10 * bound, (s, "src")


def test_sampling_loop_from_a_prompt():
    """The CPU sampling loop: top_k = 1 is the greedy loop of tests/prompt_reference.py on the same ragged prompt; an unfiltered run
    draws at the counter (row, column - 1), holds log-prob 0 in the prompt columns and is deterministic in the seed."""
    sd = synth_sd("ragged")
    g = torch.Generator().manual_seed(31)
    ids = torch.randint(0, 50000, (2, 3), generator=g)
    mask = torch.tensor([[1, 1, 1], [0, 1, 1]])
    ids[1, 0] = EOS
    feats = torch.randn((2, 1024), generator=g)
    greedy = pr.greedy_search(sd, ids, feats, 6, mask)
    one, lp1, flips = pbr.sample(sd, ids, mask, feats, 6, seed=9, top_k=1)
    assert flips == 0 and torch.equal(one, greedy) and (lp1[:, :3] == 0).all() and (lp1[:, 3:] == 0).all()   # one kept token: log 1
    a, la, _ = pbr.sample(sd, ids, mask, feats, 5, seed=9)
    b, lb, _ = pbr.sample(sd, ids, mask, feats, 5, seed=9)
    c, _, _ = pbr.sample(sd, ids, mask, feats, 5, seed=10)
    assert torch.equal(a, b) and torch.equal(la, lb) and not torch.equal(a, c)
    assert torch.equal(a[:, :3], ids) and (la[:, :3] == 0).all() and (la[:, 3] < 0).all()
    # the first draw again, by hand: row s, column 3 -> counter (s, 2)
    am = mask.clone()
    logits, _ = o_lm.lm_forward(sd, ids, am, feats, None, pr.positions_from_mask(am))
    import sample_reference as sr
    for s in range(2):
        tok, logp = sr.Row(logits[s, -1].numpy()).draw(9, s, 2)
        assert int(a[s, 3]) == tok and abs(float(la[s, 3]) - logp) <= 1e-6
