"""Diverse beam search without a GPU: the CPU references of tests/group_beam_reference.py against what the project already pins
(G = 1 is ``oracle.language_model.beam_generate``), the sufficiency of the row candidate lists that ``beam_group_merge_kernel``
ranks, the recorded end-to-end cases of tests/test_gpu_group_beam.py recomputed (gap and diversity), and the argument errors,
signatures and ABI of the new entry points."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import group_beam_reference as gbr
import prompt_beam_reference as pbr
import rgrg_amd
from conftest import synth_sd
from oracle import language_model as o_lm
from rgrg_amd import _hip

EOS = gbr.EOS


# ------------------------------------------------------------------------------------------------ the CPU loop
def test_one_group_is_beam_generate():
    sd = synth_sd("ragged")
    feats = gbr.feats_of(84, 2)
    for early, keep in ((False, 1), (True, 3)):
        ref = o_lm.beam_generate(sd, feats, 7, 4, early_stopping=early, num_return_sequences=keep)
        got = gbr.group_beam_search(sd, feats, 7, 4, 1, 0.0, early, keep)
        assert torch.equal(got, ref), (got.tolist(), ref.tolist())


@pytest.mark.parametrize("name", sorted(gbr.CASES))
def test_recorded_case(name):
    """Every end-to-end case the GPU is held to: its gap is at least the project's min_gap (an fp32 ranking that differs from the CPU
    loop's below that is no error), and its sequences differ from plain beam search with the same beams - a dropped penalty cannot
    pass."""
    c = gbr.CASES[name]
    r = gbr.case_reference(name, synth_sd)
    print(f"GROUPBEAM case={name} gap={r['gap']:.6f} recorded={c['gap']}")
    assert r["gap"] >= gbr.MIN_GAP and abs(r["gap"] - c["gap"]) < 1e-4, r["gap"]
    S = r["feats"].shape[0]
    ids = r["ids"] if r["ids"] is not None else torch.full((S, 1), EOS, dtype=torch.int64)
    mask = r["mask"] if r["mask"] is not None else torch.ones_like(ids)
    plain = pbr.beam_search(gbr.case_weights(name, synth_sd), ids, mask, r["feats"], c["L"], c["nb"], c["early"], c["nb"])
    assert r["seq"].shape[0] == S * c["nb"]
    assert plain.shape != r["seq"].shape or not torch.equal(plain, r["seq"])
    if c.get("flips"):   # `done` set by group 0 of a step and seen by a later group of the same step
        assert any(bool((~t[0] & t[g]).any()) for t in r["trace"] for g in range(1, c["G"]))


# ------------------------------------------------------------------------------------------------ the kernel's contract
@pytest.mark.parametrize("nb,G", [(2, 2), (4, 2), (4, 4), (6, 3), (6, 1), (8, 2)])
@pytest.mark.parametrize("lam", [0.3, 2.5])
def test_row_lists_are_enough(nb, G, lam):
    """merge_reference on the rows' top 2 nb equals the ranking of the FULL penalised rows: V = 97, planted ties (equal logits in a
    row, equal rows in a group, equal first rows of the groups as at the start of a search), EOS among the best tokens, and a
    penalty of 2.5 that pushes listed tokens far down their rows."""
    V, S, eos = 97, 4, 96
    rng = np.random.RandomState(100 * nb + G)
    gs, R = nb // G, S * nb
    logits = (rng.standard_normal((R, V)) * 2).astype(np.float32)
    logits[:, eos] += rng.choice([0.0, 3.0, 6.0], size=R).astype(np.float32)
    beam_scores = (-rng.random_sample(R) * 3).astype(np.float32)
    for s in range(S):
        for g in range(G):
            r0 = s * nb + g * gs
            if s == 0:      # the start of a search
                logits[r0] = logits[0]
                beam_scores[r0:r0 + gs] = -1e9
                beam_scores[r0] = 0
            if s == 1:      # near-equal rows everywhere: every group wants the same tokens
                logits[r0:r0 + gs] = logits[nb]
                beam_scores[r0:r0 + gs] = beam_scores[nb]
            if s == 2 and gs > 1:   # two equal rows in a group
                logits[r0 + 1], beam_scores[r0 + 1] = logits[r0], beam_scores[r0]
        t = rng.choice(V - 1, size=4, replace=False)
        logits[s * nb:(s + 1) * nb, t[1]] = logits[s * nb:(s + 1) * nb, t[0]]      # equal logits inside every row of the item
        logits[s * nb:(s + 1) * nb, t[3]] = logits[s * nb:(s + 1) * nb, t[2]]
    row_max, row_logsum, top_val, top_tok = gbr.row_lists(logits, 2 * nb)
    info = {}
    got = gbr.merge_reference(row_max, row_logsum, top_val, top_tok, beam_scores, S, nb, G, lam, V, eos=eos, info=info)
    ref = gbr.brute_force_merge(logits, row_max, row_logsum, beam_scores, S, nb, G, lam, eos)
    assert np.array_equal(got[0].view(np.int32), ref[0].view(np.int32))
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    if G > 1 and lam > 1:
        assert info["pushed_out"] > 0


def test_kernel_test_inputs_reach_every_branch():
    """What tests/test_gpu_group_beam.py feeds the kernel contains, over its cases: equal scores in different rows of a group, EOS
    ranked below and at or above gs, a ranked candidate whose token two or more earlier beams took (freq >= 2 as APPLIED), a
    penalised token that leaves the top 2 gs, -1e9 beam scores.  And a contracted multiply-subtract FAILS that test: at penalty 0.3
    the expected output differs from the output of the same ranking with the penalty fused into one fma (at 0.5 every product is
    exact and the two agree)."""
    info, fused_cases = {}, []
    for nb, G in gbr.MERGE_CASES:
        d = gbr.merge_inputs(nb, G)
        args = (d["row_max"], d["row_logsum"], d["top_val"], d["top_tok"], d["beam_scores"], gbr.MERGE_S, nb, G)
        for lam in (0.3, 0.5):
            one = {}
            s, t, b = gbr.merge_reference(*args, lam, gbr.V_MODEL, info=one)
            gs = nb // G
            for item in range(gbr.MERGE_S):     # every group's slots are sorted and its beams are rows of the group
                for g in range(G):
                    sl = slice(g * 2 * gs, (g + 1) * 2 * gs)
                    assert (np.diff(s[item, sl]) <= 0).all() and ((b[item, sl] // gs) == g).all()
            for k, v in one.items():
                info[k] = (info.get(k, set()) | v) if isinstance(v, set) else max(info.get(k, 0), v)
            fs, ft, fb = gbr.merge_reference(*args, lam, gbr.V_MODEL, fused=True)
            differs = not (np.array_equal(fs.view(np.int32), s.view(np.int32)) and np.array_equal(ft, t) and np.array_equal(fb, b))
            if differs:
                fused_cases.append((nb, G, lam, int((fs.view(np.int32) != s.view(np.int32)).sum())))
            if lam == 0.5:
                assert not differs
    print("GROUPBEAM fused multiply-subtract changes the expected output of", fused_cases)
    assert info["row_ties"] > 0 and info["eos_ranks"] == {"lt", "ge"} and info["max_freq"] >= 5
    assert info["pushed_out"] > 0 and info["minus_1e9"] > 0
    assert any(c[:3] == (16, 16, 0.3) for c in fused_cases), fused_cases


# ------------------------------------------------------------------------------------------------ arguments, signatures, ABI
@pytest.fixture(scope="module")
def model():
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.eval()
    return m


def test_signatures(model):
    sig = inspect.signature(model.language_model.group_beam_search)
    assert list(sig.parameters) == ["image_hidden_states", "max_length", "num_beams", "num_beam_groups", "diversity_penalty",
                                    "early_stopping", "num_return_sequences", "length_penalty", "input_ids", "attention_mask"]
    kw = [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert kw == ["early_stopping", "num_return_sequences", "length_penalty", "input_ids", "attention_mask"]
    assert sig.parameters["early_stopping"].default is False and sig.parameters["num_return_sequences"].default == 1
    assert sig.parameters["length_penalty"].default == 1.0 and sig.parameters["input_ids"].default is None
    rsig = inspect.signature(model.generate_diverse)
    assert list(rsig.parameters) == ["images", "max_length", "num_beams", "num_beam_groups", "diversity_penalty", "early_stopping",
                                     "num_return_sequences"]
    assert rsig.parameters["early_stopping"].default is False and rsig.parameters["num_return_sequences"].default == 1


def test_abi_version_and_symbols():
    assert _hip.ABI_VERSION == 28
    lib = _hip.load()
    assert lib.rgrg_abi_version() == 28
    for name in ("rgrg_decoder_group_beam_search", "rgrg_decoder_group_beam_search_prompted", "rgrg_debug_beam_group_merge"):
        assert name in _hip.SIGNATURES and getattr(lib, name).argtypes == _hip.SIGNATURES[name][1]


BAD = [   # (num_beams, num_beam_groups, diversity_penalty, num_return_sequences, max_length)
    (6, 4, 0.5, 1, 8),      # nb % G != 0
    (2, 4, 0.5, 1, 8),      # G > nb
    (4, 2, 0.0, 1, 8),      # G > 1, penalty not > 0
    (4, 2, -0.5, 1, 8),
    (4, 2, 1, 1, 8),        # ... not a float (HF's rule)
    (4, 2, None, 1, 8),
    (32, 2, 0.5, 1, 8),     # more than 16 beams
    (4, 2, 0.5, 0, 8),      # num_return_sequences outside 1 .. nb
    (4, 2, 0.5, 5, 8),
    (4, 2, 0.5, 1, None),   # max_length None
]


@pytest.mark.parametrize("nb,G,lam,keep,L", BAD)
def test_python_refusals(model, nb, G, lam, keep, L):
    f = torch.zeros(2, 1024)
    with pytest.raises(ValueError):
        model.language_model.group_beam_search(f, L, nb, G, lam, num_return_sequences=keep)
    with pytest.raises(ValueError):
        model.generate_diverse(torch.zeros(1, 1, 512, 512), L, nb, G, lam, num_return_sequences=keep)


def test_prompt_argument_errors_and_no_cpu_fallback(model):
    lm = model.language_model
    f = torch.zeros(2, 1024)
    ids, am = torch.zeros((2, 3), dtype=torch.int64), torch.ones((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="together"):
        lm.group_beam_search(f, 8, 4, 2, 0.5, input_ids=ids)
    with pytest.raises(ValueError, match="together"):
        lm.group_beam_search(f, 8, 4, 2, 0.5, attention_mask=am)
    with pytest.raises(ValueError, match="max_length"):
        lm.group_beam_search(f, 3, 4, 2, 0.5, input_ids=ids, attention_mask=am)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.group_beam_search(f, 8, 4, 2, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.group_beam_search(f, 8, 4, 1, 0.0, input_ids=ids, attention_mask=am)     # G = 1 takes any penalty
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.generate_diverse(torch.zeros(1, 1, 512, 512), 8, 4, 2, 0.5)
    # the modes generate() and beam_search() refused before are still refused there
    with pytest.raises(NotImplementedError, match="Diverse beam-search decoding is not implemented."):
        lm.generate(f, 8, num_beams=4, num_beam_groups=2)


@pytest.mark.parametrize("nb,G,lam,keep,word", [(6, 4, 0.5, 1, "divisible"), (2, 4, 0.5, 1, "smaller or equal"), (4, 2, 0.0, 1, "diversity_penalty"),
                                                (4, 2, float("nan"), 1, "diversity_penalty"), (32, 2, 0.5, 1, "at most 16"),
                                                (4, 2, 0.5, 5, "num_return_sequences"), (4, 2, 0.5, 0, "num_return_sequences")])
def test_c_refusals_carry_a_message(nb, G, lam, keep, word):
    """RGRG_EINVAL (2) with a message, decided before the decoder or the GPU is touched."""
    lib = _hip.load()
    n = C.c_int(0)
    rc = lib.rgrg_decoder_group_beam_search(None, None, 1, nb, G, lam, 8, 0, 1.0, keep, None, 8, C.byref(n), None)
    assert rc != 0 and word in lib.rgrg_last_error().decode()
    rc = lib.rgrg_decoder_group_beam_search_prompted(None, None, None, None, 1, 3, nb, G, lam, 8, 0, 1.0, keep, None, 8, C.byref(n), None)
    assert rc != 0
    assert lib.rgrg_debug_beam_group_merge(None, None, None, None, None, 1, 4, 2, 0.5, 100, None, None, None, None) != 0
