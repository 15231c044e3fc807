"""The sampler's reference (tests/sample_reference.py) checked on the CPU: its generator against published vectors, its
filters against a direct torch restatement of HF 4.19.2's warpers, its acceptance rule against eight deliberate mutations,
and the argument checks / signatures of the Python entry points."""
import inspect

import numpy as np
import pytest
import torch

import sample_reference as sr
from conftest import synth_sd


def test_philox_known_answer_vectors():
    # Random123 kat_vectors, philox4x32-10 (the first one also pins the detector samplers: tests/test_gpu_samplers.py)
    assert sr.philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert sr.philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert sr.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    assert 0.0 <= sr.uniform(7, 3, 5) < 1.0 and sr.uniform(7, 3, 5) != sr.uniform(7, 5, 3)


def _hf_keep(x, T, k, p):
    """HF 4.19.2 TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper(min_tokens_to_keep=1), restated directly."""
    s = torch.from_numpy(x).double() / T
    if 0 < k < s.numel():
        s = s.masked_fill(s < torch.topk(s, k)[0][-1], -float("inf"))
    if p < 1.0:
        sl, si = torch.sort(s, descending=True)
        remove = sl.softmax(-1).cumsum(-1) > p
        remove[1:] = remove[:-1].clone()
        remove[0] = False
        s = s.masked_fill(torch.zeros_like(remove).scatter(0, si, remove), -float("inf"))
    return torch.isfinite(s).numpy()


@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (1.0, 50, 1.0), (0.5, 0, 0.9), (2.0, 50, 0.5), (1.0, 7, 0.3), (1.0, 0, 1e-6)])
def test_kept_set_equals_hf_warpers_on_tie_free_rows(T, k, p):
    rng = np.random.default_rng(5)
    for kind in ("peaked", "dominant"):
        x = sr.make_row(kind, rng, 1501)
        while len(np.unique(x)) != len(x):   # tie-free
            x = sr.make_row(kind, rng, 1501)
        row = sr.Row(x, T, k, p)
        if row.is_coin_flip():
            continue
        assert np.array_equal(row.keep, _hf_keep(x, T, k, float(np.float32(p)))), (kind, T, k, p)


def test_top_k_1_is_first_occurrence_argmax_and_ties_rule():
    x = np.array([0.0, 3.0, 1.0, 3.0, 2.0, 2.0, -np.inf, 1.0], dtype=np.float32)
    for t in range(20):
        tok, lp = sr.Row(x, 1.0, 1, 1.0).draw(11, 0, t)
        assert tok == 1 == int(np.argmax(x)) and lp == pytest.approx(np.log(0.5))
    assert sr.Row(x, 1.0, 3, 1.0).keep.tolist() == [False, True, False, True, True, True, False, False]   # ties with the k-th: all kept
    # top-p: the two 2.0 have the same mass above (2 e^3 / total = 0.665) and are kept or dropped TOGETHER
    assert sr.Row(x, 1.0, 0, 0.7).keep.tolist() == [False, True, False, True, True, True, False, False]
    assert sr.Row(x, 1.0, 0, 0.6).keep.tolist() == [False, True, False, True, False, False, False, False]
    assert sr.Row(x, 1.0, 0, 1e-6).keep.tolist() == [False, True, False, True, False, False, False, False]   # mass above 0 <= top_p


CASES = [("peaked", 2.0, 50, 0.9), ("ties", 1.0, 50, 0.9), ("flat", 0.25, 50, 0.9), ("neg_inf", 4.0, 0, 0.5)]
MUTATIONS = ("no_temperature", "topk_strict", "topp_strict", "topp_first", "swap_counter", "second_word", "sorted_cdf",
             "unfiltered_logprob")


def _boundary_row():
    """A row whose second token sits EXACTLY on the top-p boundary in the reference's own arithmetic (top_p = its mass-above as
    float64): `<` and `<=` differ there.  Hand-made; the generators reject such rows."""
    x = np.full(64, -np.inf, dtype=np.float32)
    x[[5, 9, 30]] = (2.0, 1.0, 0.0)
    p = np.float64(sr.Row(x, 1.0, 0, np.float64(0.99)).mass_above(np.ones(64, dtype=bool))[9])
    return x, p


def test_acceptance_rule_accepts_the_reference_and_rejects_every_mutation():
    seed = 1234
    rejected = {m: 0 for m in MUTATIONS}
    for ci, (kind, T, k, p) in enumerate(CASES):
        xs, rows, _ = sr.make_rows(kind, 6, 100 + ci, T, k, p, V=4001)
        for r, (x, row) in enumerate(zip(xs, rows)):
            for t in range(8):
                tok, lp = row.draw(seed, r, t)
                ok, why = row.accept(seed, r, t, tok, np.float32(lp))
                assert ok, why
                for mname in MUTATIONS:
                    mtok, mlp = sr.Row(x, T, k, p, mut=mname).draw(seed, r, t)
                    rejected[mname] += not row.accept(seed, r, t, mtok, np.float32(mlp))[0]
    x, p = _boundary_row()
    row = sr.Row(x, 1.0, 0, p)
    assert row.keep[[5, 9, 30]].tolist() == [True, True, False] and sr.Row(x, 1.0, 0, p, mut="topp_strict").keep[9] == 0
    for t in range(64):
        tok, lp = row.draw(seed, 0, t)
        assert row.accept(seed, 0, t, tok, np.float32(lp))[0]
        mtok, mlp = sr.Row(x, 1.0, 0, p, mut="topp_strict").draw(seed, 0, t)
        rejected["topp_strict"] += not row.accept(seed, 0, t, mtok, np.float32(mlp))[0]
    assert all(n > 0 for n in rejected.values()), rejected


def test_generators_reject_fewer_than_one_percent():
    """With the reference alone: the rows the GPU tests use (same seeds) are redrawn in fewer than 1 % of the cases."""
    made = rej = 0
    for gi, (kind, T, k, p) in enumerate(sr.parameter_grid()):
        if p >= 1.0:
            continue   # no top-p, nothing to reject
        _, rows, r = sr.make_rows(kind, sr.ROWS_PER_CASE, sr.GRID_SEED0 + gi, T, k, p)
        made += len(rows) + r
        rej += r
    assert made >= 100 and rej < 0.01 * made, (rej, made)


def test_sample_argument_errors_no_cpu_fallback_and_signatures():
    import rgrg_amd
    from rgrg_amd import _hip
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.load_state_dict(synth_sd("bench"))
    m.eval()
    feats = torch.zeros((2, 1024))
    images = torch.zeros((1, 1, 512, 512))
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
                dict(num_return_sequences=0)):
        with pytest.raises(ValueError):
            m.language_model.sample(feats, 8, **bad)
        with pytest.raises(ValueError):
            m.sample(images, 8, **bad)
    with pytest.raises(_hip.RgrgHipError, match="no CPU fallback"):
        m.language_model.sample(feats, 8)
    with pytest.raises(_hip.RgrgHipError, match="no CPU fallback"):
        m.sample(images, 8)
    for fn, first in ((m.language_model.sample, "image_hidden_states"), (m.sample, "images")):
        ps = inspect.signature(fn).parameters
        assert list(ps) == [first, "max_length", "temperature", "top_k", "top_p", "num_return_sequences", "seed", "return_logprobs"]
        assert ps["max_length"].default is None
        assert all(ps[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(ps)[2:])
        assert [ps[n].default for n in list(ps)[2:]] == [1.0, 0, 1.0, 1, None, False]
    with pytest.raises(NotImplementedError, match="Multinomial"):   # generate() is unchanged
        m.language_model.generate(feats, 8, do_sample=True)
