"""CPU checks of the beam-sampling contract's reference (tests/beam_sample_reference.py): its selection follows Plackett-Luce, its
acceptance rule rejects each deliberate mutation of the contract, its generators redraw fewer than 1 % of the fixed inputs, and the
Python entries refuse bad arguments before any GPU work."""
import inspect

import numpy as np
import pytest
import torch

import beam_sample_reference as bsr
import sample_reference as sr
from conftest import synth_sd


def test_philox_words_match_the_scalar_generator():
    w = bsr.noise_words(0x0123456789ABCDEF, np.array([3, 70000]), 9, 11)
    for ri, r in enumerate((3, 70000)):
        for i in range(11):
            ref = sr.philox4x32_10((r, 9, i >> 2, 1), (0x89ABCDEF, 0x01234567))[i & 3]
            assert int(w[ri, i]) == ref
    assert not np.array_equal(w, bsr.noise_words(0x0123456789ABCDEF, np.array([3, 70000]), 9, 11, c3=0))


def test_noise_is_finite_at_both_ends_of_u():
    """n = 0 and n = 2^24 - 1: u = 2^-25 and 1 - 2^-25; an fp32 rounding of u would make the second one 1 and g infinite."""
    words = np.array([0, 0xFFFFFFFF, 0x7FFFFF00, 0x80000000], dtype=np.uint64)
    g64, g32 = bsr.gumbel64(words), bsr.gumbel32(words)
    assert np.isfinite(g64).all() and np.isfinite(g32).all()
    assert abs(g64[0] + np.log(25 * np.log(2))) < 1e-12 and abs(g64[1] - 25 * np.log(2)) < 1e-6
    assert np.abs(g32 - g64).max() < 4e-6


@pytest.mark.parametrize("seed", [bsr.PL_SEED])
def test_selection_follows_plackett_luce(seed):
    """nb = 2, V = 3, 16384 items: chi-square of the 15 unordered 4-of-6 sets against the exact probabilities of sequential draws
    without replacement <= 54.64 (the 1e-6 upper quantile at 14 degrees of freedom)."""
    sets = bsr.pl_reference_sets(seed)
    # the vectorised selection is Item.select's
    x, bs = bsr.pl_inputs()
    for s in (0, 1, 77):
        item = bsr.Item([bsr.BeamRow(x[j], bs[j], seed=seed, r=2 * s + j, t=0) for j in range(2)])
        _, tok, beam = item.select()
        assert sorted((beam * 3 + tok).tolist()) == sorted(sets[s].tolist())
    chi = bsr.pl_chi_square(sets)
    print(f"PLACKETT-LUCE reference seed {seed}: chi-square {chi:.2f} (bound {bsr.PL_BOUND})")
    assert abs(sum(bsr.pl_exact().values()) - 1.0) < 1e-12 and len(bsr.pl_exact()) == 15
    assert chi <= bsr.PL_BOUND


def test_reference_accepts_itself_on_every_case():
    for i, case in enumerate(bsr.rank_cases()):
        if case[2] > 1000 and case[4] * case[5] > 4:
            continue   # the large cases are judged on the device; two per shape are enough here
        _, _, items, _ = bsr.case_items(i)
        for item in items:
            ok, msg = item.accept(*item.select())
            assert ok, (case[0], msg)


MUT_PARAMS = dict(sampler_counter=(1.0, 0, 1.0), no_noise=(1.0, 0, 1.0), warp_after_score=(0.5, 0, 1.0), min_keep_1=(1.0, 1, 1.0),
                  order_by_key=(1.0, 0, 1.0))


@pytest.mark.parametrize("mut", sorted(MUT_PARAMS))
def test_acceptance_rule_rejects_mutation(mut):
    """Three items of 4 rows, V = 257: what the mutated contract selects is rejected by the rule of the true one (and the true
    selection accepted)."""
    T, k, p = MUT_PARAMS[mut]
    x, bs, items, _ = bsr.make_items("peaked", 3, 4, 500, T, k, p, V=257, noise_seed=77, step=2)
    rejected = 0
    for s, item in enumerate(items):
        assert item.accept(*item.select())[0]
        if mut == "order_by_key":
            got = item.select(mut=mut)
        else:
            got = bsr.Item([bsr.BeamRow(x[s * 4 + j], bs[s * 4 + j], T, k, p, 77, s * 4 + j, 2, mut=mut) for j in range(4)]).select()
        ok, msg = item.accept(*got)
        rejected += not ok
    assert rejected == len(items), (mut, rejected)


def test_generators_redraw_fewer_than_one_percent():
    made = rej = 0
    for i in range(len(bsr.rank_cases())):
        _, _, items, r = bsr.case_items(i)
        made += len(items) + r
        rej += r
    # ... and over many more items of the small shapes, where a redraw would show
    for seed in range(40):
        _, _, items, r = bsr.make_items("peaked", 8, 4, 9000 + seed, 1.0, 0, 1.0, V=257, noise_seed=seed)
        made += len(items) + r
        rej += r
    print(f"BEAM-SAMPLE generators: {rej} of {made} items redrawn")
    assert made >= 300 and rej < 0.01 * made, (rej, made)


def test_first_step_band_is_not_inflated_by_the_minus_1e9_rows():
    x, bs, items, _ = bsr.make_items("peaked", 1, 4, 11, 1.0, 0, 1.0, V=257, pattern="first")
    assert bs[1] == -1e9 and items[0].band < 1e-4


@pytest.fixture(scope="module")
def model():
    import rgrg_amd
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.load_state_dict(synth_sd("bench"))
    m.eval()
    return m


BAD = [dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1), dict(top_k=1.5), dict(top_p=0.0), dict(top_p=1.5),
       dict(num_return_sequences=0), dict(num_return_sequences=5), dict(num_beams=1), dict(num_beams=17), dict(num_beams=2.5),
       dict(max_length=None)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for d in BAD for k, v in d.items()])
def test_python_argument_errors(model, bad):
    kw = dict(max_length=8, num_beams=4)
    kw.update(bad)
    L, nb = kw.pop("max_length"), kw.pop("num_beams")
    with pytest.raises(ValueError):
        model.language_model.beam_sample(torch.zeros(2, 1024), L, nb, **kw)
    with pytest.raises(ValueError):
        model.generate_beam_sample(torch.zeros(1, 1, 512, 512), L, nb, **kw)


def test_prompt_argument_errors_no_cpu_fallback_and_signature(model):
    lm = model.language_model
    f = torch.zeros(2, 1024)
    ids, am = torch.zeros((2, 3), dtype=torch.int64), torch.ones((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="together"):
        lm.beam_sample(f, 8, 4, input_ids=ids)
    with pytest.raises(ValueError, match="max_length"):
        lm.beam_sample(f, 3, 4, input_ids=ids, attention_mask=am)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.beam_sample(f, 8, 4, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.beam_sample(f, 8, 4, input_ids=ids, attention_mask=am)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.generate_beam_sample(torch.zeros(1, 1, 512, 512), 8, 4)
    ps = inspect.signature(lm.beam_sample).parameters
    assert list(ps) == ["image_hidden_states", "max_length", "num_beams", "temperature", "top_k", "top_p", "seed", "early_stopping",
                        "num_return_sequences", "length_penalty", "input_ids", "attention_mask"]
    assert all(ps[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(ps)[3:])
    assert [ps[n].default for n in list(ps)[3:]] == [1.0, 0, 1.0, None, False, 1, 1.0, None, None]
    # generate() keeps the reference's mode table
    with pytest.raises(NotImplementedError, match="Beam-search multinomial sampling is not implemented."):
        lm.generate(f, 8, num_beams=4, do_sample=True)


def test_c_refusals_carry_a_message():
    """RGRG_EINVAL with a message, decided before the decoder or the GPU is touched."""
    import ctypes as C
    from rgrg_amd import _hip
    lib = _hip.load()
    n = C.c_int(0)
    for nb, keep, T, k, p, word in [(17, 1, 1.0, 0, 1.0, "at most 16"), (1, 1, 1.0, 0, 1.0, "more than one beam"),
                                    (4, 5, 1.0, 0, 1.0, "num_return_sequences"), (4, 1, 0.0, 0, 1.0, "temperature"),
                                    (4, 1, float("nan"), 0, 1.0, "temperature"), (4, 1, 1.0, -1, 1.0, "top_k"), (4, 1, 1.0, 0, 0.0, "top_p")]:
        rc = lib.rgrg_decoder_beam_sample(None, None, 1, nb, 8, 0, 1.0, keep, T, k, p, 1, None, 8, C.byref(n), None)
        assert rc != 0 and word in lib.rgrg_last_error().decode(), (nb, keep, T, k, p, lib.rgrg_last_error())
        rc = lib.rgrg_decoder_beam_sample_prompted(None, None, None, None, 1, 3, nb, 8, 0, 1.0, keep, T, k, p, 1, None, 8, C.byref(n), None)
        assert rc != 0 and word in lib.rgrg_last_error().decode()
    assert lib.rgrg_debug_beam_sample_rank(None, 8, 8, 1, 17, None, 1.0, 0, 1.0, 1, 0, 0, None, None, None, None, None, None, None) != 0
