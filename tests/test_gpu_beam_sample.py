"""Beam-search sampling on the MI355X (rgrg_decoder_beam_sample[_prompted]; LanguageModel.beam_sample,
ReportGenerationModel.generate_beam_sample): the ranking alone, through rgrg_debug_beam_sample_rank, judged by the acceptance rule
of tests/beam_sample_reference.py on every shape and parameter of rank_cases(); its distribution against Plackett-Luce; fp32
sequences against the CPU loop at a seed whose every decision has a margin >= 2e-3; determinism, graph replay, prompts; the 16-bit
plans and the e4m3 cache for structure only; refusals; the model-level entry."""
import numpy as np
import pytest
import torch

import beam_sample_reference as bsr
from conftest import gpu_model, synth_sd
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = PAD = 50256
POISON = 3.0e38   # in the columns V .. ld - 1, which the kernel must not read: as a logit it would win every ranking


def _engine():
    return gpu_model("ragged").engine()


def _rank(x, bs, nb, ld, T, k, p, seed, step, row0, row_lists=False):
    R, V = x.shape
    logits = torch.full((R, ld), POISON, dtype=torch.float32)
    logits[:, :V] = torch.from_numpy(x)
    out = _engine().beam_sample_rank(logits.to(DEV), torch.from_numpy(bs).to(DEV), nb, T, k, p, seed, step, row0, ld=ld, vocab=V,
                                     row_lists=row_lists)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


# ------------------------------------------------------------------------------------------------ 1. the ranking alone
CASES = bsr.rank_cases()


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c[0] for c in CASES])
def test_rank_against_the_contract(index):
    name, kind, V, ld, nb, S, T, k, p, pattern = CASES[index]
    x, bs, items, _ = bsr.case_items(index)
    score, tok, beam, rkey, rs, rtok = _rank(x, bs, nb, ld, T, k, p, bsr.CASE_NOISE_SEED, bsr.CASE_STEP, bsr.CASE_ROW0, row_lists=True)
    K = 2 * nb
    for s, item in enumerate(items):
        ok, msg = item.accept(score[s], tok[s], beam[s])
        assert ok, (name, s, msg)
        # the row lists: key descending, every finite entry a kept token with its s; the item's candidates come from them
        for j in range(nb):
            r = s * nb + j
            keys, toks = rkey[r, :K], rtok[r, :K]
            assert (keys[:-1] >= keys[1:]).all(), (name, r, keys.tolist())
            live = np.isfinite(keys)
            assert live.sum() == min(K, int(item.rows[j].keep.sum())), (name, r, int(live.sum()))
            assert item.rows[j].keep[toks[live]].all() and len(set(toks[live].tolist())) == int(live.sum())
            row = item.rows[j]   # the keys: 8 x the fp32 error of the row's key expression (over all its tokens: a row may keep two) + one ulp
            ref = row.key[toks[live]]
            tol = bsr.MARGIN * row.err_row + float(np.spacing(np.float32(np.abs(ref).max())))
            assert (np.abs(keys[live].astype(np.float64) - ref) <= tol).all(), (name, r, tol)
            assert (np.abs(rs[r, :K][live].astype(np.float64) - row.s[toks[live]]) <= tol).all(), (name, r, tol)
            mine = tok[s][beam[s] == j]
            assert set(mine.tolist()) <= set(toks[live].tolist())


def test_rank_is_deterministic_and_reads_its_counter():
    name, kind, V, ld, nb, S, T, k, p, pattern = CASES[0]
    x, bs, items, _ = bsr.case_items(0)
    a = _rank(x, bs, nb, ld, T, k, p, 5, 3, 0)
    b = _rank(x, bs, nb, ld, T, k, p, 5, 3, 0)
    assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(a, b))
    for other in ((6, 3, 0), (5, 4, 0), (5, 3, 1)):   # seed, step, row0
        c = _rank(x, bs, nb, ld, T, k, p, *other)
        assert not np.array_equal(a[1], c[1]), other


# ------------------------------------------------------------------------------------------------ 2. the distribution
def test_distribution_is_plackett_luce():
    """nb = 2, V = 3, 16384 items in ONE launch at seed 1234, step 0: chi-square of the 15 unordered 4-of-6 sets against the exact
    probabilities of sequential draws without replacement <= 54.64 (the 1e-6 upper quantile at 14 degrees of freedom)."""
    x, bs = bsr.pl_inputs()
    score, tok, beam = _rank(x, bs, 2, 3, 1.0, 0, 1.0, bsr.PL_SEED, 0, 0)
    sets = beam.astype(np.int64) * 3 + tok
    assert sets.shape == (bsr.PL_ITEMS, 4) and (np.sort(sets, 1)[:, 1:] != np.sort(sets, 1)[:, :-1]).all()
    chi = bsr.pl_chi_square(sets)
    same = (np.sort(sets, 1) == np.sort(bsr.pl_reference_sets(), 1)).all(1).mean()
    print(f"PLACKETT-LUCE device seed {bsr.PL_SEED}: chi-square {chi:.2f} (bound {bsr.PL_BOUND}); sets equal to the reference's {same:.5f}")
    assert chi <= bsr.PL_BOUND
    assert (score[:, :-1] >= score[:, 1:]).all()


# ------------------------------------------------------------------------------------------------ 3. end to end, fp32
@pytest.mark.parametrize("early", [False, True])
def test_fp32_ids_equal_the_cpu_loop(early):
    """S = 2, nb = 4, max_length 12, num_return_sequences 4, synthetic weights: at the first seed of the walk at which every decision
    of the CPU run (K-th against (K+1)-th key, adjacent s among the chosen, the scorer's is_done / heap / final-order comparisons)
    has a margin >= 2e-3, the device ids are the loop's."""
    c = bsr.E2E
    r = bsr.e2e_reference(synth_sd, early)
    print(f"BEAM-SAMPLE e2e early={early}: seed {r['seed']} ({r['tried']} tried), margins " +
          ", ".join(f"{k} {v:.4g}" for k, v in r["margins"].items()))
    lm = gpu_model(c["profile"]).language_model
    got = lm.beam_sample(r["feats"].to(DEV), c["L"], c["nb"], temperature=c["temperature"], top_k=c["top_k"], top_p=c["top_p"],
                         seed=r["seed"], early_stopping=early, num_return_sequences=c["keep"]).cpu()
    assert got.dtype == torch.int64 and torch.equal(got, r["seq"]), (got.tolist(), r["seq"].tolist())


# ------------------------------------------------------------------------------------------------ 4. other behaviour
def _feats(S, seed):
    return torch.randn((S, 1024), generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_seed_determinism_graph_replay_and_other_seed():
    lm = gpu_model("ragged").language_model
    feats = _feats(3, 91)
    kw = dict(temperature=0.9, top_k=50, top_p=0.95, num_return_sequences=4)
    plain = lm.generate(feats, max_length=10, num_beams=4, num_return_sequences=4)
    first = lm.beam_sample(feats, 10, 4, seed=11, **kw)      # captures the step (or replays an earlier test's)
    again = lm.beam_sample(feats, 10, 4, seed=11, **kw)      # replays it
    assert first.dtype == torch.int64 and first.shape[0] == 12 and torch.equal(first, again)
    other = lm.beam_sample(feats, 10, 4, seed=12, **kw)      # the same graph, another seed in the device block
    L = min(first.shape[1], other.shape[1])
    assert first.shape != other.shape or not torch.equal(first[:, :L], other[:, :L])
    assert torch.equal(lm.beam_sample(feats, 10, 4, seed=11, **kw), first)
    # the plain beam step of the same rows has a graph of its own
    assert torch.equal(lm.generate(feats, max_length=10, num_beams=4, num_return_sequences=4), plain)
    torch.manual_seed(1234)
    a = lm.beam_sample(feats, 10, 4, **kw)
    torch.manual_seed(1234)
    assert torch.equal(lm.beam_sample(feats, 10, 4, **kw), a)   # seed=None: torch's CPU generator


def test_bos_prompt_equals_unprompted():
    lm = gpu_model("ragged").language_model
    feats = _feats(3, 92)
    bos = torch.full((3, 1), EOS, dtype=torch.int64, device=DEV)
    kw = dict(temperature=0.8, top_k=0, top_p=0.9, seed=21, num_return_sequences=4)
    ref = lm.beam_sample(feats, 9, 4, **kw)
    got = lm.beam_sample(feats, 9, 4, input_ids=bos, attention_mask=torch.ones_like(bos), **kw)
    assert torch.equal(got, ref)


def test_left_padded_ragged_prompt():
    lm = gpu_model("ragged").language_model
    S, T, nb = 3, 4, 4
    feats = _feats(S, 93)
    ids = torch.randint(0, 50000, (S, T), generator=torch.Generator().manual_seed(94))
    mask = torch.ones((S, T), dtype=torch.int64)
    for s, pad in enumerate((0, 1, 3)):
        mask[s, :pad] = 0
        ids[s, :pad] = EOS
    kw = dict(temperature=1.0, top_k=100, seed=31, num_return_sequences=nb, input_ids=ids.to(DEV), attention_mask=mask.to(DEV))
    got = lm.beam_sample(feats, 10, nb, **kw).cpu()
    assert got.shape[0] == S * nb and T + 1 <= got.shape[1] <= 10
    assert torch.equal(got[:, :T], ids.repeat_interleave(nb, 0))
    assert torch.equal(lm.beam_sample(feats, 10, nb, **kw).cpu(), got)


# ------------------------------------------------------------------------------------------------ 5. the 16-bit plans
def _structure(ids, rows, L):
    """int64 [rows, <= L]; BOS in front; behind a row's first generated EOS nothing but PAD."""
    assert ids.dtype == torch.int64 and ids.shape[0] == rows and 2 <= ids.shape[1] <= L
    assert (ids[:, 0] == EOS).all() and ((ids >= 0) & (ids <= 50256)).all()
    for row in ids.tolist():
        if EOS in row[1:]:
            e = 1 + row[1:].index(EOS)
            assert all(t == PAD for t in row[e:])


@pytest.mark.parametrize("kv", [None, "fp8_e4m3"])
def test_16bit_plan_and_e4m3_cache(kv):
    """17 items x 4 beams = 68 beam rows under bf16 autocast, above the fused plans' 64: the 16-bit cache, or its e4m3 form.  Shape,
    determinism and EOS / PAD structure only: against fp32 a 16-bit beam-sampling run agrees in distribution, not id by id - one
    flipped draw changes every later one - so parity with fp32 is statistical and not asserted here."""
    m = gpu_model("ragged")
    lm = m.language_model
    S, nb, L = 17, 4, 9
    feats = _feats(S, 95)
    lm.set_kv_cache_dtype(kv)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            a = lm.beam_sample(feats, L, nb, temperature=0.9, top_k=50, seed=41, num_return_sequences=2)
            b = lm.beam_sample(feats, L, nb, temperature=0.9, top_k=50, seed=41, num_return_sequences=2)
            assert m.engine().kv_format_in_use(S * nb) == (3 if kv else 1)
    finally:
        lm.set_kv_cache_dtype(None)
    assert torch.equal(a, b)
    _structure(a.cpu(), S * 2, L)


# ------------------------------------------------------------------------------------------------ 6. refusals, model level
def test_refusals_carry_their_message():
    m = gpu_model("ragged")
    lm, eng = m.language_model, m.engine()
    feats = _feats(2, 96)
    with pytest.raises(_hip.RgrgHipError, match="at most 16 beams"):
        eng.beam_sample(feats, 8, 17)
    with pytest.raises(_hip.RgrgHipError, match="num_return_sequences 5 outside 1 .. num_beams 4"):
        eng.beam_sample(feats, 8, 4, num_return_sequences=5)
    with pytest.raises(_hip.RgrgHipError, match="temperature has to be a finite float > 0"):
        eng.beam_sample(feats, 8, 4, temperature=0.0)
    with pytest.raises(_hip.RgrgHipError, match="temperature has to be a finite float > 0"):
        eng.beam_sample(feats, 8, 4, temperature=-1.0)
    ids = torch.zeros((2, 3), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="max_length has to be at least 4 for a prompt of 3 tokens"):
        eng.beam_sample_prompted(feats, ids, torch.ones_like(ids), 3, 4)
    with pytest.raises(ValueError, match="max_length has to be at least 4 for a prompt of 3 tokens"):
        lm.beam_sample(feats, 3, 4, input_ids=ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(ValueError, match="at most 16 beams"):
        lm.beam_sample(feats, 8, 17)
    with pytest.raises(NotImplementedError, match="Beam-search multinomial sampling is not implemented."):
        lm.generate(feats, 8, num_beams=4, do_sample=True)
    assert lm.beam_sample(feats, 6, 2, seed=1).shape[0] == 2   # the decoder is usable after the refusals


def test_generate_beam_sample():
    m = gpu_model("ragged")
    images = synth.make_images(2, 77).to(DEV)
    out = m.generate_beam_sample(images, 8, 4, temperature=0.9, top_k=50, seed=51, early_stopping=True, num_return_sequences=2)
    assert isinstance(out, tuple) and len(out) == 4
    seqs, sel, det, cd = out
    ref = m.generate(images, max_length=8)
    assert torch.equal(sel, ref[1]) and torch.equal(cd, ref[3]) and all(torch.equal(det[k], ref[2][k]) for k in ref[2])
    _, _, top_feats, cd2 = m.object_detector(images)
    _, feats = m.binary_classifier_region_selection(top_feats, cd2, return_loss=False)
    S = feats.shape[0]
    assert S > 0
    direct = m.language_model.beam_sample(feats, 8, 4, temperature=0.9, top_k=50, seed=51, early_stopping=True, num_return_sequences=2)
    assert seqs.shape[0] == 2 * S and torch.equal(seqs, direct)
    sd = dict(synth_sd("ragged"))
    sd["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m.load_state_dict(sd)
    m.to(DEV)
    try:
        assert m.generate_beam_sample(synth.make_images(1, 77).to(DEV), 8, 4, seed=51) == -1
    finally:
        m.load_state_dict(synth_sd("ragged"))
        m.to(DEV)
