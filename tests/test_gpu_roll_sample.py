"""Rolling-batch sampling end to end on the MI355X (rgrg_decoder_sample_rolling; LanguageModel.sample_rolling,
Engine.sample_decode_rolling, ReportGenerationModel.sample_rolling): S * n sampled sequences through R decoder rows give the ids and
log-probs of ``sample()`` bit for bit wherever both run the same step plan, whichever row decodes a sequence and when.

Setup of tests/test_gpu_rolling.py: the ``ragged`` synthetic weights with ``prompt_reference.eos_boosted(sd, 0.98)`` and its ROWS
feature rows.  Drawn at (temperature, top_k, top_p) = (0.6, 20, 0.8) the sequences are ragged (unfiltered draws at temperature 1
almost never emit EOS on these weights); every case first asserts that on ``sample()``'s own output, so that no case passes with
nothing to roll.

Equality with ``sample()`` is asserted only where both sides run ONE step plan - fp32: the fused plan up to 128 rows, the tiled plan
above; under autocast: the same number of rows.  It rests on a row's logits not depending on its position or its neighbours within a
plan.  Across plans the logits differ by rounding, a draw may differ with them, and nothing is claimed."""
import pytest
import torch

import prompt_reference as pr
from conftest import gpu_model, synth_sd
from rgrg_amd import _hip, synth
from test_gpu_rolling import BOOST, POOL, POOL_SEED, ROWS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = PAD = 50256
FILTER = dict(temperature=0.6, top_k=20, top_p=0.8)


def _sd():
    return pr.eos_boosted(synth_sd("ragged"), BOOST)


@pytest.fixture(scope="module")
def feats():
    return torch.randn((POOL, 1024), generator=torch.Generator().manual_seed(POOL_SEED))[ROWS].contiguous().to(DEV)


@pytest.fixture(scope="module")
def model():
    import rgrg_amd
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.load_state_dict(_sd())
    m.to(DEV).eval()
    yield m
    m.invalidate_engine()


def _lens(ids):
    """Tokens of every sequence, BOS and EOS included; a sequence without an EOS is as long as the output is wide."""
    hit = ids[:, 1:] == EOS
    first = torch.where(hit.any(1), hit.float().argmax(1) + 2, torch.full_like(hit[:, 0], ids.shape[1], dtype=torch.int64))
    return first.cpu()


def _something_to_roll(ids, L):
    lens = _lens(ids)
    assert len(set(lens.tolist())) >= 3 and int(lens.max()) == L and int(lens.min()) <= 4, sorted(lens.tolist())
    return lens


def _structure(ids, lp, L):
    """BOS column, PAD only behind EOS, as wide as the longest sequence, log-prob 0 in the BOS column and under PAD, <= 0 elsewhere."""
    lens = _lens(ids)
    assert ids.dtype == torch.int64 and lp.dtype == torch.float32 and ids.shape == lp.shape and ids.shape[1] == int(lens.max()) <= L
    assert (ids[:, 0] == EOS).all() and (lp[:, 0] == 0).all() and (lp <= 0).all()
    cols = torch.arange(ids.shape[1])[None, :]
    behind = cols >= lens[:, None]
    assert (ids.cpu()[behind] == PAD).all() and (lp.cpu()[behind] == 0).all()
    assert (ids.cpu()[(cols >= 1) & (cols < lens[:, None] - 1)] != EOS).all()   # an EOS is a sequence's last token
    return lens


CASES_F32 = [(11, 1, 4, 12, 7), (11, 1, 1, 6, 7), (6, 3, 5, 10, 17), (70, 1, 33, 8, 99), (140, 1, 129, 6, 99), (9, 1, 16, 10, 7)]


@pytest.mark.parametrize("S,n,R,L,seed", CASES_F32)
def test_rolling_equals_sample_on_the_same_plan_fp32(model, feats, S, n, R, L, seed):
    """4 rows and 1 row; 3 hypotheses per region through 5 rows; 33 rows = two row tiles of the fused plan; 129 rows = the tiled fp32
    plan on both sides (140 rows in ``sample()``); 9 sequences in 16 rows: no row is ever refilled."""
    lm, eng = model.language_model, model.engine()
    f = feats[:S]
    kw = dict(num_return_sequences=n, seed=seed, return_logprobs=True, **FILTER)
    ref, ref_lp = lm.sample(f, L, **kw)
    lens = _something_to_roll(ref, L)
    if n > 1:
        assert all(len({tuple(r.tolist()) for r in ref[s * n:(s + 1) * n]}) > 1 for s in range(S)), "hypotheses of a region coincide"
    got, lp = lm.sample_rolling(f, L, rows=R, **kw)
    steps = eng.last_rolling_steps
    assert eng.kv_format_in_use(R) == 0 and eng.fused_row_limit() == 128 and (S * n <= 128) == (R <= 128)
    Q, work = S * n, int((lens - 1).sum())
    bound = ((Q + R - 1) // R + 1) * (L - 1)
    print(f"ROLLSAMPLE S={S} n={n} R={R} L={L} lengths {sorted(lens.tolist())} steps {steps} longest {int(lens.max()) - 1} "
          f"work/R {work / R:.1f} bound {bound}")
    assert got.shape == ref.shape and torch.equal(got, ref), (got.tolist(), ref.tolist())
    assert torch.equal(lp.view(torch.int32), ref_lp.view(torch.int32)), (lp - ref_lp).abs().max().item()
    _structure(got, lp, L)
    assert max(int(lens.max()) - 1, -(-work // R)) <= steps <= bound
    if Q <= R:
        assert steps == int(lens.max()) - 1
    again, again_lp = lm.sample_rolling(f, L, rows=R, **kw)
    assert torch.equal(again, got) and torch.equal(again_lp.view(torch.int32), lp.view(torch.int32))
    eager, eager_lp = eng.sample_decode_rolling(f, L, R, FILTER["temperature"], FILTER["top_k"], FILTER["top_p"], seed, n, use_graph=False)
    assert torch.equal(eager, got) and torch.equal(eager_lp.view(torch.int32), lp.view(torch.int32))


@pytest.mark.parametrize("S,R,L", [(11, 4, 12), (140, 129, 6)])
def test_top_k_1_equals_greedy_fp32(model, feats, S, R, L):
    lm = model.language_model
    f = feats[:S]
    ids, lp = lm.sample_rolling(f, L, rows=R, top_k=1, seed=5, return_logprobs=True)
    assert torch.equal(ids, lm.generate_rolling(f, L, rows=R)) and torch.equal(ids, lm.generate(f, L))
    _structure(ids, lp, L)
    assert torch.equal(lm.sample_rolling(f, L, rows=R, top_k=1, seed=6), ids)       # no random word enters


def test_logprobs_match_the_teacher_forced_pass(model, feats):
    """The rule of tests/test_gpu_sample.py::test_logprobs_match_the_teacher_forced_pass with its 2e-3 bound (what the existing tests
    put on both fp32 passes' logits against one oracle): temperature 1, no filters, 5 sequences through 2 rows."""
    lm = model.language_model
    f = feats[:5]
    ids, lp = lm.sample_rolling(f, 12, rows=2, seed=4, return_logprobs=True)
    am = torch.ones_like(ids, dtype=torch.float32)
    ref = torch.log_softmax(lm.teacher_forced_logits(ids, am, f).double(), -1)
    got = ref[:, :-1].gather(2, ids[:, 1:, None])[..., 0]
    live = torch.cat([torch.ones_like(ids[:, :1], dtype=torch.bool), (ids[:, 1:-1] == PAD).cumsum(1) == 0], 1)
    err = (got - lp[:, 1:].double()).abs()[live].max().item()
    print(f"ROLLSAMPLE largest |log-prob - teacher-forced log-softmax|: {err:.3e} over {int(live.sum())} tokens")
    assert err <= 2e-3, err
    assert (lp[:, 1:][~live] == 0).all()


@pytest.mark.parametrize("dtype,S,R,L", [(torch.float16, 90, 40, 9), (torch.bfloat16, 150, 70, 9), (torch.float16, 150, 70, 9)])
def test_rolling_16bit_plans(model, feats, dtype, S, R, L):
    """The plan follows R: 40 rows under fp16 = the fused plan on 16-bit weight fragments (fp32 cache); 70 rows = the many-sequence step
    on the 16-bit cache.  No agreement across plans is claimed: S sequences through R rows are checked for determinism and structure,
    the first R sequences through R rows against ``sample()`` of R rows under the same autocast - the same rows, plan and order of work."""
    lm, eng = model.language_model, model.engine()
    f = feats[:S]
    kw = dict(seed=99, return_logprobs=True, **FILTER)
    with torch.autocast("cuda", dtype=dtype):
        got, lp = lm.sample_rolling(f, L, rows=R, **kw)
        steps = eng.last_rolling_steps
        again, again_lp = lm.sample_rolling(f, L, rows=R, **kw)
        assert eng.fused_row_limit() == 64
        assert eng.kv_format_in_use(R) == (0 if R <= 64 else (2 if dtype == torch.float16 else 1))
        lock, lock_lp = lm.sample_rolling(f[:R], L, rows=R, **kw)
        ref, ref_lp = lm.sample(f[:R], L, **kw)
    assert torch.equal(got, again) and torch.equal(lp.view(torch.int32), again_lp.view(torch.int32))
    _something_to_roll(ref, L)
    assert torch.equal(lock, ref), (lock.tolist(), ref.tolist())
    assert torch.equal(lock_lp.view(torch.int32), ref_lp.view(torch.int32))
    assert got.shape[0] == S
    lens = _structure(got, lp, L)
    work = int((lens - 1).sum())
    print(f"ROLLSAMPLE16 {dtype} S={S} R={R} lengths {sorted(set(lens.tolist()))} steps {steps} work/R {work / R:.1f}")
    assert max(int(lens.max()) - 1, -(-work // R)) <= steps <= ((S + R - 1) // R + 1) * (L - 1)


def test_hypotheses_share_the_image_row(model, feats):
    lm = model.language_model
    f = feats[:6]
    kw = dict(rows=5, seed=17, return_logprobs=True, **FILTER)
    a, a_lp = lm.sample_rolling(f, 10, num_return_sequences=3, **kw)
    b, b_lp = lm.sample_rolling(f.repeat_interleave(3, 0), 10, num_return_sequences=1, **kw)
    assert a.shape[0] == 18 and torch.equal(a, b) and torch.equal(a_lp.view(torch.int32), b_lp.view(torch.int32))


def test_rows_default_and_manual_seed(model, feats):
    lm = model.language_model
    f = feats[:5]
    ref = lm.sample(f, 8, seed=7, num_return_sequences=2, **FILTER)
    assert torch.equal(lm.sample_rolling(f, 8, seed=7, num_return_sequences=2, **FILTER), ref)     # rows=None: min(S * n, what fits) = 10
    assert model.engine().last_rolling_steps == ref.shape[1] - 1
    torch.manual_seed(123)
    a = lm.sample_rolling(f, 8, rows=3, **FILTER)
    b = lm.sample_rolling(f, 8, rows=3, **FILTER)
    torch.manual_seed(123)
    assert torch.equal(lm.sample_rolling(f, 8, rows=3, **FILTER), a) and not torch.equal(a, b)     # seed=None: torch's CPU generator


def test_refusals(model, feats):
    lm = model.language_model
    f = feats[:6]
    with pytest.raises(ValueError, match="max_length"):
        lm.sample_rolling(f, None)
    with pytest.raises(ValueError, match="max_length"):
        lm.sample_rolling(f, 1)
    with pytest.raises(ValueError, match="rows"):
        lm.sample_rolling(f, 6, rows=0)
    with pytest.raises(ValueError, match="temperature"):
        lm.sample_rolling(f, 6, temperature=0.0)
    with pytest.raises(ValueError, match="top_k"):
        lm.sample_rolling(f, 6, top_k=-1)
    with pytest.raises(ValueError, match="top_p"):
        lm.sample_rolling(f, 6, top_p=0.0)
    with pytest.raises(ValueError, match="num_return_sequences"):
        lm.sample_rolling(f, 6, num_return_sequences=0)
    images = synth.make_images(1, 1234).to(DEV)
    with pytest.raises(ValueError, match="rows"):
        model.sample_rolling(images, 6, rows=-2)                                       # before the detector runs
    with pytest.raises(ValueError, match="top_p"):
        model.sample_rolling(images, 6, top_p=1.5)
    with pytest.raises(_hip.RgrgHipError, match="no CPU fallback"):
        lm.sample_rolling(f.cpu(), 6)
    with pytest.raises(_hip.RgrgHipError, match="rows"):
        lm.sample_rolling(f, 6, rows=10 ** 6)                                          # more rows than any cache holds
    # the C entry's own bounds: rows above the decoder's cache, max_length above its slots, no hypotheses
    eng = model.engine()
    lm.sample_rolling(f, 6, rows=4)
    dec, (cap_s, cap_l) = eng._decoder, eng._decoder_caps
    out = torch.empty((6, 6), dtype=torch.int64, device=DEV)
    lens = torch.empty((6,), dtype=torch.int32, device=DEV)
    lib = _hip.load()
    call = lambda n, R, L, T=1.0: lib.rgrg_decoder_sample_rolling(dec, f.data_ptr(), 6, n, R, L, T, 0, 1.0, 1, out.data_ptr(), None,   # noqa: E731
                                                                  lens.data_ptr(), None, 1, None)
    assert call(1, cap_s + 1, 6) != 0 and b"decoder rows" in lib.rgrg_last_error()
    assert call(1, 0, 6) != 0 and call(1, 4, cap_l + 1) != 0 and call(1, 4, 1) != 0 and call(0, 4, 6) != 0 and call(1, 4, 6, 0.0) != 0
    assert call(1, 4, 6) == 0                                                          # (log-probs are optional in the C entry)
    # the e4m3 cache where it would be used (16-bit mode, more rows than the fused plan takes): refused with generate_rolling's message
    ref = lm.sample_rolling(f, 6, rows=4, seed=3, **FILTER)
    lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with pytest.raises(_hip.RgrgHipError, match="e4m3 K/V cache has no per-row step"):
                lm.sample_rolling(feats[:80], 6, rows=70)
            assert lm.sample_rolling(f, 6, rows=4).shape[0] == 6        # 4 rows keep an fp32 cache: the setting has no effect there
    finally:
        lm.set_kv_cache_dtype(None)
    assert torch.equal(lm.sample_rolling(f, 6, rows=4, seed=3, **FILTER), ref)   # still works afterwards


def test_report_model_sample_rolling_matches_sample():
    import rgrg_amd
    m = gpu_model("ragged")
    images = synth.make_images(2, 1234).to(DEV)
    ref = m.sample(images, 8, top_k=50, seed=3, return_logprobs=True)
    got = m.sample_rolling(images, 8, rows=16, top_k=50, seed=3, return_logprobs=True)
    assert isinstance(got, tuple) and len(got) == 4
    (ids, lp), sel, det, cd = got
    assert torch.equal(sel, ref[1]) and torch.equal(cd, ref[3])
    assert sorted(det) == sorted(ref[2]) and all(torch.equal(det[k], ref[2][k]) for k in ref[2])
    assert ids.shape[0] == ref[0][0].shape[0] and lp.shape == ids.shape and ids.dtype == torch.int64
    g = m.generate(images, 8)
    one = m.sample_rolling(images, 8, rows=16, top_k=1)
    assert torch.equal(one[0], g[0]) and torch.equal(one[1], g[1])
    print(f"ROLLSAMPLE report model: {ids.shape[0]} selected regions through 16 rows")
    # nothing selected: the -1 of sample()
    sd0 = dict(synth_sd("ragged"))
    sd0["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m0 = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m0.load_state_dict(sd0)
    m0.to(DEV).eval()
    try:
        assert m0.sample_rolling(images[:1], 6, rows=4) == -1
    finally:
        m0.invalidate_engine()
