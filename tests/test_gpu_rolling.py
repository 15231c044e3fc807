"""Rolling-batch greedy decoding end to end on the MI355X (rgrg_decoder_generate_rolling; LanguageModel.generate_rolling,
Engine.greedy_decode_rolling, ReportGenerationModel.generate_rolling): S sequences through R decoder rows give the ids of
``generate()`` - on every step plan, graph and eager - and the refusals.

Weights: the ``ragged`` synthetic profile with ``prompt_reference.eos_boosted(sd, 0.98)``.  Feature rows: ROWS, 150 rows of
``torch.randn((400, 1024), seed 777)`` (the first S of them make a case), chosen once on the CPU with the oracle's greedy search at
max_length 12 so that, for every prefix of 9 rows or more and every max_length used here,
  * the sequences have at least three distinct lengths (the first 11 at max_length 12: 12, 3, 2, 12, 7, 2, 12, 5, 2, 12, 3),
  * at least one reaches max_length without an EOS and at least one ends within three tokens,
  * the oracle's smallest top-2 logit gap over all steps of an unfinished row is 0.0201 >= 10 x the 2e-3 logit tolerance of
    tests/test_gpu_lm_forms.py, so no plan's rounding changes an arg-max in fp32.
(The tokens behind a row's EOS are PAD by bookkeeping, not by arg-max: their gaps do not count.)  Rows decode independently, so a
row's sequence at a smaller max_length is the prefix of its sequence at 12; ``test_feature_rows_meet_the_conditions`` re-checks all
of it from the one oracle run the other tests share."""
import pytest
import torch

import prompt_reference as pr
from conftest import gpu_model, synth_sd
from oracle import language_model as o_lm
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = 50256
BOOST, POOL, POOL_SEED, L_MAX = 0.98, 400, 777, 12
ROWS = [10, 42, 1, 28, 43, 2, 34, 44, 4, 38, 46, 6, 55, 58, 7, 60, 109, 8, 66, 111, 11, 79, 117, 12, 82, 141, 13, 125, 152, 14, 133, 170, 15,
        135, 178, 16, 161, 190, 17, 174, 223, 18, 179, 229, 20, 194, 254, 22, 198, 294, 23, 247, 384, 24, 253, 385, 25, 263, 26, 27, 279,
        30, 31, 285, 32, 33, 298, 35, 37, 302, 41, 45, 336, 47, 48, 359, 49, 50, 363, 51, 52, 373, 53, 54, 380, 57, 59, 381, 61, 62, 391, 63,
        65, 67, 70, 72, 76, 77, 78, 80, 81, 84, 85, 86, 89, 90, 91, 92, 94, 95, 96, 97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 110,
        113, 114, 115, 116, 119, 121, 122, 123, 124, 127, 128, 129, 130, 131, 132, 134, 136, 138, 139, 140, 142, 143, 144, 145, 146, 147,
        148]
TOL_LOGIT = 2e-3   # tests/test_gpu_lm_forms.py


def _sd():
    return pr.eos_boosted(synth_sd("ragged"), BOOST)


@pytest.fixture(scope="module")
def feats():
    return torch.randn((POOL, 1024), generator=torch.Generator().manual_seed(POOL_SEED))[ROWS].contiguous()


@pytest.fixture(scope="module")
def oracle(feats):
    """The oracle's greedy search over all 150 rows at max_length 12, once: ids [150, 12], per-step logits, lengths."""
    ids, logits = o_lm.greedy_generate(_sd(), feats, L_MAX, return_logits=True)
    assert ids.shape[1] == L_MAX
    lens = []
    for row in ids[:, 1:].tolist():
        lens.append(1 + (row.index(EOS) + 1 if EOS in row else len(row)))
    return {"ids": ids, "logits": logits, "lens": torch.tensor(lens)}


def _oracle_ids(oracle, S, L):
    """generate()'s result for the first S rows at max_length L, from the run at 12: the prefix, PAD behind a row's EOS, as wide as
    the longest sequence."""
    lens = oracle["lens"][:S].clamp(max=L)
    return oracle["ids"][:S, :int(lens.max())].clone(), lens


@pytest.fixture(scope="module")
def model():
    import rgrg_amd
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.load_state_dict(_sd())
    m.to(DEV).eval()
    yield m
    m.invalidate_engine()


CASES_F32 = [(11, 4, 12), (11, 1, 6), (70, 33, 8), (140, 129, 6), (9, 16, 10), (12, 12, 12)]
CASES_16 = [(torch.float16, 90, 40, 9, 6e-3), (torch.bfloat16, 150, 70, 9, 3e-2), (torch.float16, 150, 70, 9, 6e-3)]


def test_feature_rows_meet_the_conditions(oracle):
    gap = oracle["logits"].topk(2, dim=-1).values
    gap = gap[..., 0] - gap[..., 1]
    live = torch.arange(L_MAX - 1)[None, :] < (oracle["lens"] - 1)[:, None]
    print(f"ROLLING smallest top-2 gap of an unfinished row {gap[live].min().item():.4f}, logit range {oracle['logits'].abs().max().item():.3f}")
    assert gap[live].min().item() >= 10 * TOL_LOGIT
    for S, L in sorted({(S, L) for S, _, L in CASES_F32} | {(S, L) for _, S, _, L, _ in CASES_16}):
        ids, lens = _oracle_ids(oracle, S, L)
        no_eos = (lens == L) & (ids[:, L - 1] != EOS) if ids.shape[1] == L else torch.zeros(S, dtype=torch.bool)
        print(f"ROLLING S={S} L={L} lengths {sorted(set(lens.tolist()))} without EOS {int(no_eos.sum())} sum {int((lens - 1).sum())}")
        assert len(set(lens.tolist())) >= 3 and bool(no_eos.any()) and bool((lens <= 4).any())


def _roll(lm, feats, L, R, **kw):
    return lm.generate_rolling(feats.to(DEV), L, rows=R, **kw).cpu()


@pytest.mark.parametrize("S,R,L", CASES_F32)
def test_rolling_equals_generate_and_the_oracle_fp32(model, feats, oracle, S, R, L):
    """4 rows and 1 row (every sequence through the same row); 33 rows = two row tiles of the fused plan; 129 rows = the tiled fp32
    plan; S <= R (9 in 16 rows: no row is ever refilled, 7 idle from the start) and S = R."""
    lm = model.language_model
    f = feats[:S]
    got = _roll(lm, f, L, R)
    steps = model.engine().last_rolling_steps
    assert model.engine().kv_format_in_use(R) == 0 and model.engine().fused_row_limit() == 128
    ref = lm.generate(f.to(DEV), L).cpu()
    want, lens = _oracle_ids(oracle, S, L)
    assert got.dtype == torch.int64 and torch.equal(got, ref), (got.tolist(), ref.tolist())
    assert torch.equal(got, want)
    work = int((lens - 1).sum())
    print(f"ROLLING S={S} R={R} L={L} steps {steps} longest {int(lens.max()) - 1} work/R {work / R:.1f} bound {((S + R - 1) // R + 1) * (L - 1)}")
    assert max(int(lens.max()) - 1, -(-work // R)) <= steps <= ((S + R - 1) // R + 1) * (L - 1)
    if S <= R:
        assert steps == int(lens.max()) - 1
    assert torch.equal(_roll(lm, f, L, R), got)


def _rule_16bit(got, feats, tie_frac):
    """``_rule_16bit`` of tests/test_gpu_prompted.py for a BOS prompt: on the fp32 oracle, teacher-forced on the GPU's own history
    ``got``, every generated token is the oracle's arg-max at its position or within tie_frac x logit range of it."""
    S, Lh = got.shape
    am = torch.ones((S, Lh - 1), dtype=torch.int64)
    with torch.no_grad():
        logits, _ = o_lm.lm_forward(_sd(), got[:, :-1], am, feats, None, pr.positions_from_mask(am))
    rng = logits.abs().max().item()
    chosen = got[:, 1:]
    done = torch.zeros(S, dtype=torch.bool)
    for k in range(chosen.shape[1]):
        top = logits[:, k].max(-1).values
        margin = top - logits[:, k].gather(-1, chosen[:, k:k + 1]).squeeze(-1)
        bad = (margin > tie_frac * rng) & ~done   # PAD behind a row's EOS is bookkeeping, not a prediction
        print(f"ROLLING16 step={k} max margin {margin[~done].max().item() if (~done).any() else 0.0:.4e} of range {rng:.3f}")
        assert not bad.any(), (k, margin.tolist(), rng)
        done |= chosen[:, k] == EOS
    return rng


@pytest.mark.parametrize("dtype,S,R,L,tie", CASES_16)
def test_rolling_16bit_plans(model, feats, oracle, dtype, S, R, L, tie):
    """The plan follows R: 40 rows under fp16 = the fused plan on 16-bit weight fragments (fp32 cache); 70 rows under bf16 / fp16 = the
    many-sequence step on the 16-bit cache (attn_decode_kv16_wave_kernel<.., ROWSTEP>, which stores the new key / value itself)."""
    lm, eng = model.language_model, model.engine()
    f = feats[:S]
    with torch.autocast("cuda", dtype=dtype):
        got = _roll(lm, f, L, R)
        again = _roll(lm, f, L, R)
        assert eng.fused_row_limit() == 64
        assert eng.kv_format_in_use(R) == (0 if R <= 64 else (2 if dtype == torch.float16 else 1))
        # S <= R: the same rows, plan and order of work as generate() under the same autocast
        lock = _roll(lm, f[:R], L, R)
        ref = lm.generate(f[:R].to(DEV), L).cpu()
    assert torch.equal(got, again)
    assert torch.equal(lock, ref), (lock.tolist(), ref.tolist())
    assert got.shape[0] == S and got.shape[1] <= L and (got[:, 0] == EOS).all()
    _rule_16bit(got, f, tie)
    want, _ = _oracle_ids(oracle, S, L)
    print(f"ROLLING16 rows that differ from the fp32 oracle: {int((got[:, :want.shape[1]] != want[:, :got.shape[1]]).any(dim=1).sum())} of {S}")


def test_graph_equals_eager(model, feats):
    eng = model.engine()
    f = feats[:11].to(DEV)
    a = eng.greedy_decode_rolling(f, 12, 4, use_graph=True)
    b = eng.greedy_decode_rolling(f, 12, 4, use_graph=False)
    assert torch.equal(a, b)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        f = feats[:100].to(DEV)
        c = eng.greedy_decode_rolling(f, 7, 70, use_graph=True, bf16=1)
        d = eng.greedy_decode_rolling(f, 7, 70, use_graph=False, bf16=1)
    assert torch.equal(c, d)


def test_rows_default_and_more_sequences_than_generate_took(model, feats, oracle):
    lm = model.language_model
    got = lm.generate_rolling(feats[:5].to(DEV), 6).cpu()          # rows=None: min(S, what fits) = 5
    assert torch.equal(got, _oracle_ids(oracle, 5, 6)[0])


def test_refusals(model, feats):
    lm = model.language_model
    f = feats[:6].to(DEV)
    with pytest.raises(ValueError, match="max_length"):
        lm.generate_rolling(f, None)
    with pytest.raises(ValueError, match="max_length"):
        lm.generate_rolling(f, 1)
    with pytest.raises(ValueError, match="rows"):
        lm.generate_rolling(f, 6, rows=0)
    with pytest.raises(ValueError, match="rows"):
        model.generate_rolling(synth.make_images(1, 1234).to(DEV), 6, rows=-2)     # before the detector runs
    with pytest.raises(_hip.RgrgHipError, match="no CPU fallback"):
        lm.generate_rolling(feats[:6], 6)
    with pytest.raises(_hip.RgrgHipError, match="rows"):
        lm.generate_rolling(f, 6, rows=10 ** 6)                                       # more rows than any cache holds
    # the C entry's own bounds: rows above the decoder's cache, max_length above its slots
    eng = model.engine()
    lm.generate_rolling(f, 6, rows=4)
    dec, (cap_s, cap_l) = eng._decoder, eng._decoder_caps
    out = torch.empty((6, 6), dtype=torch.int64, device=DEV)
    lens = torch.empty((6,), dtype=torch.int32, device=DEV)
    lib = _hip.load()
    assert lib.rgrg_decoder_generate_rolling(dec, f.data_ptr(), 6, cap_s + 1, 6, out.data_ptr(), lens.data_ptr(), None, 1, None) != 0
    assert b"decoder rows" in lib.rgrg_last_error()
    assert lib.rgrg_decoder_generate_rolling(dec, f.data_ptr(), 6, 0, 6, out.data_ptr(), lens.data_ptr(), None, 1, None) != 0
    assert lib.rgrg_decoder_generate_rolling(dec, f.data_ptr(), 6, 4, cap_l + 1, out.data_ptr(), lens.data_ptr(), None, 1, None) != 0
    assert lib.rgrg_decoder_generate_rolling(dec, f.data_ptr(), 6, 4, 1, out.data_ptr(), lens.data_ptr(), None, 1, None) != 0
    # the e4m3 cache where it would be used (16-bit mode, more rows than the fused plan takes): refused, naming the format
    lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with pytest.raises(_hip.RgrgHipError, match="e4m3"):
                lm.generate_rolling(feats[:80].to(DEV), 6, rows=70)
            assert lm.generate_rolling(f, 6, rows=4).shape[0] == 6      # 4 rows keep an fp32 cache: the setting has no effect there
    finally:
        lm.set_kv_cache_dtype(None)
    assert torch.equal(lm.generate_rolling(f, 6, rows=4), lm.generate(f, 6))   # still works afterwards


def test_report_model_generate_rolling_equals_generate():
    import rgrg_amd
    m = gpu_model("ragged")
    images = synth.make_images(2, 1234).to(DEV)
    ref = m.generate(images, 8)
    got = m.generate_rolling(images, 8, rows=16)
    assert not isinstance(ref, int) and len(got) == 4
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[3])
    assert sorted(got[2]) == sorted(ref[2]) and all(torch.equal(got[2][k], ref[2][k]) for k in ref[2])
    print(f"ROLLING report model: {ref[0].shape[0]} selected regions through 16 rows")
    # nothing selected: the -1 of generate()
    sd0 = dict(synth_sd("ragged"))
    sd0["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m0 = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m0.load_state_dict(sd0)
    m0.to(DEV).eval()
    try:
        assert m0.generate_rolling(images[:1], 6, rows=4) == -1
    finally:
        m0.invalidate_engine()
