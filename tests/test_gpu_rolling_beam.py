"""Rolling-batch beam search end to end on the MI355X (rgrg_decoder_beam_search_rolling; LanguageModel.beam_search_rolling,
Engine.beam_search_rolling, ReportGenerationModel.generate_rolling_beam): S regions through rows // num_beams slots of beam rows give
the ids of ``generate(num_beams=..)`` - the same padded width, the same order -, graph and eager, and the refusals.

Weights and feature rows are those of tests/test_gpu_rolling.py (the ``ragged`` profile with ``prompt_reference.eos_boosted(sd,
0.98)``; ROWS of ``torch.randn((400, 1024), seed 777)``); tests/test_rolling_beam_reference.py shows on the CPU that every prefix used
here has regions that leave at three or more distinct iterations, one that runs to max_length and one that is done within 3.

fp32 equality holds between calls that sit on the SAME step plan - the fused plan up to 128 token rows, the tiled plan above: the two
plans round differently and a beam may flip between them.  So every case compares rolling on R rows against lock step on S * 4 rows
with both numbers on one side of 128.  The lock-step result is first compared with the CPU oracle, as a precondition on the inputs:
a failure there names the inputs, not the rolling loop."""
import pytest
import torch

import prompt_reference as pr
import rolling_beam_reference as M
from conftest import gpu_model, synth_sd
from oracle import language_model as o_lm
from rgrg_amd import _hip, synth
from test_gpu_rolling import BOOST, POOL, POOL_SEED, ROWS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = 50256
NB, L_MAX = 4, 12


def _sd():
    return pr.eos_boosted(synth_sd("ragged"), BOOST)


@pytest.fixture(scope="module")
def feats():
    return torch.randn((POOL, 1024), generator=torch.Generator().manual_seed(POOL_SEED))[ROWS].contiguous()


@pytest.fixture(scope="module")
def model():
    import rgrg_amd
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.load_state_dict(_sd())
    m.to(DEV).eval()
    yield m
    m.invalidate_engine()


_ORACLE = {}


def _oracle(feats, S, nb, early, keep=1):
    """``beam_generate`` on the CPU for the first S rows with its trace, once per setting."""
    key = (S, nb, early, keep)
    if key not in _ORACLE:
        _ORACLE[key] = o_lm.beam_generate(_sd(), feats[:S], L_MAX, nb, early_stopping=early, num_return_sequences=keep, return_trace=True)
    return _ORACLE[key]


def _check_case(model, feats, S, R, nb, early, keep=1):
    lm, eng = model.language_model, model.engine()
    f = feats[:S].to(DEV)
    want, trace = _oracle(feats, S, nb, early, keep)
    lock = lm.generate(f, L_MAX, num_beams=nb, early_stopping=early, num_return_sequences=keep).cpu()
    assert torch.equal(lock, want), ("precondition: lock step differs from the oracle on these inputs", lock.tolist(), want.tolist())
    got = lm.beam_search_rolling(f, L_MAX, nb, rows=R, early_stopping=early, num_return_sequences=keep).cpu()
    steps = eng.last_rolling_steps
    G = min(R // nb, S)
    assert eng.fused_row_limit() == 128 and eng.kv_format_in_use(G * nb) == 0
    assert (G * nb <= 128) == (S * nb <= 128), "the two sides sit on different step plans"
    assert got.dtype == torch.int64 and got.shape == lock.shape and torch.equal(got, lock), (got.tolist(), lock.tolist())
    ref = M.schedule(trace, S, nb, G, L_MAX, early, keep=keep)
    _, iters = M.lockstep_inputs(trace, S, nb, L_MAX, early)
    work, longest = sum(iters), max(iters)
    print(f"ROLLBEAM S={S} R={R} nb={nb} early={early} steps {steps} lock-step {longest} work/G {work / G:.1f} bound {M.bound(S, G, L_MAX)}")
    assert max(longest, -(-work // G)) <= steps <= M.bound(S, G, L_MAX)
    assert steps == ref["steps"], "the schedule is a function of the tokens: the model's step count"
    if S <= R // nb:
        assert steps == longest
    again = lm.beam_search_rolling(f, L_MAX, nb, rows=R, early_stopping=early, num_return_sequences=keep).cpu()
    assert torch.equal(again, got) and eng.last_rolling_steps == steps
    return got


@pytest.mark.parametrize("early", (True, False))
@pytest.mark.parametrize("S,R", [(11, 8), (11, 4), (20, 12), (40, 132), (5, 32)])
def test_rolling_equals_generate_and_the_oracle_fp32(model, feats, S, R, early):
    """2 slots; 1 slot (every region through it); 3 slots; 33 slots = 132 rows against the 160-row lock step, both on the tiled
    plan; S <= G (5 regions in 8 slots: no slot is ever refilled, the steps are the longest region's)."""
    _check_case(model, feats, S, R, NB, early)


def test_num_return_sequences_equal_to_num_beams(model, feats):
    got = _check_case(model, feats, 11, 8, NB, True, keep=NB)
    assert got.shape[0] == 11 * NB


def test_17_beams_take_the_wide_ranking(model, feats):
    """More than 16 beams: the K-round ranking kernels on 34-wide candidate rows; 3 regions through one slot of 17 rows."""
    _check_case(model, feats, 3, 17, 17, True)


def test_graph_equals_eager_and_partial_slots(model, feats):
    eng = model.engine()
    f = feats[:11].to(DEV)
    a = eng.beam_search_rolling(f, L_MAX, NB, 8, True, use_graph=True)
    steps = eng.last_rolling_steps
    b = eng.beam_search_rolling(f, L_MAX, NB, 8, True, use_graph=False)
    assert torch.equal(a, b) and eng.last_rolling_steps == steps
    # rows that are no multiple of num_beams: rows // num_beams slots
    c = eng.beam_search_rolling(f, L_MAX, NB, 11, True)
    assert torch.equal(a, c) and eng.last_rolling_steps == steps
    # rows=None: min(S, what fits // num_beams) slots - all regions seated at once
    d = model.language_model.beam_search_rolling(f[:5], L_MAX, NB, early_stopping=True)
    assert torch.equal(d, model.language_model.generate(f[:5], L_MAX, num_beams=NB, early_stopping=True))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        f = feats[:40].to(DEV)
        g = eng.beam_search_rolling(f, 8, NB, 80, True, use_graph=True, bf16=1)
        h = eng.beam_search_rolling(f, 8, NB, 80, True, use_graph=False, bf16=1)
    assert torch.equal(g, h)


_FP32_ROLLING = {}


@pytest.mark.parametrize("dtype,S,R", [(torch.float16, 10, 40), (torch.bfloat16, 40, 80), (torch.float16, 40, 80)])
def test_16bit_plans(model, feats, dtype, S, R):
    """10 regions through 40 rows under fp16: the fused plan on 16-bit weights, fp32 cache.  40 regions through 80 rows under bf16 /
    fp16: the 16-bit cache, and with it attn_decode_kv16_wave_kernel<true, .., ROWSTEP>.  Against the fp32 rolling beams of the same
    inputs, over the generated columns: the thresholds tests/test_gpu_group_beam.py::test_16bit_plans takes from
    tests/test_gpu_parity_gaps.py (16-bit beams against fp32 beams)."""
    lm, eng = model.language_model, model.engine()
    f = feats[:S].to(DEV)
    if (S, R) not in _FP32_ROLLING:
        _FP32_ROLLING[(S, R)] = lm.beam_search_rolling(f, L_MAX, NB, rows=R, early_stopping=True).cpu()
    a = _FP32_ROLLING[(S, R)]
    with torch.autocast("cuda", dtype=dtype):
        b = lm.beam_search_rolling(f, L_MAX, NB, rows=R, early_stopping=True).cpu()
        again = lm.beam_search_rolling(f, L_MAX, NB, rows=R, early_stopping=True).cpu()
        assert eng.fused_row_limit() == 64
        assert eng.kv_format_in_use(R) == (0 if R <= 64 else (2 if dtype == torch.float16 else 1))
    assert torch.equal(b, again)
    assert b.dtype == torch.int64 and b.shape[0] == S and (b[:, 0] == EOS).all()
    Lc = min(a.shape[1], b.shape[1])
    same = a[:, 1:Lc] == b[:, 1:Lc]
    tok, seq = same.float().mean().item(), same.all(1).float().mean().item()
    print(f"ROLLBEAM16 dtype={dtype} rows={R} steps {eng.last_rolling_steps} tokens equal to the fp32 rolling beams {tok:.4f} sequences {seq:.4f}")
    assert tok >= 0.85 and seq >= 0.75, (tok, seq)


def test_refusals(model, feats):
    lm = model.language_model
    f = feats[:6].to(DEV)
    with pytest.raises(ValueError, match="max_length"):
        lm.beam_search_rolling(f, None, NB)
    with pytest.raises(ValueError, match="max_length"):
        lm.beam_search_rolling(f, 1, NB)
    with pytest.raises(ValueError, match="rows"):
        lm.beam_search_rolling(f, 6, NB, rows=0)
    with pytest.raises(ValueError, match="rows"):
        lm.beam_search_rolling(f, 6, NB, rows=NB - 1)
    with pytest.raises(ValueError, match="num_beams"):
        lm.beam_search_rolling(f, 6, 1)
    with pytest.raises(ValueError, match="num_return_sequences"):
        lm.beam_search_rolling(f, 6, NB, num_return_sequences=NB + 1)
    with pytest.raises(ValueError, match="rows"):
        model.generate_rolling_beam(synth.make_images(1, 1234).to(DEV), 6, NB, rows=-2)     # before the detector runs
    with pytest.raises(_hip.RgrgHipError, match="no CPU fallback"):
        lm.beam_search_rolling(feats[:6], 6, NB)
    with pytest.raises(_hip.RgrgHipError, match="rows"):
        lm.beam_search_rolling(f, 6, NB, rows=10 ** 6)                                       # more rows than any cache holds
    # what generate() refuses stays refused
    with pytest.raises(NotImplementedError):
        lm.generate(f, 6, num_beams=NB, do_sample=True)
    # the C entry's own bounds: rows above the decoder's cache and below one slot, max_length above its slots
    eng = model.engine()
    lm.beam_search_rolling(f, 6, NB, rows=8)
    dec, (cap_s, cap_l) = eng._decoder, eng._decoder_caps
    out = torch.empty((6, 6), dtype=torch.int64, device=DEV)
    lib = _hip.load()
    import ctypes as C
    n, steps = C.c_int(0), C.c_int(0)

    def call(R, L):
        return lib.rgrg_decoder_beam_search_rolling(dec, f.data_ptr(), 6, NB, R, L, 1, 1.0, 1, out.data_ptr(), 6, C.byref(n), C.byref(steps), 1, None)
    assert call(cap_s + 1, 6) != 0
    assert b"decoder rows" in lib.rgrg_last_error()
    assert call(NB - 1, 6) != 0
    assert b"decoder rows" in lib.rgrg_last_error()
    assert call(8, cap_l + 1) != 0
    assert b"max_length" in lib.rgrg_last_error()
    assert call(8, 1) != 0
    assert call(8, 6) == 0 and n.value >= 2 and steps.value >= 5
    # the e4m3 cache where it would be used (16-bit mode, more rows than the fused plan takes): refused, naming the format
    lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with pytest.raises(_hip.RgrgHipError, match="e4m3"):
                lm.beam_search_rolling(feats[:40].to(DEV), 6, NB, rows=80)
            assert lm.beam_search_rolling(f, 6, NB, rows=8).shape[0] == 6      # 8 rows keep an fp32 cache: the setting has no effect there
    finally:
        lm.set_kv_cache_dtype(None)
    assert torch.equal(lm.beam_search_rolling(f, 6, NB, rows=8), lm.generate(f, 6, num_beams=NB))   # still works afterwards


def test_report_model_generate_rolling_beam_equals_generate():
    import rgrg_amd
    m = gpu_model("ragged")
    images = synth.make_images(2, 1234).to(DEV)
    ref = m.generate(images, 8, num_beams=NB, early_stopping=True)
    got = m.generate_rolling_beam(images, 8, NB, rows=16, early_stopping=True)
    assert not isinstance(ref, int) and len(got) == 4
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[3])
    assert sorted(got[2]) == sorted(ref[2]) and all(torch.equal(got[2][k], ref[2][k]) for k in ref[2])
    print(f"ROLLBEAM report model: {ref[0].shape[0]} selected regions through 16 rows")
    # nothing selected: the -1 of generate()
    sd0 = dict(synth_sd("ragged"))
    sd0["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m0 = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m0.load_state_dict(sd0)
    m0.to(DEV).eval()
    try:
        assert m0.generate_rolling_beam(images[:1], 6, NB, rows=8) == -1
    finally:
        m0.invalidate_engine()
