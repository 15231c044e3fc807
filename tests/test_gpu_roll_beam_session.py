"""Rolling beam sessions end to end on the MI355X (rgrg_decoder_beam_roll_*; LanguageModel.open_rolling(num_beams=..),
HipEngine.open_rolling(beam=..), ReportGenerationModel.open_rolling(num_beams=..)): regions that join a beam search that is running
get the hypotheses ``generate(num_beams=..)`` gives them, under every arrival schedule tried; the host's counts - steps launched,
unfinished, steps, delivered regions, watermark - are those of the host model (tests/rolling_beam_session_reference.py) driven by
the same calls.

Weights, feature rows, the oracle runs and the 16-bit thresholds are those of tests/test_gpu_rolling_beam.py (imported, not copied),
and so is its rule for fp32 equality: both sides of a comparison sit on ONE step plan (the fused plan up to 128 token rows)."""
import ctypes as C

import pytest
import torch

import rolling_beam_session_reference as B
import test_gpu_rolling_beam as TB
from conftest import gpu_model, synth_sd
from test_gpu_rolling_beam import feats, model  # noqa: F401  (fixtures)
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = PAD = 50256
NB, L_MAX = TB.NB, TB.L_MAX
assert (NB, L_MAX) == (4, 12)


def _drive(ses, f, ops, mdl=None):
    """Runs ops (rolling_beam_session_reference.play's) on the session - and on the host model, comparing every count the host
    reports and every delivered region - then drains and collects -> {q: ids [num_return_sequences, L_q] on the CPU}."""
    got, fed = {}, 0
    for op in list(ops) + [("advance", None), ("collect",)]:
        if op[0] == "submit":
            r = ses.submit(f[fed:fed + op[1]])
            assert r == range(fed, fed + op[1]) and (mdl is None or r == mdl.submit(op[1]))
            fed += op[1]
        elif op[0] == "refused":
            before = (ses.submitted, ses.unfinished, ses.watermark, ses.steps)
            with pytest.raises(_hip.RgrgHipError, match=f"capacity {ses.capacity} regions") as e:
                ses.submit(f[:op[1]])             # (any rows: nothing is read)
            assert "room for" in str(e.value) and (ses.submitted, ses.unfinished, ses.watermark, ses.steps) == before
            if mdl is not None:
                with pytest.raises(B.RingFull):
                    mdl.submit(op[1])
        elif op[0] == "advance":
            launched = ses.advance(op[1])
            if mdl is not None:
                assert (launched, ses.unfinished, ses.steps) == (mdl.advance(op[1]), mdl.unfinished, mdl.steps), op
        else:
            items = ses.collect()
            if mdl is not None:
                assert [q for q, _ in items] == mdl.collect() and ses.watermark == mdl.watermark
            for q, ids in items:
                assert q not in got and ids.dtype == torch.int64 and ids.shape[0] == ses.num_return_sequences
                got[q] = ids.cpu()
                assert mdl is None or torch.equal(got[q], mdl.result[q]), (q, got[q].tolist(), mdl.result[q].tolist())
            assert [q for q, _ in items] == sorted(q for q, _ in items)
    assert ses.unfinished == 0 and ses.watermark == ses.submitted == fed and sorted(got) == list(range(fed))
    return got


def _rows_of(ref, got, keep=1):
    """Every delivered region against its rows of a one-call result ``ref`` [S * keep, L]: PAD behind the region's own width."""
    assert torch.equal(B.table(got, sorted(got), keep, pad_to=ref.shape[1]), ref), (B.table(got, sorted(got), keep).tolist(), ref.tolist())
    assert max(v.shape[1] for v in got.values()) == ref.shape[1]


def _mdl(feats, S, case, early=True, keep=1):  # noqa: F811
    R, nb, cap, L, ops = case
    want, trace = TB._oracle(feats, S, nb, early, keep)
    return B.Session(trace, nb, R, cap, L, early, keep=keep), want


def test_case_1_joins_wraps_and_refusals_fp32(model, feats):  # noqa: F811
    """rows = 8 (2 slots of 4 beams), capacity 3, L = 12, 7 regions in submits of 1, 3 and 3 (CASE_1 of the host model): a region
    alone next to an idle slot, regions left mid-flight between advances, a ring that wraps twice - once inside a submit -, three
    ring-full refusals that leave the session intact, out-of-order delivery behind an unfinished region."""
    lm, eng = model.language_model, model.engine()
    R, nb, cap, L, ops = B.CASE_1
    f = feats[:7].to(DEV)
    lock = lm.generate(f, L, num_beams=nb, early_stopping=True).cpu()
    mdl, want = _mdl(feats, 7, B.CASE_1)
    assert torch.equal(lock, want), "precondition: lock step differs from the oracle on these inputs"
    with lm.open_rolling(L, rows=R, capacity=cap, num_beams=nb, early_stopping=True) as ses:
        assert eng.fused_row_limit() == 128 and eng.kv_format_in_use(R) == 0 and ses.slots == 2 and ses.capacity == 3
        got = _drive(ses, f, ops, mdl)
        assert ses.steps == 38
    _rows_of(lock, got)
    assert len(set(v.shape[1] for v in got.values())) >= 2, "the regions differ in length"


def _all_at_once(lm, eng, f, L, R, nb):
    one = lm.beam_search_rolling(f, L, nb, rows=R, early_stopping=True).cpu()
    steps = eng.last_rolling_steps
    with lm.open_rolling(L, rows=R, capacity=f.shape[0], num_beams=nb, early_stopping=True) as ses:
        got = _drive(ses, f, [("submit", f.shape[0])])
        assert ses.steps == steps
    _rows_of(one, got)
    return one


def test_all_regions_before_the_first_step_is_beam_search_rolling(model, feats):  # noqa: F811
    """The same schedule on the same plan, so the same bits: ids and step count of ``beam_search_rolling``.  fp32 on 2 slots; bf16 and
    fp16 on 17 slots of 4 = 68 rows (the many-sequence step on the 16-bit cache), 40 regions, L = 9 - and those against fp32
    ``generate`` over the generated columns under the thresholds of tests/test_gpu_rolling_beam.py::test_16bit_plans."""
    lm, eng = model.language_model, model.engine()
    _all_at_once(lm, eng, feats[:11].to(DEV), L_MAX, 8, NB)
    f = feats[:40].to(DEV)
    a = lm.generate(f, 9, num_beams=NB, early_stopping=True).cpu()
    for dtype in (torch.bfloat16, torch.float16):
        with torch.autocast("cuda", dtype=dtype):
            b = _all_at_once(lm, eng, f, 9, 68, NB)
            assert eng.fused_row_limit() == 64 and eng.kv_format_in_use(68) == (2 if dtype == torch.float16 else 1)
        assert b.shape[0] == 40 and (b[:, 0] == EOS).all()
        Lc = min(a.shape[1], b.shape[1])
        same = a[:, 1:Lc] == b[:, 1:Lc]
        tok, seq = same.float().mean().item(), same.all(1).float().mean().item()
        print(f"BEAMSESSION16 dtype={dtype} rows=68 tokens equal to the fp32 beams {tok:.4f} sequences {seq:.4f}")
        assert tok >= 0.85 and seq >= 0.75, (tok, seq)


# 2 + 1 + 1 regions fill the ring of 4 whatever their lengths; the last 3 wrap it after a drain
STREAM = (("submit", 2), ("advance", 2), ("collect",), ("submit", 1), ("advance", 3), ("collect",), ("submit", 1), ("advance", 1),
          ("refused", 1), ("advance", None), ("collect",), ("submit", 3), ("advance", 2), ("collect",))


@pytest.mark.parametrize("early,lp,keep", [(True, 1.0, NB), (False, 1.0, 1), (True, 0.6, 1), (False, 1.7, 2)])
def test_options_against_beam_search(model, feats, early, lp, keep):  # noqa: F811
    """num_return_sequences = num_beams, early stopping both ways, length_penalty != 1: 7 regions arriving in four submits through 2
    slots and a ring of 4, against ``beam_search`` on the same arguments."""
    lm, eng = model.language_model, model.engine()
    f = feats[:7].to(DEV)
    ref = eng.beam_search(f, L_MAX, NB, early, lp, num_return_sequences=keep).cpu()
    if lp == 1.0:
        want, trace = TB._oracle(feats, 7, NB, early, keep)
        assert torch.equal(ref, want), "precondition: lock step differs from the oracle on these inputs"
        mdl = B.Session(trace, NB, 8, 4, L_MAX, early, keep=keep)
    else:
        mdl = None
    with lm.open_rolling(L_MAX, rows=8, capacity=4, num_beams=NB, early_stopping=early, length_penalty=lp, num_return_sequences=keep) as ses:
        got = _drive(ses, f, STREAM, mdl)
    _rows_of(ref, got, keep)


def test_17_beams_take_the_wide_ranking(model, feats):  # noqa: F811
    """More than 16 beams: one slot of 17 rows, 3 regions through a ring of 2, the third joining while the second runs."""
    lm = model.language_model
    f = feats[:3].to(DEV)
    lock = lm.generate(f, L_MAX, num_beams=17, early_stopping=True).cpu()
    want, trace = TB._oracle(feats, 3, 17, True)
    assert torch.equal(lock, want), "precondition: lock step differs from the oracle on these inputs"
    ops = (("submit", 2), ("refused", 1), ("advance", 4), ("collect",), ("advance", None), ("collect",), ("submit", 1), ("advance", 2))
    with lm.open_rolling(L_MAX, rows=17, capacity=2, num_beams=17, early_stopping=True) as ses:
        got = _drive(ses, f, ops, B.Session(trace, 17, 17, 2, L_MAX, True))
    _rows_of(lock, got)


def test_idle_and_reuse(model, feats):  # noqa: F811
    lm = model.language_model
    f = feats[:4].to(DEV)
    lock = lm.generate(f, L_MAX, num_beams=NB, early_stopping=True).cpu()
    R, nb, cap, L, ops = B.IDLE_AND_REUSE
    with lm.open_rolling(L, rows=R, capacity=cap, num_beams=nb, early_stopping=True) as ses:
        assert ses.advance() == 0 and ses.advance(3) == 0 and ses.collect() == [] and ses.steps == 0   # nothing was ever submitted
        ses.submit(f[:1])
        assert ses.advance() > 0 and ses.unfinished == 0
        steps = ses.steps
        assert ses.advance() == 0 and ses.advance(5) == 0 and ses.steps == steps                      # drained: nothing is launched
        got = {q: ids.cpu() for q, ids in ses.collect()}
        ses.submit(f[1:4])                                                                            # slot 1 has idled since the open
        assert ses.unfinished == 3 and ses.advance() > 0 and ses.steps > steps
        got.update({q: ids.cpu() for q, ids in ses.collect()})
    _rows_of(lock, got)
    with lm.open_rolling(L, rows=R, capacity=cap, num_beams=nb, early_stopping=True) as ses:          # the model's counts for such calls
        _rows_of(lock, _drive(ses, f, ops, _mdl(feats, 7, B.IDLE_AND_REUSE)[0]))


def test_graph_equals_eager(model, feats):  # noqa: F811
    eng = model.engine()
    R, nb, cap, L, ops = B.CASE_1
    f = feats[:7].to(DEV)
    outs = []
    for use_graph in (True, False):
        with eng.open_rolling(L, R, cap, beam=dict(num_beams=nb, early_stopping=True), use_graph=use_graph) as ses:
            outs.append(_drive(ses, f, ops, _mdl(feats, 7, B.CASE_1)[0]))
    assert all(torch.equal(outs[0][q], outs[1][q]) for q in range(7))


def test_staleness_and_refusals(model, feats):  # noqa: F811
    lm = model.language_model
    f = feats[:7].to(DEV)
    ref = lm.generate(f, 6, num_beams=NB)
    with pytest.raises(ValueError, match="do_sample"):
        lm.open_rolling(6, rows=8, num_beams=NB, do_sample=True)
    for bad in (dict(rows=NB - 1), dict(rows=None), dict(rows=8, capacity=0), dict(rows=8, num_return_sequences=NB + 1)):
        with pytest.raises(ValueError):
            lm.open_rolling(6, num_beams=NB, **bad)
    with pytest.raises(ValueError, match="max_length"):
        lm.open_rolling(None, rows=8, num_beams=NB)
    ses = lm.open_rolling(6, rows=10, num_beams=NB)
    assert ses.slots == 2 and ses.capacity == 8                  # None: 4 * (rows // num_beams) regions
    for kind in (dict(num_beams=NB), dict()):                    # a second session of either kind
        with pytest.raises(ValueError, match="already open"):
            lm.open_rolling(6, rows=8, **kind)
    eng, lib = model.engine(), _hip.load()
    assert lib.rgrg_decoder_roll_open(eng._decoder, 4, 4, 1, 6, 0, 1.0, 0, 1.0, 0, 1, None) != 0 and b"beam session is already open" in lib.rgrg_last_error()
    assert lib.rgrg_decoder_beam_roll_open(eng._decoder, 8, NB, 4, 6, 0, 1.0, 1, 1, None) != 0 and b"already open" in lib.rgrg_last_error()
    assert lib.rgrg_decoder_beam_roll_open(eng._decoder, 8, NB, 0, 6, 0, 1.0, 1, 1, None) != 0 and b"at least 1" in lib.rgrg_last_error()
    assert lib.rgrg_decoder_beam_roll_open(eng._decoder, NB - 1, NB, 4, 6, 0, 1.0, 1, 1, None) != 0 and b"decoder rows" in lib.rgrg_last_error()
    ses.submit(f[:3])
    ses.advance(1)
    # collect of an unfinished region and release past one, on the C entries (the Python surface never asks for either)
    out, width, fin = torch.empty((1, 6), dtype=torch.int64, device=DEV), C.c_int(0), (C.c_int * 3)()
    assert lib.rgrg_decoder_beam_roll_collect(eng._decoder, 0, 3, None, 0, None, fin, None) == 0 and list(fin) == [0, 0, 0]
    assert lib.rgrg_decoder_beam_roll_collect(eng._decoder, 0, 1, out.data_ptr(), 6, C.byref(width), None, None) != 0
    assert b"has not finished" in lib.rgrg_last_error()
    assert lib.rgrg_decoder_beam_roll_collect(eng._decoder, 2, 2, None, 0, None, fin, None) != 0 and b"the session holds" in lib.rgrg_last_error()
    assert lib.rgrg_decoder_beam_roll_release(eng._decoder, 1) != 0 and b"has not finished" in lib.rgrg_last_error()
    assert lib.rgrg_decoder_beam_roll_release(eng._decoder, 4) != 0 and lib.rgrg_decoder_beam_roll_release(eng._decoder, 0) == 0
    assert ses.advance(1) == 1 and ses.steps == 2                # ... and the session is intact
    assert torch.equal(lm.generate(f, 6, num_beams=NB), ref)    # another decode entry works as without a session ...
    for call in (lambda: ses.advance(), lambda: ses.submit(f[3:4]), lambda: ses.collect()):
        with pytest.raises(_hip.RgrgHipError, match="stale"):    # ... and the session has lost its rows
            call()
    ses.close()
    ses.close()
    with pytest.raises(_hip.RgrgHipError, match="closed"):
        ses.submit(f[:1])
    with lm.open_rolling(6, rows=8, num_beams=NB) as again:     # a new session opens afterwards
        _rows_of(ref.cpu(), _drive(again, f, [("submit", 7)]))
    with lm.open_rolling(6, rows=4) as greedy:                   # ... and a greedy one blocks a beam session
        with pytest.raises(ValueError, match="already open"):
            lm.open_rolling(6, rows=8, num_beams=NB)
        assert lib.rgrg_decoder_beam_roll_open(eng._decoder, 8, NB, 4, 6, 0, 1.0, 1, 1, None) != 0 and b"already open" in lib.rgrg_last_error()
        assert greedy.advance() == 0


def test_e4m3_cache_is_refused_with_the_words_of_roll_check(model, feats):  # noqa: F811
    """16-bit mode and more rows than the fused plan takes: the e4m3 cache would be used, and open refuses it as every rolling entry
    does; 8 rows keep an fp32 cache, where the setting has no effect."""
    lm = model.language_model
    lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with pytest.raises(_hip.RgrgHipError, match="the e4m3 K/V cache has no per-row step: call rgrg_decoder_set_kv_format") as e:
                lm.open_rolling(6, rows=80, num_beams=NB)
            assert "rgrg_decoder_beam_roll_open" in str(e.value)
            with lm.open_rolling(6, rows=8, num_beams=NB) as small:
                assert small.advance() == 0
    finally:
        lm.set_kv_cache_dtype(None)


def _same_result(got, ref):
    assert not isinstance(ref, int) and len(got) == 4
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[3])
    assert sorted(got[2]) == sorted(ref[2]) and all(torch.equal(got[2][k], ref[2][k]) for k in ref[2])


def test_report_model_open_rolling_with_beams():
    import rgrg_amd
    m = gpu_model("ragged")
    images = synth.make_images(3, 1234).to(DEV)
    kw = dict(num_beams=NB, early_stopping=True, num_return_sequences=2)
    ref_a = m.generate(images[:2], 8, **kw)
    ref_b = m.generate(images[2:], 8, **kw)
    with m.open_rolling(8, rows=16, capacity=96, **kw) as ses:
        a = ses.submit(images[:2])
        assert ses.advance(3) == 3
        first = ses.collect()
        b = ses.submit(images[2:])                               # joins while the first ticket's regions are half done
        ses.advance()
        done = dict(first + ses.collect())
        assert ses.unfinished == 0 and ses.collect() == []
    assert (a, b) == (0, 1) and sorted(done) == [0, 1]
    _same_result(done[a], ref_a)
    _same_result(done[b], ref_b)
    print(f"BEAMSESSION report model: {ref_a[1].sum().item()} + {ref_b[1].sum().item()} selected regions through 4 slots")
    sd0 = dict(synth_sd("ragged"))
    sd0["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m0 = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m0.load_state_dict(sd0)
    m0.to(DEV).eval()
    try:
        with m0.open_rolling(6, rows=8, num_beams=NB) as ses:
            t = ses.submit(images[:1])
            assert t == 0 and ses.collect() == [(t, -1)] and ses.unfinished == 0 and ses.advance() == 0
    finally:
        m0.invalidate_engine()
