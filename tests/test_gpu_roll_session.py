"""Rolling sessions end to end on the MI355X (rgrg_decoder_roll_*; LanguageModel.open_rolling, HipEngine.open_rolling,
ReportGenerationModel.open_rolling): sentences that join a decode that is running get the tokens ``generate()`` gives them, under
every arrival schedule tried; the host's counts - steps launched, unfinished, finished sets, watermark - are those of the numpy
model (tests/rolling_session_reference.py) driven by the same calls.

Weights, feature rows and the 16-bit rule are those of tests/test_gpu_rolling.py (imported, not copied): only prefixes of at least 9
rows and max_length in {6, 8, 9, 12} are used, so that file's conditions hold - re-asserted here on this module's oracle run: the
smallest top-2 gap of an unfinished row is 10 x the 2e-3 logit tolerance, so in fp32 the reference alone decides every token."""
import pytest
import torch

import rolling_session_reference as S
import test_gpu_rolling as TR
from conftest import gpu_model, synth_sd
from test_gpu_rolling import feats, model, oracle  # noqa: F401  (fixtures)
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = PAD = 50256
assert (TR.BOOST, TR.POOL, TR.POOL_SEED, TR.L_MAX, len(TR.ROWS)) == (0.98, 400, 777, 12, 150)


def test_feature_rows_keep_their_gap(oracle):  # noqa: F811
    gap = oracle["logits"].topk(2, dim=-1).values
    gap = gap[..., 0] - gap[..., 1]
    live = torch.arange(TR.L_MAX - 1)[None, :] < (oracle["lens"] - 1)[:, None]
    print(f"SESSION smallest top-2 gap of an unfinished row {gap[live].min().item():.4f}")
    assert gap[live].min().item() >= 10 * TR.TOL_LOGIT
    assert TR._oracle_ids(oracle, 11, 12)[1].tolist() == S.LENGTHS_12


def _lengths(ids, L):
    """Natural lengths of the rows of a generate() result at max_length L (BOS and EOS included; L + 1: cut without an EOS)."""
    out = []
    for row in ids[:, 1:].tolist():
        out.append(row.index(EOS) + 2 if EOS in row else L + 1)
    return out


def _drive(ses, f, ops, lengths=None):
    """Runs ops (rolling_session_reference.play's) on the session - and, given the sentences' lengths, on the numpy model, comparing
    every count the host reports - then drains and collects -> {q: (ids[, logprobs])}."""
    R, C, n, L = ses.rows, ses.capacity * ses.n, ses.n, ses.max_length
    mdl = S.Session(lengths, R, C, n, L) if lengths is not None else None
    got, fed = {}, 0

    def submit(m):
        nonlocal fed
        r = ses.submit(f[fed:fed + m])
        assert r == range(fed * n, (fed + m) * n) and (mdl is None or r == mdl.submit(m))
        fed += m

    def advance(k):
        launched = ses.advance(k)
        if mdl is not None:
            assert launched == mdl.advance(k) and ses.unfinished == mdl.unfinished and ses.steps == mdl.device_steps
        return launched

    def collect():
        items = ses.collect()
        if mdl is not None:
            assert [it[0] for it in items] == mdl.collect() and ses.watermark == mdl.watermark
        assert [it[0] for it in items] == sorted(it[0] for it in items)
        for it in items:
            assert it[0] not in got
            got[it[0]] = it[1:]
        return items

    for op in list(ops) + [("advance", None), ("collect",)]:
        if op[0] == "submit":
            submit(op[1])
        elif op[0] == "refused":
            before = (ses.submitted, ses.unfinished, ses.watermark)
            with pytest.raises(_hip.RgrgHipError, match=f"capacity {ses.capacity} feature rows") as e:
                ses.submit(f[fed:fed + op[1]])
            assert "room for" in str(e.value) and (ses.submitted, ses.unfinished, ses.watermark) == before
            if mdl is not None:
                with pytest.raises(S.RingFull):
                    mdl.submit(op[1])
        elif op[0] == "advance":
            advance(op[1])
        elif op[0] == "stream":
            while ses.submitted < op[1] * n:
                m = min(op[2], op[1] - fed, (ses.watermark + C - ses.submitted) // n)
                if m > 0:
                    submit(m)
                advance(op[3])
                collect()
        else:
            collect()
    assert ses.unfinished == 0 and ses.watermark == ses.submitted == fed * n and sorted(got) == list(range(fed * n))
    return got


def _table(got, total, col=0):
    """The collected sentences as generate() returns them: [total, longest], PAD (log-probs: 0) behind a sentence's end."""
    width = max(got[q][0].shape[0] for q in range(total))
    fill = PAD if col == 0 else 0
    out = torch.full((total, width), fill, dtype=got[0][col].dtype)
    for q in range(total):
        out[q, :got[q][col].shape[0]] = got[q][col].cpu()
    return out


def _ops(name):
    return [c for c in S.schedule_cases() if c[0] == name][0][6]


def test_case_1_join_refuse_wrap_fp32(model, feats, oracle):  # noqa: F811
    """R = 4, C = 6, L = 12, the first 11 rows: submit 5; 3 more refused; two steps, after which exactly 1 and 2 have ended; 2 more
    refused (the watermark is still 0: 0 is running); 1 goes to the idle row; drain (watermark 6); the remaining 5 wrap; drain."""
    lm = model.language_model
    f = feats[:11].to(DEV)
    ref = lm.generate(f, 12).cpu()
    want, lens = TR._oracle_ids(oracle, 11, 12)
    with lm.open_rolling(12, rows=4, capacity=6) as ses:
        assert model.engine().kv_format_in_use(4) == 0
        got = _drive(ses, f, S.CASE_1_OPS, lens.tolist())
    out = _table(got, 11)
    assert torch.equal(out, ref) and torch.equal(out, want)
    for q in range(11):
        assert got[q][0].shape[0] == int(lens[q]) and got[q][0].dtype == torch.int64


@pytest.mark.parametrize("name,S_,R,C,L", [("turnover", 70, 33, 40, 8), ("more_rows_than_ring", 30, 8, 4, 6)])
def test_ring_turns_over_fp32(model, feats, oracle, name, S_, R, C, L):  # noqa: F811
    """70 rows in submits of 10 every 3 steps through 33 rows (two row tiles of the fused plan) and a ring of 40; 30 rows through
    8 rows and a ring of 4 - more rows than ring, several revolutions."""
    lm = model.language_model
    f = feats[:S_].to(DEV)
    ref = lm.generate(f, L).cpu()
    want, lens = TR._oracle_ids(oracle, S_, L)
    with lm.open_rolling(L, rows=R, capacity=C) as ses:
        got = _drive(ses, f, _ops(name), _lengths(want, L))
    assert torch.equal(_table(got, S_), ref) and torch.equal(ref, want)


def _all_at_once(lm, eng, f, L, R):
    one = lm.generate_rolling(f, L, rows=R).cpu()
    steps = eng.last_rolling_steps
    with lm.open_rolling(L, rows=R, capacity=f.shape[0]) as ses:
        got = _drive(ses, f, [("submit", f.shape[0])])
        assert ses.steps == steps
    assert torch.equal(_table(got, f.shape[0]), one)
    return one, steps


def test_all_rows_before_the_first_step_is_generate_rolling(model, feats):  # noqa: F811
    """The same schedule on the same plan: ids and device step count equal, fp32 on 4 rows and 150 rows through 70 under bf16 / fp16."""
    lm, eng = model.language_model, model.engine()
    _all_at_once(lm, eng, feats[:11].to(DEV), 12, 4)
    for dtype in (torch.bfloat16, torch.float16):
        with torch.autocast("cuda", dtype=dtype):
            _all_at_once(lm, eng, feats[:150].to(DEV), 9, 70)
            assert eng.kv_format_in_use(70) == (2 if dtype == torch.float16 else 1)


@pytest.mark.parametrize("dtype,tie", [(d, t) for d, S_, R, L, t in TR.CASES_16 if (S_, R, L) == (150, 70, 9)])
def test_16bit_arrivals(model, feats, dtype, tie):  # noqa: F811
    """R = 70 (the many-sequence step on the 16-bit cache), C = 100, 150 rows, L = 9: two arrival schedules, each under the rule of
    tests/test_gpu_rolling.py::_rule_16bit with that file's tolerance; 70 rows at once on 70 rows are generate()'s."""
    lm = model.language_model
    f = feats[:150].to(DEV)
    outs = []
    with torch.autocast("cuda", dtype=dtype):
        for m, k in ((50, 2), (30, 3)):
            with lm.open_rolling(9, rows=70, capacity=100) as ses:
                got = _drive(ses, f, [("stream", 150, m, k)])
            out = _table(got, 150)
            assert (out[:, 0] == EOS).all() and out.shape[1] <= 9
            outs.append(out)
        ref = lm.generate(f[:70], 9).cpu()
        with lm.open_rolling(9, rows=70, capacity=100) as ses:
            lock = _table(_drive(ses, f[:70], [("submit", 70)]), 70)
    assert torch.equal(lock, ref), (lock.tolist(), ref.tolist())
    width = max(o.shape[1] for o in outs)      # one teacher-forced oracle pass over both schedules' histories
    both = torch.cat([torch.nn.functional.pad(o, (0, width - o.shape[1]), value=PAD) for o in outs])
    TR._rule_16bit(both, torch.cat([feats[:150], feats[:150]]), tie)


def test_sampling_session_equals_sample_rolling(model, feats):  # noqa: F811
    """fp32, n = 2, R = 4, C = 8 sequences, a fixed seed, arrivals in three submits: ids and log-probs bit for bit."""
    lm = model.language_model
    f = feats[:9].to(DEV)
    kw = dict(temperature=0.9, top_k=40, top_p=0.95, num_return_sequences=2, seed=20240607)
    ids, lp = lm.sample_rolling(f, 12, rows=4, return_logprobs=True, **kw)
    ids, lp = ids.cpu(), lp.cpu()
    with lm.open_rolling(12, rows=4, capacity=4, do_sample=True, **kw) as ses:
        assert ses.n == 2 and ses.capacity * ses.n == 8
        got = _drive(ses, f, _ops("sampling_n2"), _lengths(torch.nn.functional.pad(ids, (0, 12 - ids.shape[1]), value=PAD), 12))
    assert torch.equal(_table(got, 18), ids)
    assert torch.equal(_table(got, 18, col=1), lp)
    assert len(set(_lengths(ids, 12))) >= 2


def test_idle_and_reuse(model, feats, oracle):  # noqa: F811
    lm = model.language_model
    f = feats[:11].to(DEV)
    want, lens = TR._oracle_ids(oracle, 11, 12)
    with lm.open_rolling(12, rows=4, capacity=8) as ses:
        assert ses.advance() == 0 and ses.advance(3) == 0 and ses.collect() == []       # nothing was ever submitted
        ses.submit(f[:3])
        assert ses.advance() > 0 and ses.unfinished == 0
        steps = ses.steps
        assert ses.advance() == 0 and ses.advance(5) == 0 and ses.steps == steps          # drained: nothing is launched
        first = {q: ids for q, ids in ses.collect()}
        ses.submit(f[3:5])
        assert ses.unfinished == 2 and ses.advance() > 0 and ses.steps > steps
        first.update({q: ids for q, ids in ses.collect()})
    for q in range(5):
        assert torch.equal(first[q].cpu(), want[q, :int(lens[q])])
    with lm.open_rolling(12, rows=4, capacity=8) as ses:      # the model's counts for the same calls
        _drive(ses, f, _ops("idle_and_reuse"), lens.tolist())


def test_graph_equals_eager(model, feats, oracle):  # noqa: F811
    eng = model.engine()
    f = feats[:11].to(DEV)
    want, lens = TR._oracle_ids(oracle, 11, 12)
    outs = []
    for use_graph in (True, False):
        with eng.open_rolling(12, 4, 6, use_graph=use_graph) as ses:
            outs.append(_table(_drive(ses, f, S.CASE_1_OPS, lens.tolist()), 11))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], want)


def test_staleness_and_refusals(model, feats):  # noqa: F811
    lm = model.language_model
    f = feats[:9].to(DEV)
    ref = lm.generate(f, 6)
    for bad in (dict(rows=4, capacity=0), dict(rows=0), dict(rows=-2), dict(rows=None)):
        with pytest.raises(ValueError):
            lm.open_rolling(6, **bad)
    for L in (1, None):
        with pytest.raises(ValueError, match="max_length"):
            lm.open_rolling(L, rows=4)
    with pytest.raises(ValueError, match="temperature"):
        lm.open_rolling(6, rows=4, do_sample=True, temperature=0.0)
    ses = lm.open_rolling(6, rows=4)
    assert ses.capacity == 16
    with pytest.raises(ValueError, match="already open"):
        lm.open_rolling(6, rows=4)
    ses.submit(f[:5])
    ses.advance(1)
    assert torch.equal(lm.generate(f, 6), ref)                 # works as without a session ...
    for call in (lambda: ses.advance(), lambda: ses.submit(f[5:6]), lambda: ses.collect()):
        with pytest.raises(_hip.RgrgHipError, match="stale"):   # ... and the session has lost its rows
            call()
    ses.close()
    ses.close()
    with pytest.raises(_hip.RgrgHipError, match="closed"):
        ses.submit(f[:1])
    with lm.open_rolling(6, rows=4) as again:                   # a new session opens afterwards
        got = _drive(again, f, [("submit", 9)])
    assert torch.equal(_table(got, 9), ref.cpu())
    # a stale session that was not closed does not block the next open
    stale = lm.open_rolling(6, rows=4)
    lm.generate(f, 6)
    with pytest.raises(_hip.RgrgHipError, match="stale"):
        stale.advance()
    with lm.open_rolling(6, rows=4) as again:
        assert stale.closed and again.advance() == 0
    # the e4m3 cache where it would be used: refused at open, naming the format
    lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with pytest.raises(_hip.RgrgHipError, match="e4m3"):
                lm.open_rolling(6, rows=70)
            with lm.open_rolling(6, rows=4) as small:          # 4 rows keep an fp32 cache: the setting has no effect there
                assert small.advance() == 0
    finally:
        lm.set_kv_cache_dtype(None)


def _same_result(got, ref):
    assert not isinstance(ref, int) and len(got) == 4
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[3])
    assert sorted(got[2]) == sorted(ref[2]) and all(torch.equal(got[2][k], ref[2][k]) for k in ref[2])


def test_report_model_open_rolling():
    import rgrg_amd
    m = gpu_model("ragged")
    images = synth.make_images(3, 1234).to(DEV)
    ref_a = m.generate_rolling(images[:2], 8, rows=16)
    ref_b = m.generate_rolling(images[2:], 8, rows=16)
    with m.open_rolling(8, rows=16, capacity=96) as ses:
        a = ses.submit(images[:2])
        assert ses.advance(3) == 3
        early = ses.collect()
        b = ses.submit(images[2:])
        ses.advance()
        done = dict(early + ses.collect())
        assert ses.unfinished == 0 and ses.collect() == []
    assert (a, b) == (0, 1) and sorted(done) == [0, 1]
    _same_result(done[a], ref_a)
    _same_result(done[b], ref_b)
    print(f"SESSION report model: {ref_a[0].shape[0]} + {ref_b[0].shape[0]} selected regions through 16 rows")
    sd0 = dict(synth_sd("ragged"))
    sd0["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m0 = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m0.load_state_dict(sd0)
    m0.to(DEV).eval()
    try:
        with m0.open_rolling(6, rows=4) as ses:
            t = ses.submit(images[:1])
            assert ses.collect() == [(t, -1)] and ses.unfinished == 0 and ses.advance() == 0
    finally:
        m0.invalidate_engine()
