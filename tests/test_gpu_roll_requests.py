"""Requests of a rolling session end to end on the MI355X (RollingSession.submit(.., max_length, temperature, top_k,
top_p, seed, stop_token_ids), RollingSession.cancel, ReportRollingSession): every submit is decoded as the stand-alone call with its
parameters decodes its feature rows, whatever else is in the session, and the host's counts - steps launched, unfinished, device
steps, finished sets, watermark, cancelled - are those of the numpy model (tests/rolling_request_reference.py) driven by the same calls.

Weights, feature rows, the gap condition and the 16-bit rule are those of tests/test_gpu_rolling.py (imported, not copied; the
condition is re-asserted by tests/test_gpu_roll_session.py on the same fixtures): in fp32 the reference alone decides every token.
R = 4 rows and a ring of 6 sequences unless a test says otherwise."""
import pytest
import torch

import rolling_request_reference as Q
import test_gpu_roll_session as TS
import test_gpu_rolling as TR
from conftest import gpu_model
from test_gpu_rolling import feats, model, oracle  # noqa: F401  (fixtures)
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = PAD = 50256


def _drive(ses, f, ops, lengths=None):
    """Runs ops (rolling_request_reference.play's) on the session - and, given the sentences' natural lengths, on the numpy model,
    comparing every count the host reports - then drains and collects -> ({q: (ids[, logprobs])}, [(range, keywords)] of the submits)."""
    R, C, n, L = ses.rows, ses.capacity * ses.n, ses.n, ses.max_length
    mdl = Q.Session(lengths, R, C, n, L) if lengths is not None else None
    got, subs, fed = {}, [], 0
    to_model = lambda kw: {k: v for k, v in kw.items() if k == "max_length"}   # noqa: E731  (the model's tokens are not the decoder's)
    for op in list(ops) + [("advance", None), ("collect",)]:
        before = (ses.submitted, ses.unfinished, ses.watermark)
        if op[0] == "submit":
            r = ses.submit(f[fed:fed + op[1]], **op[2])
            assert r == range(fed * n, (fed + op[1]) * n) and (mdl is None or r == mdl.submit(op[1], **to_model(op[2])))
            subs.append((r, op[2]))
            fed += op[1]
        elif op[0] == "refused":
            with pytest.raises(_hip.RgrgHipError, match=f"capacity {ses.capacity} feature rows"):
                ses.submit(f[fed:fed + op[1]], **op[2])
            assert (ses.submitted, ses.unfinished, ses.watermark) == before
        elif op[0] == "cancel":
            ses.cancel(op[1])
            if mdl is not None:
                mdl.cancel(op[1])
        elif op[0] == "bad_cancel":
            with pytest.raises(ValueError, match="can be cancelled"):
                ses.cancel(op[1])
            assert (ses.submitted, ses.unfinished, ses.watermark) == before
        elif op[0] == "advance":
            launched = ses.advance(op[1])
            if mdl is not None:
                assert launched == mdl.advance(op[1]) and ses.unfinished == mdl.unfinished and ses.steps == mdl.device_steps
        else:
            items = ses.collect()
            if mdl is not None:
                assert [it[0] for it in items] == mdl.collect() and ses.watermark == mdl.watermark and ses.cancelled == mdl.cancelled
            for it in items:
                assert it[0] not in got
                got[it[0]] = it[1:]
    assert ses.unfinished == 0 and ses.watermark == ses.submitted == fed * n and sorted(got) == list(range(fed * n))
    return got, subs


def _rows(got, qs, col=0):
    """The collected sentences qs as the stand-alone calls return them: [len(qs), longest], PAD (log-probs: 0) behind a sentence's end."""
    qs = list(qs)
    width = max(got[q][0].shape[0] for q in qs)
    out = torch.full((len(qs), width), PAD if col == 0 else 0, dtype=got[qs[0]][col].dtype)
    for i, q in enumerate(qs):
        out[i, :got[q][col].shape[0]] = got[q][col].cpu()
    return out


# ------------------------------------------------------------------------------------------------ 1. limits, 6. graph = eager
def _limits(model, feats, oracle, name, opener):  # noqa: F811
    lm = model.language_model
    f = feats[:11].to(DEV)
    _, lens = TR._oracle_ids(oracle, 11, 12)
    with opener() as ses:
        assert model.engine().kv_format_in_use(4) == 0
        got, subs = _drive(ses, f, Q.LIMITS_OPS[name], lens.tolist())
        assert ses.cancelled == set()
    assert len({kw.get("max_length") for _, kw in subs}) == 3        # 6, 8 and None
    for rng, kw in subs:
        ml = kw.get("max_length", 12)
        ref = lm.generate(f[rng.start:rng.stop], ml).cpu()
        want, _ = TR._oracle_ids(oracle, rng.stop, ml)
        assert torch.equal(_rows(got, rng), ref), (name, rng, kw)
        assert torch.equal(ref[:, :want.shape[1]], want[rng.start:, :ref.shape[1]])
    return got


@pytest.mark.parametrize("name", sorted(Q.LIMITS_OPS))
def test_limits_per_submit_fp32(model, feats, oracle, name):  # noqa: F811
    """A greedy session at L = 12 takes submits with max_length 6, 8 and None while steps run: each submit's rows are generate()'s at
    its limit, the host counts the model's."""
    lm = model.language_model
    _limits(model, feats, oracle, name, lambda: lm.open_rolling(12, rows=4, capacity=6))


def test_graph_equals_eager_limits_and_cancel(model, feats, oracle):  # noqa: F811
    eng = model.engine()
    f = feats[:11].to(DEV)
    _, lens = TR._oracle_ids(oracle, 11, 12)
    a = _limits(model, feats, oracle, "case_1", lambda: eng.open_rolling(12, 4, 6, use_graph=True))
    b = _limits(model, feats, oracle, "case_1", lambda: eng.open_rolling(12, 4, 6, use_graph=False))
    assert all(torch.equal(a[q][0], b[q][0]) for q in a)
    outs = []
    for use_graph in (True, False):
        with eng.open_rolling(12, 4, 8, use_graph=use_graph) as ses:
            got, _ = _drive(ses, f, Q.CANCEL_OPS, lens.tolist())
            outs.append((got, set(ses.cancelled)))
    assert outs[0][1] == outs[1][1] == set(Q.CANCEL_CUT) and all(torch.equal(outs[0][0][q][0], outs[1][0][q][0]) for q in outs[0][0])


# ------------------------------------------------------------------------------------------------ 4. cancel
def test_cancel_running_pending_and_finished_fp32(model, feats, oracle):  # noqa: F811
    """A ring of 8: sequence 0 is cut while it runs (3 tokens: the first 3 of its generate() row), 6 while it is pending (BOS alone), 1
    had ended (intact); `cancelled` holds exactly the first two; every other sentence is generate()'s; the counts - the pending
    sequence takes the freed row in the same step among them - are the model's."""
    lm = model.language_model
    f = feats[:9].to(DEV)
    ref = lm.generate(f, 12).cpu()
    _, lens = TR._oracle_ids(oracle, 9, 12)
    with lm.open_rolling(12, rows=4, capacity=8) as ses:
        got, _ = _drive(ses, f, Q.CANCEL_OPS, lens.tolist())
        assert ses.cancelled == {0, 6}
    for q in range(9):
        k = Q.CANCEL_CUT.get(q, int(lens[q]))
        assert got[q][0].dtype == torch.int64 and torch.equal(got[q][0].cpu(), ref[q, :k]), (q, got[q][0].tolist(), ref[q].tolist())
    assert int(lens[0]) > 3 and int(lens[1]) == 3      # 0 was cut short, 1 is complete although it was cancelled


# ------------------------------------------------------------------------------------------------ 5. stop tokens
def test_stop_tokens_fp32(model, feats, oracle):  # noqa: F811
    lm = model.language_model
    f = feats[:7].to(DEV)
    want, lens = TR._oracle_ids(oracle, 7, 12)
    # the second generated token of a row that has one, and that another row never produces (checked on the oracle run, on the CPU)
    pick = None
    for r in range(7):
        if int(lens[r]) >= 4 and int(want[r, 2]) != EOS:
            t = int(want[r, 2])
            if any(t not in want[o, 1:int(lens[o])].tolist() for o in range(7) if o != r):
                pick = (r, t)
                break
    assert pick is not None
    r, t = pick
    ref = lm.generate(f, 12).cpu()
    with lm.open_rolling(12, rows=4, capacity=8) as ses:      # (a ring of 8: the second submit fits whichever row was picked)
        got, _ = _drive(ses, f, [("submit", 4, dict(stop_token_ids=[t])), ("advance", 2), ("collect",), ("submit", 3, dict(stop_token_ids=[3, 5, 7, t]))])
        assert ses.cancelled == set()
    assert got[r][0].cpu().tolist() == want[r, :3].tolist() and got[r][0][-1] == t      # ends there, the stop token last
    unchanged = 0
    for q in range(7):
        row = ref[q, :int(lens[q])].tolist()
        cut = row[:row.index(t, 1) + 1] if t in row[1:] else row
        unchanged += cut == row
        assert got[q][0].cpu().tolist() == cut, (q, t)
    assert unchanged >= 1


# ------------------------------------------------------------------------------------------------ 2. + 3. sampling requests
SESSION_KW = dict(temperature=0.9, top_k=40, top_p=0.95, num_return_sequences=2, seed=20240607)
REQ_A = dict(temperature=0.7, top_k=20, top_p=0.9, seed=11)
REQ_B = dict(temperature=1.3, top_k=0, top_p=0.8, seed=2 ** 40 + 3)
REQ_C = dict(temperature=1.0, top_k=5, top_p=1.0, seed=11, max_length=8)


def _submit_when_room(ses, f, got, **kw):
    """submit, stepping and collecting while the ring is full."""
    for _ in range(64):
        try:
            return ses.submit(f, **kw)
        except _hip.RgrgHipError as e:
            assert "capacity" in str(e)
            ses.advance(2)
            for it in ses.collect():
                got[it[0]] = it[1:]
    raise AssertionError("the ring never made room")


def _drain(ses, got):
    ses.advance()
    for it in ses.collect():
        assert it[0] not in got
        got[it[0]] = it[1:]
    assert ses.unfinished == 0 and ses.watermark == ses.submitted


def test_sampling_requests_equal_sample_rolling_fp32(model, feats):  # noqa: F811
    """n = 2, R = 4, a ring of 6 sequences.  A first submit without keywords is sample_rolling under the session's seed (today's
    numbering); three more with their own (temperature, top_k, top_p, seed) join at different steps, wrap the ring, and are
    sample_rolling on their feature rows alone with those values - ids and log-probs bit for bit."""
    lm = model.language_model
    f = feats[:7].to(DEV)
    got, subs = {}, []
    with lm.open_rolling(12, rows=4, capacity=3, do_sample=True, **SESSION_KW) as ses:
        assert ses.n == 2 and ses.capacity * ses.n == 6
        subs.append((ses.submit(f[0:2]), 0, 2, {}))
        ses.advance(2)
        subs.append((_submit_when_room(ses, f[2:3], got, **REQ_A), 2, 3, REQ_A))
        ses.advance(1)
        subs.append((_submit_when_room(ses, f[3:5], got, **REQ_B), 3, 5, REQ_B))
        ses.advance(3)
        subs.append((_submit_when_room(ses, f[5:7], got, **REQ_C), 5, 7, REQ_C))
        _drain(ses, got)
        assert ses.submitted == 14 and ses.cancelled == set()
    assert [r for r, *_ in subs] == [range(0, 4), range(4, 6), range(6, 10), range(10, 14)]
    for rng, lo, hi, kw in subs:
        kw = dict(SESSION_KW, **kw)
        ml = kw.pop("max_length", 12)
        ids, lp = lm.sample_rolling(f[lo:hi], ml, rows=4, return_logprobs=True, **kw)
        assert torch.equal(_rows(got, rng), ids.cpu()), (rng, kw)
        assert torch.equal(_rows(got, rng, col=1), lp.cpu()), (rng, kw)


def test_greedy_and_stopped_requests_in_a_sampling_session_fp32(model, feats, oracle):  # noqa: F811
    """top_k = 1 requests between sampled ones are the rows of generate(); a sampled request with a stop token is sample_rolling's row
    up to that token."""
    lm = model.language_model
    f = feats[:7].to(DEV)
    ids_b, lp_b = lm.sample_rolling(f[4:5], 12, rows=4, return_logprobs=True, **dict(SESSION_KW, **REQ_A))
    ids_b, lp_b = ids_b.cpu(), lp_b.cpu()
    row = ids_b[0].tolist()
    n_b = row.index(EOS, 1) + 1 if EOS in row[1:] else len(row)
    stop = row[2] if n_b >= 4 else None          # the second drawn token of hypothesis 0, when it is not the last
    got = {}
    with lm.open_rolling(12, rows=4, capacity=3, do_sample=True, **SESSION_KW) as ses:
        ses.submit(f[0:1], **REQ_B)
        ses.advance(1)
        g1 = _submit_when_room(ses, f[1:3], got, top_k=1)
        ses.advance(2)
        sb = _submit_when_room(ses, f[4:5], got, stop_token_ids=None if stop is None else [stop], **REQ_A)
        g2 = _submit_when_room(ses, f[3:4], got, top_k=1, max_length=8)
        _drain(ses, got)
    ref = lm.generate(f[:4], 12).cpu()
    want, lens = TR._oracle_ids(oracle, 4, 12)
    assert torch.equal(ref, want)
    for rng, rows in ((g1, (1, 2)), (g2, (3,))):
        for i, q in enumerate(rng):
            src = rows[i // 2]
            k = min(int(lens[src]), 8 if rng is g2 else 12)
            assert torch.equal(got[q][0].cpu(), ref[src, :k]), (q, src)
            assert got[q][1].cpu().abs().max().item() <= 1e-6         # one token is kept: q = 1
    for i, q in enumerate(sb):
        r = ids_b[i].tolist()
        n = r.index(EOS, 1) + 1 if EOS in r[1:] else len(r)
        k = r.index(stop, 1) + 1 if stop is not None and stop in r[1:n] else n
        assert got[q][0].cpu().tolist() == r[:k] and torch.equal(got[q][1].cpu(), lp_b[i, :k]), (q, stop)
    print(f"REQUESTS sampling session: stop token {stop}, hypothesis 0 kept {got[sb[0]][0].shape[0]} of {n_b} tokens")


# ------------------------------------------------------------------------------------------------ 7. the 16-bit plan
def test_16bit_requests_bf16(model, feats):  # noqa: F811
    """R = 70 under bf16 autocast (the many-sequence step on the 16-bit cache), a sampling session whose submits carry max_length and
    top_k = 1.  70 rows at once are the stand-alone sample_rolling(.., top_k=1) on 70 rows at that limit - the same rows, plan and order
    of work -; arrivals in two submits with different limits are judged by tests/test_gpu_rolling.py::_rule_16bit with the tolerance
    of its bf16 case at these shapes, as tests/test_gpu_roll_session.py::test_16bit_arrivals judges that path."""
    tie = [t for d, S_, R, L, t in TR.CASES_16 if (d, S_, R, L) == (torch.bfloat16, 150, 70, 9)][0]
    lm, eng = model.language_model, model.engine()
    f = feats[:100].to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with lm.open_rolling(9, rows=70, capacity=100, do_sample=True, temperature=0.8, top_k=30, seed=5) as ses:
            assert eng.kv_format_in_use(70) == 1
            got = {}
            a = ses.submit(f[:50], max_length=8, top_k=1)
            ses.advance(2)
            b = ses.submit(f[50:100], max_length=6, top_k=1)
            _drain(ses, got)
        with lm.open_rolling(9, rows=70, capacity=100, do_sample=True, temperature=0.8, top_k=30, seed=5) as ses:
            lock = {}
            ses.submit(f[:70], max_length=8, top_k=1)
            _drain(ses, lock)
        ref = lm.sample_rolling(f[:70], 8, rows=70, top_k=1).cpu()
    assert torch.equal(_rows(lock, range(70)), ref)
    for rng, ml in ((a, 8), (b, 6)):
        out = _rows(got, rng)
        assert (out[:, 0] == EOS).all() and out.shape[1] <= ml and max(got[q][0].shape[0] for q in rng) <= ml
        TR._rule_16bit(out, feats[rng.start:rng.stop], tie)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_session_as_it_was(model, feats):  # noqa: F811
    lm = model.language_model
    f = feats[:9].to(DEV)

    def refused(ses, call, match, exc=ValueError):
        before = (ses.submitted, ses.unfinished, ses.watermark)
        with pytest.raises(exc, match=match):
            call()
        assert (ses.submitted, ses.unfinished, ses.watermark) == before

    with lm.open_rolling(12, rows=4, capacity=6) as ses:
        refused(ses, lambda: ses.cancel(0), "can be cancelled")                    # nothing submitted yet
        ses.submit(f[:3])
        for ml in (1, 13, 0, 2.5):
            refused(ses, lambda: ses.submit(f[3:4], max_length=ml), "max_length")
        for kw in (dict(temperature=0.5), dict(top_k=1), dict(top_p=0.9), dict(seed=3)):
            refused(ses, lambda: ses.submit(f[3:4], **kw), "greedy session")
        refused(ses, lambda: ses.submit(f[3:4], stop_token_ids=[1, 2, 3, 4, 5]), "up to 4")
        refused(ses, lambda: ses.submit(f[3:4], stop_token_ids=[-1]), "token ids")
        refused(ses, lambda: ses.cancel(3), "can be cancelled")                    # not submitted
        refused(ses, lambda: ses.cancel([1, -1]), "can be cancelled")
        refused(ses, lambda: ses.submit(f[:4], max_length=6), "capacity 6 feature rows", _hip.RgrgHipError)   # ring full, with a request
        ses.advance()
        assert [q for q, _ in ses.collect()] == [0, 1, 2] and ses.watermark == 3
        refused(ses, lambda: ses.cancel(2), "can be cancelled")                    # below the watermark
        assert ses.cancelled == set()
        r = ses.submit(f[3:5], max_length=2, stop_token_ids=[7])                   # the session still works
        ses.advance()
        assert [(q, ids.shape[0]) for q, ids in ses.collect()] == [(r[0], 2), (r[1], 2)]
    # the C entries refuse on their own
    eng = model.engine()
    with eng.open_rolling(12, 4, 6) as ses:
        lib, dec, p = eng.lib, ses._dec, _hip.ptr(f)
        assert lib.rgrg_decoder_roll_submit_req(dec, p, 1, 13, 0.0, -1, 0.0, 0, 0, None, 0, None, None) != 0 and b"max_length" in lib.rgrg_last_error()
        assert lib.rgrg_decoder_roll_submit_req(dec, p, 1, 0, 0.0, 1, 0.0, 0, 0, None, 0, None, None) != 0 and b"greedy session" in lib.rgrg_last_error()
        assert lib.rgrg_decoder_roll_submit_req(dec, p, 1, 0, 0.0, -1, 0.0, 0, 0, None, 5, None, None) != 0
        assert lib.rgrg_decoder_roll_cancel(dec, 0, 1) != 0 and b"the ring holds" in lib.rgrg_last_error()
        assert (ses.advance(), ses.unfinished) == (0, 0)
    with lm.open_rolling(12, rows=4, capacity=3, do_sample=True, **SESSION_KW) as ses:
        for kw, match in ((dict(temperature=0.0), "temperature"), (dict(top_p=1.5), "top_p"), (dict(top_k=-1), "top_k"), (dict(top_p=0.0), "top_p"),
                          (dict(seed=1.5), "seed")):
            refused(ses, lambda: ses.submit(f[:1], **kw), match)
        assert ses.submit(f[:1], top_k=1) == range(0, 2)
    with lm.open_rolling(6, rows=4, num_beams=2) as ses:
        refused(ses, lambda: ses.submit(f[:1], max_length=5), "beam session")
        refused(ses, lambda: ses.submit(f[:1], stop_token_ids=[3]), "beam session")
        refused(ses, lambda: ses.cancel(0), "beam session")
        assert ses.submit(f[:1]) == range(0, 1)
        refused(ses, lambda: ses.cancel(0), "beam session")
    # the e4m3 cache where it would be used is still refused at open
    lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with pytest.raises(_hip.RgrgHipError, match="e4m3"):
                lm.open_rolling(6, rows=70)
    finally:
        lm.set_kv_cache_dtype(None)


# ------------------------------------------------------------------------------------------------ 9. the report model
def test_report_model_requests_and_cancel():
    m = gpu_model("ragged")
    images = synth.make_images(2, 1234).to(DEV)
    ref_a = m.generate_rolling(images[:1], 6, rows=16)
    ref_b = m.generate_rolling(images[1:], 8, rows=16)
    with m.open_rolling(8, rows=16, capacity=96) as ses:
        a = ses.submit(images[:1], max_length=6)
        b = ses.submit(images[1:])
        with pytest.raises(ValueError, match="max_length"):
            ses.submit(images[:1], max_length=9)
        assert ses.advance(2) == 2
        ses.cancel(b)
        ses.advance()
        done = dict(ses.collect())
        assert ses.unfinished == 0 and ses.collect() == [] and sorted(done) == [a, b] == [0, 1]
        assert b in ses.cancelled and a not in ses.cancelled
        with pytest.raises(ValueError, match="not open"):
            ses.cancel(b)
    TS._same_result(done[a], ref_a)
    got_b = done[b]
    assert len(got_b) == 4 and torch.equal(got_b[1], ref_b[1]) and torch.equal(got_b[3], ref_b[3]) and got_b[0].shape[0] == ref_b[0].shape[0]
    cut = 0
    for row, full in zip(got_b[0].tolist(), ref_b[0].tolist()):       # every sentence is a prefix of its whole one: BOS alone, or 3 tokens
        full = full + [PAD] * (8 - len(full))
        k = max(i + 1 for i, t in enumerate(row) if i == 0 or t != PAD)
        assert row[:k] == full[:k] and all(t == PAD for t in row[k:])
        cut += k < 8 and full[k] != PAD                                # (EOS and PAD are one id: a cut in front of the EOS does not show)
    assert cut >= 1
    print(f"REQUESTS report model: ticket {b} cancelled, {cut} of {len(got_b[0])} sentences cut")
