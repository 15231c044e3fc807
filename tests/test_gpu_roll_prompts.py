"""Prompts in a rolling session end to end on the MI355X (LanguageModel.open_rolling(.., max_prompt_length),
RollingSession.submit(feats, prompt_ids=..), ReportRollingSession.submit(images, region_prompts=..)): a submitted sentence continues
its prompt as greedy_search continues input_ids under a mask of ones - whatever row it takes, whatever else is in the session.

Weights: the ``ragged`` synthetic profile, fp32 unless a test says otherwise.  fp32 token ids are held to the REAL reference
(tests/golden/lm_prompt_greedy.pt) and to the oracle loop of tests/rolling_prompt_reference.py under the project's gap rule: the
oracle's smallest top-2 logit gap over the generated positions is asserted to be >= 2e-3 (the logit tolerance of
tests/test_gpu_lm_forms.py) before ids are compared, so no plan's rounding changes an arg-max.  One submit has one prompt length:
ragged prompts are separate submits, in order of q.  The 16-bit plans are held to tests/test_gpu_prompted.py::_rule_16bit.

In fp32 the prompt pass takes no split-K, so its result does not depend on how many prompt rows ran together; sampled sessions are
compared bit for bit across rows, schedules and hypothesis counts (the same submits in every run)."""
import pytest
import torch

import rolling_prompt_reference as P
import test_gpu_prompted as TP
from conftest import gpu_model, load_golden, synth_sd
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = PAD = 50256
TOL_GAP = 2e-3


def _lm():
    return gpu_model("ragged").language_model


def _drain(ses, got):
    ses.advance()
    for it in ses.collect():
        assert it[0] not in got
        got[it[0]] = it[1:]
    assert ses.unfinished == 0 and ses.watermark == ses.submitted


def _play(ses, subs, stagger=False):
    """subs: [(feats [m, 1024], prompt [m, P] / [P] / None, keywords)] -> ({q: (ids[, logprobs])}, the ranges).  stagger: two steps
    between the submits."""
    got, rngs = {}, []
    for f, p, kw in subs:
        rngs.append(ses.submit(f.to(DEV), prompt_ids=p, **kw))
        if stagger:
            ses.advance(2)
            for it in ses.collect():
                got[it[0]] = it[1:]
    _drain(ses, got)
    return got, rngs


def _trim(row, P_):
    """A row of greedy_search / the fixture -> its tokens: up to the first generated EOS."""
    row = row.tolist()
    return row[:next((j + 1 for j in range(P_, len(row)) if row[j] == EOS), len(row))]


def _singles(prompts, feats, **kw):
    return [(feats[q:q + 1], prompts[q][None, :], dict(kw)) for q in range(len(prompts))]


# ------------------------------------------------------------------------------------------------ the real reference's rows
def test_fixture_rows_unpadded_fp32():
    """The 13 rows of the prompted-greedy fixture, each submitted alone with its prompt stripped of padding (P = 2 .. 5) and its
    case's max_length (one_token: 5), through 4 rows.  12 must be the fixture's row (pad columns and PAD behind the end aside, on the
    columns the fixture has: its rows end at the PADDED width).  Row 0 of leftpad_s4_t5 is left out, and only that row: the oracle
    reproduces all 13 unpadded rows on the CPU with top-2 gaps of 4.9e-4 for that row and >= 1.09e-2 for the other twelve."""
    fx = load_golden("lm_prompt_greedy.pt")
    subs, want = [], []
    for case in ("ones_s3_t4", "eos_inside_s3_t4", "one_token_s3_t4", "leftpad_s4_t5"):
        c = fx["cases"][case]
        for s in range(c["input_ids"].shape[0]):
            pad = int((c["attention_mask"][s] == 0).sum())
            prompt = c["input_ids"][s, pad:]
            ml = 5 if case == "one_token_s3_t4" else int(c["max_length"])
            subs.append((c["feats"][s:s + 1], prompt[None, :], dict(max_length=ml)))
            want.append((case, s, _trim(c["output_ids"][s, pad:], prompt.shape[0])))
    assert len(subs) == 13 and sorted({p.shape[1] for _, p, _ in subs}) == [2, 3, 4, 5]
    with _lm().open_rolling(11, rows=4, capacity=13, max_prompt_length=5) as ses:
        got, _ = _play(ses, subs)
    checked = 0
    for q, (case, s, w) in enumerate(want):
        if (case, s) == ("leftpad_s4_t5", 0):
            continue
        g = got[q][0].cpu().tolist()
        assert g[:len(w)] == w and (len(g) == len(w) or w[-1] != EOS), (case, s, g, w)
        checked += 1
    assert checked == 12


# ------------------------------------------------------------------------------------------------ mixed lengths
@pytest.fixture(scope="module")
def mixed():
    g = torch.Generator().manual_seed(97)
    prompts = [torch.randint(0, 50000, ((1, 3, 2, 5, 4)[q % 5],), generator=g) for q in range(11)]
    feats = torch.randn((11, 1024), generator=g)
    ids, gap = P.oracle_greedy(synth_sd("ragged"), prompts, feats, 12)
    return dict(prompts=prompts, feats=feats, ids=ids, gap=gap)


def test_mixed_lengths_three_schedules_fp32(mixed):
    """11 prompts of 1, 3, 2, 5, 4, .. tokens, L = 12: all at once through 4 rows, through 3 rows, staggered between advance(2) calls -
    the oracle's ids for all 11 (lengths 2, 12, 3, 8, 5, 2, 9, 12, 12, 6, 4; smallest gap 3.09e-3), and greedy_search's per length group."""
    prompts, feats = mixed["prompts"], mixed["feats"]
    print(f"ROLLPROMPT mixed: oracle gap {mixed['gap']:.3e}, lengths {[len(x) for x in mixed['ids']]}")
    assert mixed["gap"] >= TOL_GAP and [len(x) for x in mixed["ids"]] == [2, 12, 3, 8, 5, 2, 9, 12, 12, 6, 4]
    lm = _lm()
    runs = []
    for rows, stagger in ((4, False), (3, False), (4, True)):
        with lm.open_rolling(12, rows=rows, capacity=11, max_prompt_length=5) as ses:
            got, rngs = _play(ses, _singles(prompts, feats), stagger)
            assert rngs == [range(q, q + 1) for q in range(11)]
        runs.append([got[q][0].cpu() for q in range(11)])
    for run in runs:
        for q in range(11):
            assert run[q].dtype == torch.int64 and torch.equal(run[q], mixed["ids"][q]), (q, run[q].tolist(), mixed["ids"][q].tolist())
            assert torch.equal(run[q], runs[0][q])
    for p in (1, 2, 3, 4, 5):
        qs = [q for q in range(11) if prompts[q].shape[0] == p]
        ref = lm.greedy_search(torch.stack([prompts[q] for q in qs]).to(DEV), feats[qs].to(DEV), 12,
                               attention_mask=torch.ones((len(qs), p), dtype=torch.int64, device=DEV), use_cache=True).cpu()
        for i, q in enumerate(qs):
            assert _trim(ref[i], p) == runs[0][q].tolist(), (p, q)


def test_one_more_row_than_the_fused_plan_fp32():
    """129 rows (the tiled fp32 plan), 140 sequences in 28 submits of 5 with prompts of 4, 3, 2, 1, 4, .. tokens, L = 7.  The sequences
    that start in rows 0, 1, 2, 3, 31, 32, 127 and 128 are held to the oracle (seed chosen on the CPU: their smallest gap is 5.36e-3)."""
    held = [0, 1, 2, 3, 31, 32, 127, 128]
    g = torch.Generator().manual_seed(201)
    prompts = [torch.randint(0, 50000, ((4, 3, 2, 1)[(q // 5) % 4],), generator=g) for q in range(140)]
    feats = torch.randn((140, 1024), generator=g)
    want, gap = P.oracle_greedy(synth_sd("ragged"), [prompts[q] for q in held], feats[held], 7)
    print(f"ROLLPROMPT 129 rows: oracle gap {gap:.3e}")
    assert gap >= TOL_GAP
    m = gpu_model("ragged")
    subs = [(feats[q:q + 5], torch.stack(prompts[q:q + 5]), {}) for q in range(0, 140, 5)]
    with m.language_model.open_rolling(7, rows=129, capacity=140, max_prompt_length=4) as ses:
        assert m.engine().fused_row_limit() == 128 and m.engine().kv_format_in_use(129) == 0
        got, _ = _play(ses, subs)
    assert sorted(got) == list(range(140))
    for q, w in zip(held, want):
        assert torch.equal(got[q][0].cpu(), w), (q, got[q][0].tolist(), w.tolist())
    for q in range(140):
        p = prompts[q].shape[0]
        assert got[q][0][:p].cpu().tolist() == prompts[q].tolist() and p + 1 <= got[q][0].shape[0] <= 7


# ------------------------------------------------------------------------------------------------ a BOS column
def test_bos_column_is_no_prompt(mixed):
    lm = _lm()
    f = mixed["feats"][:6]
    bos = torch.full((6, 1), EOS, dtype=torch.int64)
    outs = []
    for prompt, mp in ((None, 0), (None, 3), (bos, 3), (bos[0], 3)):
        with lm.open_rolling(10, rows=4, capacity=6, max_prompt_length=mp) as ses:
            got, _ = _play(ses, [(f, prompt, {})])
        outs.append([got[q][0].cpu() for q in range(6)])
    assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(outs[0], o))
    kw = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, seed=11, num_return_sequences=2)
    outs = []
    for prompt, mp in ((None, 0), (bos, 3)):
        with lm.open_rolling(10, rows=4, capacity=6, max_prompt_length=mp, **kw) as ses:
            got, _ = _play(ses, [(f, prompt, {})])
        outs.append([got[q] for q in range(12)])
    for a, b in zip(*outs):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ sampling
SAMPLE = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, seed=20240607)


def _same(a, b):
    assert sorted(a) == sorted(b)
    for q in a:
        assert torch.equal(a[q][0], b[q][0]), (q, a[q][0].tolist(), b[q][0].tolist())
        assert torch.equal(a[q][1].view(torch.int32), b[q][1].view(torch.int32)), q


def test_sampling_rows_schedules_and_hypotheses_fp32(mixed):
    """Sequence q draws column c under the counter (q, c - 1) whichever row holds it, behind a prompt too: 4 rows = 7 rows, staggered
    = all at once (the same submits), n = 3 = repeat_interleave(3) with n = 1; top_k = 1 is the greedy prompted session; log-probs
    are 0 in the prompt columns."""
    lm = _lm()
    prompts, feats = mixed["prompts"], mixed["feats"]
    subs = _singles(prompts, feats)
    runs = {}
    for key, rows, stagger in (("r4", 4, False), ("r7", 7, False), ("st", 4, True)):
        with lm.open_rolling(12, rows=rows, capacity=11, max_prompt_length=5, num_return_sequences=3, **SAMPLE) as ses:
            runs[key], _ = _play(ses, subs, stagger)
    _same(runs["r4"], runs["r7"])
    _same(runs["r4"], runs["st"])
    rep = [(f.repeat_interleave(3, dim=0), p.repeat_interleave(3, dim=0), kw) for f, p, kw in subs]
    with lm.open_rolling(12, rows=4, capacity=33, max_prompt_length=5, num_return_sequences=1, **SAMPLE) as ses:
        one, _ = _play(ses, rep)
    _same(runs["r4"], one)
    lens = set()
    for q, (ids, lp) in runs["r4"].items():
        p = prompts[q // 3].shape[0]
        assert ids[:p].cpu().tolist() == prompts[q // 3].tolist() and (lp[:p] == 0).all() and (lp[p:] <= 0).all() and ids.shape == lp.shape
        lens.add(ids.shape[0] - p)
    assert len(lens) >= 3 and any(not torch.equal(runs["r4"][3 * i][0], runs["r4"][3 * i + 1][0]) for i in range(11))
    with lm.open_rolling(12, rows=4, capacity=11, max_prompt_length=5, **SAMPLE) as ses:
        greedy, _ = _play(ses, _singles(prompts, feats, top_k=1))
    for q in range(11):
        assert torch.equal(greedy[q][0].cpu(), mixed["ids"][q]) and greedy[q][1].abs().max().item() <= 1e-6


def test_a_submit_larger_than_one_pass_fp32():
    """150 prompts of 5 tokens in ONE submit are 600 prompt rows, more than the 512 a pass takes: two passes (128 + 22 sentences).  A
    greedy session on 70 rows; sentences 0, 1, 127 (the last of the first pass), 128, 129 (the first of the second) and 149 are held to
    the oracle (seed chosen on the CPU: their smallest gap is 2.6e-2), in that run and in one that submits the same sentences ten at
    a time.  Ids only, and under the gap rule: a submit of 150 feature rows and one of 10 are different row counts for the image key /
    value GEMMs of the prefill - as in a session without prompts - so the logits of the two runs may differ in their last bits."""
    held = [0, 1, 127, 128, 129, 149]
    g = torch.Generator().manual_seed(211)
    prompts = torch.randint(0, 50000, (150, 5), generator=g)
    feats = torch.randn((150, 1024), generator=g)
    want, gap = P.oracle_greedy(synth_sd("ragged"), [prompts[q] for q in held], feats[held], 8)
    print(f"ROLLPROMPT two passes: oracle gap {gap:.3e}")
    assert gap >= TOL_GAP
    lm = _lm()
    for step in (150, 10):
        with lm.open_rolling(8, rows=70, capacity=150, max_prompt_length=5) as ses:
            got, _ = _play(ses, [(feats[q:q + step], prompts[q:q + step], {}) for q in range(0, 150, step)])
        assert sorted(got) == list(range(150))
        for q, w in zip(held, want):
            assert torch.equal(got[q][0].cpu(), w), (step, q, got[q][0].tolist(), w.tolist())
        assert all(torch.equal(got[q][0][:5].cpu(), prompts[q]) and 6 <= got[q][0].shape[0] <= 8 for q in range(150))


# ------------------------------------------------------------------------------------------------ the 16-bit plans
@pytest.mark.parametrize("dtype,tie", [(torch.bfloat16, 3e-2), (torch.float16, 6e-3)])
def test_16bit_plans(dtype, tie):
    """70 rows under autocast (the many-sequence step on the 16-bit cache, a 16-bit prompt K/V ring), 150 sequences in 15 submits of
    10 with prompts of 1 .. 5 tokens, L = 9: the rule of tests/test_gpu_prompted.py on six sequences of every length group, twice the
    same bits, captured graph = eager."""
    g = torch.Generator().manual_seed(97)
    plen = [(1, 2, 3, 4, 5)[(q // 10) % 5] for q in range(150)]
    prompts = [torch.randint(0, 50000, (plen[q],), generator=g) for q in range(150)]
    feats = torch.randn((150, 1024), generator=g)
    subs = [(feats[q:q + 10], torch.stack(prompts[q:q + 10]), {}) for q in range(0, 150, 10)]
    m = gpu_model("ragged")
    eng = m.engine()
    runs = []
    with torch.autocast("cuda", dtype=dtype):
        for use_graph in (True, True, False):
            modes = m.language_model._decode_modes(DEV)
            with eng.open_rolling(9, 70, 150, use_graph=use_graph, max_prompt_length=5, **modes) as ses:
                assert eng.kv_format_in_use(70) == (2 if dtype == torch.float16 else 1)
                got, _ = _play(ses, subs)
            runs.append([got[q][0].cpu() for q in range(150)])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), "twice the same bits"
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[2])), "graph = eager"
    for p in (1, 2, 3, 4, 5):
        qs = [q for q in range(150) if plen[q] == p][:3] + [q for q in range(150) if plen[q] == p][-3:]
        width = max(runs[0][q].shape[0] for q in qs)
        hist = torch.full((len(qs), width), PAD, dtype=torch.int64)
        for i, q in enumerate(qs):
            assert runs[0][q][:p].tolist() == prompts[q].tolist() and p + 1 <= runs[0][q].shape[0] <= 9
            hist[i, :runs[0][q].shape[0]] = runs[0][q]
        ids = torch.stack([prompts[q] for q in qs])
        TP._rule_16bit(hist, ids, torch.ones_like(ids), feats[qs], list(range(len(qs))), tie)


# ------------------------------------------------------------------------------------------------ requests
def test_requests_with_prompts_fp32(mixed):
    lm = _lm()
    prompts, feats, ids = mixed["prompts"], mixed["feats"], mixed["ids"]
    # 1. a submit's max_length counts the prompt: sequence 3 (P = 5, 8 tokens) at 6 is its first 6 tokens, 6 (P = 3, 9 tokens) at 4 its first 4
    # 2. a stop token inside the prompt ends nothing, the same kind of token generated does: sequence 1 (P = 3, 12 tokens) with its second
    #    prompt token and its second GENERATED token as stop ids ends with the latter
    stop_in, stop_gen = int(prompts[1][1]), int(ids[1][4])
    assert stop_in not in ids[1][3:].tolist() and stop_gen not in ids[1][:4].tolist() and stop_in < 65535 and stop_gen < 65535
    with lm.open_rolling(12, rows=2, capacity=4, max_prompt_length=5) as ses:
        got, _ = _play(ses, [(feats[3:4], prompts[3], dict(max_length=6)), (feats[6:7], prompts[6][None, :], dict(max_length=4)),
                             (feats[1:2], prompts[1], dict(stop_token_ids=[stop_in, stop_gen]))])
        assert ses.cancelled == set()
    assert torch.equal(got[0][0].cpu(), ids[3][:6]) and torch.equal(got[1][0].cpu(), ids[6][:4]) and torch.equal(got[2][0].cpu(), ids[1][:5])
    # 3. one row: 1 runs, 3 (P = 5) is pending and cancelled - delivered as its prompt alone, and in `cancelled`; 4. the ring of 2 is full
    with lm.open_rolling(12, rows=1, capacity=2, max_prompt_length=5) as ses:
        a = ses.submit(feats[1:2].to(DEV), prompt_ids=prompts[1])
        b = ses.submit(feats[3:4].to(DEV), prompt_ids=prompts[3])
        before = (ses.submitted, ses.unfinished, ses.watermark)
        with pytest.raises(_hip.RgrgHipError, match="capacity 2 feature rows"):
            ses.submit(feats[4:5].to(DEV), prompt_ids=prompts[4])
        assert (ses.submitted, ses.unfinished, ses.watermark) == before
        ses.cancel(b[0])
        got = {}
        _drain(ses, got)
        assert ses.cancelled == {b[0]} and torch.equal(got[b[0]][0].cpu(), prompts[3]) and torch.equal(got[a[0]][0].cpu(), ids[1])
        c = ses.submit(feats[4:5].to(DEV), prompt_ids=prompts[4])          # the session still works, the ring row is reused
        _drain(ses, got)
        assert torch.equal(got[c[0]][0].cpu(), ids[4])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(mixed):
    lm = _lm()
    eng = gpu_model("ragged").engine()
    f = mixed["feats"][:3].to(DEV)
    p3 = torch.randint(0, 50000, (3, 3), generator=torch.Generator().manual_seed(5))

    def refused(ses, call, match, exc=ValueError):
        before = (ses.submitted, ses.unfinished, ses.watermark)
        with pytest.raises(exc, match=match):
            call()
        assert (ses.submitted, ses.unfinished, ses.watermark) == before

    for mp in (8, 9, -1, 1.5):
        with pytest.raises(ValueError, match="max_prompt_length"):
            lm.open_rolling(8, rows=4, max_prompt_length=mp)
    with pytest.raises(ValueError, match="beam session"):
        lm.open_rolling(8, rows=4, num_beams=2, max_prompt_length=3)
    with lm.open_rolling(8, rows=4, num_beams=2) as ses:
        refused(ses, lambda: ses.submit(f[:1], prompt_ids=p3[:1]), "beam session")
        assert ses._dec is not None and eng.lib.rgrg_decoder_roll_submit_prompt(ses._dec, _hip.ptr(f), 1, p3.data_ptr(), 3, 0, 0.0, -1, 0.0, 0, 0,
                                                                               None, 0, None, None) != 0
        assert b"beam session" in eng.lib.rgrg_last_error()
    with lm.open_rolling(8, rows=4, capacity=6) as ses:                       # max_prompt_length = 0
        refused(ses, lambda: ses.submit(f, prompt_ids=p3), "without max_prompt_length")
        assert eng.lib.rgrg_decoder_roll_submit_prompt(ses._dec, _hip.ptr(f), 3, p3.data_ptr(), 3, 0, 0.0, -1, 0.0, 0, 0, None, 0, None, None) != 0
        assert b"without max_prompt_length" in eng.lib.rgrg_last_error()
        assert ses.submit(f) == range(0, 3)
    with lm.open_rolling(8, rows=4, capacity=6, max_prompt_length=4) as ses:
        assert ses.max_prompt_length == 4
        lib, dec = eng.lib, ses._dec
        refused(ses, lambda: ses.submit(f, prompt_ids=torch.zeros((3, 5), dtype=torch.int64)), "1 .. 4 are possible")           # P > max_prompt_length
        refused(ses, lambda: ses.submit(f, prompt_ids=torch.zeros((3, 0), dtype=torch.int64)), "are possible")                 # P = 0
        refused(ses, lambda: ses.submit(f, prompt_ids=p3, max_length=3), "1 .. 2 are possible")                                # P + 1 > the limit
        refused(ses, lambda: ses.submit(f, prompt_ids=p3.to(torch.int32)), "int64")
        refused(ses, lambda: ses.submit(f, prompt_ids=p3.tolist()), "int64")
        refused(ses, lambda: ses.submit(f, prompt_ids=p3[:2]), r"\[m = 3, P\]")
        refused(ses, lambda: ses.submit(f, prompt_ids=p3[None]), r"\[m = 3, P\]")
        bad = p3.clone()
        bad[1, 2] = 50257
        refused(ses, lambda: ses.submit(f, prompt_ids=bad), "token ids in 0 .. 50256")
        bad[1, 2] = -1
        refused(ses, lambda: ses.submit(f, prompt_ids=bad), "token ids in 0 .. 50256")
        # the C entry refuses on its own
        def call(ids, P_, ml):
            return lib.rgrg_decoder_roll_submit_prompt(dec, _hip.ptr(f), 3, ids.data_ptr(), P_, ml, 0.0, -1, 0.0, 0, 0, None, 0, None, None)

        wide = torch.zeros((3, 5), dtype=torch.int64)
        assert call(wide, 5, 0) != 0 and b"a prompt of 5 tokens" in lib.rgrg_last_error()
        assert call(wide, 0, 0) != 0 and call(p3, 3, 3) != 0 and b"a prompt of 3 tokens" in lib.rgrg_last_error()
        assert call(bad, 3, 0) != 0 and b"prompt token id -1" in lib.rgrg_last_error()
        assert call(p3, 3, 9) != 0 and b"max_length" in lib.rgrg_last_error()
        assert (ses.advance(), ses.unfinished, ses.submitted) == (0, 0, 0)
        assert ses.submit(f, prompt_ids=p3, max_length=4) == range(0, 3)       # the session still works: P + 1 = the limit
        ses.advance()
        assert [(q, ids.shape[0]) for q, ids in ses.collect()] == [(0, 4), (1, 4), (2, 4)]
    with eng.open_rolling(8, 4, 6) as ses:
        lib = eng.lib
    dec = eng._decoder
    assert lib.rgrg_decoder_roll_open_prompt(dec, 4, 6, 1, 8, 8, 0, 1.0, 0, 1.0, 0, 1, None) != 0 and b"max_prompt_length 8" in lib.rgrg_last_error()
    assert lib.rgrg_decoder_roll_open_prompt(dec, 4, 6, 1, 8, -1, 0, 1.0, 0, 1.0, 0, 1, None) != 0
    # a ring that does not fit is refused at open, naming its size: 10000 feature rows x 255 slots x 24 layers of fp32 are 478125 MiB
    # (the image key / value ring of the same session is 255 times smaller and fits)
    with pytest.raises(_hip.RgrgHipError, match=r"prompt K/V ring: 10000 feature rows x 255 prompt slots x 24 layers need 478125.0 MiB"):
        eng.open_rolling(256, 4, 10_000, max_prompt_length=255)
    with lm.open_rolling(8, rows=4, capacity=6, max_prompt_length=4) as ses:    # ... and leaves the engine usable
        assert ses.submit(f[:1], prompt_ids=p3[0]) == range(0, 1)


# ------------------------------------------------------------------------------------------------ the report model
def test_report_model_region_prompts():
    import rgrg_amd
    m = gpu_model("ragged")
    B, T = 2, 3
    images = synth.make_images(B, 1234).to(DEV)
    prompts = torch.randint(0, 50000, (B, 29, T), generator=torch.Generator().manual_seed(107))
    with m.open_rolling(7, rows=16, capacity=96, max_prompt_length=3) as ses:
        with pytest.raises(ValueError, match="region_prompts"):
            ses.submit(images, region_prompts=prompts[:1])
        t = ses.submit(images, region_prompts=prompts)
        ses.advance()
        done = dict(ses.collect())
    ids, sel, det, cd = done[t]
    _, sel_g, det_g, cd_g = m.generate(images, max_length=4)
    assert torch.equal(sel, sel_g) and torch.equal(cd, cd_g) and torch.equal(det["top_region_boxes"], det_g["top_region_boxes"])
    _, _, top, cd2 = m.object_detector(images)
    _, feats = m.binary_classifier_region_selection(top, cd2, return_loss=False)
    chosen = prompts.reshape(B * 29, T)[sel.reshape(-1).cpu()]
    with m.language_model.open_rolling(7, rows=16, capacity=96, max_prompt_length=3) as ses:
        got, _ = _play(ses, [(feats, chosen, {})])
    S = int(sel.sum())
    assert ids.shape[0] == S > 0 and ids.shape[1] <= 7 and torch.equal(ids[:, :T].cpu(), chosen)
    for q in range(S):
        row = got[q][0]
        assert torch.equal(ids[q, :row.shape[0]], row) and (ids[q, row.shape[0]:] == PAD).all()
    # nothing selected: the -1 of generate(), at once
    sd0 = dict(synth_sd("ragged"))
    sd0["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m0 = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m0.load_state_dict(sd0)
    m0.to(DEV).eval()
    try:
        with m0.open_rolling(6, rows=16, max_prompt_length=3) as ses:
            t = ses.submit(images[:1], region_prompts=prompts[:1])
            assert ses.collect() == [(t, -1)]
            with pytest.raises(ValueError, match="are possible"):
                ses.submit(images[:1], region_prompts=torch.zeros((1, 29, 4), dtype=torch.int64))
    finally:
        m0.invalidate_engine()
