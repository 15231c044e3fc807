"""The host model of the rolling beam session (tests/rolling_beam_session_reference.py) on the CPU: fed with the oracle's per-region
candidate traces it gives every region ``beam_generate``'s hypotheses under every arrival schedule, all-at-once it IS the schedule
model of rolling beam search (tests/rolling_beam_reference.py), its counts for CASE_1 are the ones worked out by hand from the
regions' iteration counts, and the cases the GPU tests run reject every named defect - which is what makes it a reference for
tests/test_gpu_roll_beam_session.py.

Inputs as tests/test_rolling_beam_reference.py: the first 11 feature rows of tests/test_gpu_rolling.py, the ``ragged`` weights with
``prompt_reference.eos_boosted(sd, 0.98)``, 4 beams, max_length 12."""
import pytest
import torch

import prompt_reference as pr
import rolling_beam_reference as M
import rolling_beam_session_reference as B
from conftest import synth_sd
from oracle import language_model as o_lm
from test_gpu_rolling import BOOST, POOL, POOL_SEED, ROWS

NB, L_MAX, S_ALL = 4, 12, 11


@pytest.fixture(scope="module")
def runs():
    feats = torch.randn((POOL, 1024), generator=torch.Generator().manual_seed(POOL_SEED))[ROWS][:S_ALL].contiguous()
    sd = pr.eos_boosted(synth_sd("ragged"), BOOST)
    out = {}
    for early in (True, False):
        seq, trace = o_lm.beam_generate(sd, feats, L_MAX, NB, early_stopping=early, return_trace=True)
        out[early] = {"seq": seq, "trace": trace, "feats": feats, "sd": sd}
    return out


def _same_as_oracle(ses, seq, regions, keep=1):
    got = B.table(ses.result, regions, keep, pad_to=seq.shape[1])
    want = torch.cat([seq[q * keep:(q + 1) * keep] for q in regions])
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    for q in regions:   # the width of a region alone
        rows = seq[q * keep:(q + 1) * keep]
        used = max(int((r[1:] != B.PAD).sum()) for r in rows) + 2   # BOS, the tokens, one EOS / PAD column
        assert ses.result[q].shape == (keep, min(used, L_MAX))


def check_play(log):
    """What holds for every schedule: an advance launches at most what was asked, nothing when nothing was unfinished, and every
    launched step is counted; collects deliver ascending regions and the watermark never passes what was delivered."""
    unfinished = steps = 0
    for op, val, unf, st, wm in log:
        if op[0] == "advance":
            assert (val == 0) == (unfinished == 0 or op[1] == 0), (op, val, unfinished)
            assert (op[1] is None or val <= op[1]) and st == steps + val
            assert op[1] is not None or unf == 0
        elif op[0] == "collect":
            assert val == sorted(val)
        unfinished, steps = unf, st


@pytest.mark.parametrize("early", (True, False))
@pytest.mark.parametrize("name", sorted(B.CASES))
def test_cases_give_beam_generate(runs, name, early):
    R, nb, cap, L, ops = B.CASES[name]
    ses = B.Session(runs[early]["trace"], nb, R, cap, L, early)
    log = B.play(ses, ops)
    check_play(log)
    assert ses.unfinished == 0 and ses.watermark == ses.submitted
    _same_as_oracle(ses, runs[early]["seq"], list(range(ses.submitted)))
    print(f"BEAMSESSION {name} early={early} launched {[v for o, v, *_ in log if o[0] == 'advance']} steps {ses.steps}")


def test_case_1_counts_by_hand(runs):
    """Iterations 10, 3, 11, 11, 5, 3, 11 on 2 slots (the docstring of CASE_1): the steps every advance launches, what is unfinished
    behind it, what every collect delivers and where the watermark stands."""
    _, iters = M.lockstep_inputs(runs[True]["trace"], S_ALL, NB, L_MAX, True)
    assert iters[:7] == [10, 3, 11, 11, 5, 3, 11]
    R, nb, cap, L, ops = B.CASE_1
    log = B.play(B.Session(runs[True]["trace"], nb, R, cap, L, True), ops)
    assert [(v, u, s) for o, v, u, s, _ in log if o[0] == "advance"] == [
        (1, 1, 1), (3, 1, 4), (6, 0, 10), (0, 0, 10), (3, 2, 13), (1, 2, 14), (10, 0, 24), (3, 2, 27), (11, 0, 38)]
    assert [(v, w) for o, v, _, _, w in log if o[0] == "collect"] == [([], 0), ([0], 1), ([1], 2), ([2, 3], 4), ([5], 4), ([4, 6], 7)]
    assert [v for o, v, *_ in log if o[0] == "refused"] == ["refused"] * 3
    assert [v for o, v, *_ in log if o[0] == "submit"] == [range(0, 1), range(1, 4), range(4, 7)]


@pytest.mark.parametrize("early", (True, False))
@pytest.mark.parametrize("G", (1, 2, 3, S_ALL))
def test_all_at_once_is_the_schedule_model(runs, G, early):
    trace, S = runs[early]["trace"], S_ALL
    ref = M.schedule(trace, S, NB, G, L_MAX, early)
    ses = B.Session(trace, NB, G * NB + 1, S, L_MAX, early)      # (rows that are no multiple of num_beams)
    log = B.play(ses, [("submit", S), ("advance", None), ("collect",)])
    assert ses.G == G and log[1][1] == ses.steps == ref["steps"]
    assert torch.equal(B.table(ses.result, list(range(S)), 1), ref["seq"]) and torch.equal(ref["seq"], runs[early]["seq"])


@pytest.mark.parametrize("m,k,G,cap", [(1, 1, 2, 2), (2, 3, 3, 4), (3, 2, 1, 3), (4, 5, 2, 11)])
def test_streams_of_arrivals(runs, m, k, G, cap):
    """m regions every k steps whenever they fit, collected after every advance, through G slots and a ring of cap."""
    for early in (True, False):
        ses = B.Session(runs[early]["trace"], NB, G * NB, cap, L_MAX, early)
        log = []
        while ses.submitted < S_ALL:
            fit = min(m, S_ALL - ses.submitted, ses.watermark + cap - ses.submitted)
            log += B.play(ses, ([("submit", fit)] if fit > 0 else []) + [("advance", k), ("collect",)])
        log += B.play(ses, [("advance", None), ("collect",)])
        check_play(log)
        _same_as_oracle(ses, runs[early]["seq"], list(range(S_ALL)))


def test_return_sequences_and_length_penalty(runs):
    run = runs[True]
    ref = o_lm.beam_generate(run["sd"], run["feats"], L_MAX, NB, early_stopping=True, num_return_sequences=NB)
    R, nb, cap, L, ops = B.CASE_1
    ses = B.Session(run["trace"], nb, R, cap, L, True, keep=NB)
    B.play(ses, ops)
    _same_as_oracle(ses, ref, list(range(7)), keep=NB)


@pytest.mark.parametrize("mutation", B.MUTATIONS)
def test_named_mutations_are_rejected(runs, mutation):
    """By a case the GPU tests run: the defect raises a violation, accepts a submit that must be refused, or changes a count or a
    hypothesis against the model without it - which is what the GPU test compares the device with."""
    rejected = []
    for name in sorted(B.CASES):
        R, nb, cap, L, ops = B.CASES[name]
        good = B.Session(runs[True]["trace"], nb, R, cap, L, True)
        want = B.play(good, ops)
        try:
            bad = B.Session(runs[True]["trace"], nb, R, cap, L, True, mutate=mutation)
            got = B.play(bad, ops)
            check_play(got)
            assert got == want, "counts differ"
            assert sorted(bad.result) == sorted(good.result) and all(torch.equal(bad.result[q], good.result[q]) for q in good.result), "hypotheses differ"
        except (AssertionError, IndexError, KeyError) as e:
            rejected.append((name, str(e)[:70]))
    print(f"BEAMSESSION mutation {mutation} rejected by {rejected}")
    assert rejected, f"no case rejects {mutation}"
