"""The schedule model of rolling-batch beam search (tests/rolling_beam_reference.py) on the CPU: fed with the oracle's per-region
candidate traces it returns ``beam_generate``'s sequences for every slot count, within the step bounds, and it rejects the named
defects - which is what makes it a reference for tests/test_gpu_rolling_beam.py.

Inputs: the feature rows of tests/test_gpu_rolling.py (ROWS of ``torch.randn((400, 1024), seed 777)``), the ``ragged`` weights with
``prompt_reference.eos_boosted(sd, 0.98)``, 4 beams, max_length 12.  ``test_prefixes_meet_the_conditions`` re-checks, from the one
oracle run per early-stopping setting that all tests here share, what the GPU cases rely on."""
import pytest
import torch

import prompt_reference as pr
import rolling_beam_reference as M
from conftest import synth_sd
from oracle import language_model as o_lm
from test_gpu_rolling import BOOST, POOL, POOL_SEED, ROWS

NB, L_MAX, S_ALL = 4, 12, 40
PREFIXES = (5, 10, 11, 20, 40)   # the region counts of the 4-beam cases of tests/test_gpu_rolling_beam.py
S_MODEL = 11


@pytest.fixture(scope="module")
def runs():
    """``beam_generate`` over the first 40 rows with its trace, early stopping on and off, once."""
    feats = torch.randn((POOL, 1024), generator=torch.Generator().manual_seed(POOL_SEED))[ROWS][:S_ALL].contiguous()
    sd = pr.eos_boosted(synth_sd("ragged"), BOOST)
    out = {}
    for early in (True, False):
        seq, trace = o_lm.beam_generate(sd, feats, L_MAX, NB, early_stopping=early, return_trace=True)
        out[early] = {"seq": seq, "trace": trace, "feats": feats, "sd": sd,
                      "ref11": o_lm.beam_generate(sd, feats[:S_MODEL], L_MAX, NB, early_stopping=early)}   # its own padded width
    return out


def test_prefixes_meet_the_conditions(runs):
    """Under early stopping (the mode the issue measured): at least three distinct leaving iterations, a region undone at max_length
    and a region done within 3 iterations, in every prefix the GPU tests decode with 4 beams.  (Their 17-beam case has its own
    trace: 3 regions through ONE slot, where every region is a refill whatever it does.)"""
    for early in (True, False):
        trace = runs[early]["trace"]
        want, iters = M.lockstep_inputs(trace, S_ALL, NB, L_MAX, early)
        print(f"ROLLBEAM early={early} iterations of the first 20 regions {iters[:20]}")
        for S in PREFIXES:
            it = iters[:S]
            done_early = sorted(set(i for i in it if i < L_MAX - 1))
            print(f"ROLLBEAM early={early} S={S} leaving iterations {done_early} full length {sum(i == L_MAX - 1 for i in it)} work {sum(it)}")
            if early:
                assert len(done_early) >= 3 and any(i == L_MAX - 1 for i in it) and any(i <= 3 for i in it), (S, it)
    # the issue's own figures for the first 20 rows (a dash = the region ran to max_length)
    iters = M.lockstep_inputs(runs[True]["trace"], S_ALL, NB, L_MAX, True)[1]
    assert iters[:20] == [10, 3, 11, 11, 5, 3, 11, 5, 2, 11, 4, 9, 11, 5, 2, 11, 3, 2, 11, 9]


@pytest.mark.parametrize("early", (True, False))
@pytest.mark.parametrize("G", (1, 2, 3, S_MODEL, S_MODEL + 2))
def test_schedule_equals_beam_generate(runs, G, early):
    S = S_MODEL
    run = runs[early]
    trace = [tuple(t[:S] for t in it) for it in run["trace"]]
    ref = run["ref11"]
    res = M.schedule(trace, S, NB, G, L_MAX, early)
    assert torch.equal(res["seq"], ref), (res["seq"].tolist(), ref.tolist())
    want, iters = M.lockstep_inputs(trace, S, NB, L_MAX, early)
    M.check_log(res, S, G, want, iters)
    work, longest = sum(iters), max(iters)
    print(f"ROLLBEAM S={S} G={G} early={early} steps {res['steps']} longest {longest} work {work} bound {M.bound(S, min(G, S), L_MAX)}")
    assert max(longest, -(-work // G)) <= res["steps"] <= M.bound(S, min(G, S), L_MAX)
    if G >= S:
        assert res["steps"] == longest


def test_return_sequences(runs):
    S, early = S_MODEL, True
    run = runs[early]
    trace = [tuple(t[:S] for t in it) for it in run["trace"]]
    ref = o_lm.beam_generate(run["sd"], run["feats"][:S], L_MAX, NB, early_stopping=early, num_return_sequences=NB)
    assert torch.equal(M.schedule(trace, S, NB, 2, L_MAX, early, keep=NB)["seq"], ref)


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_named_mutations_are_rejected(runs, mutation):
    S = S_MODEL
    rejected = []
    for early in (True, False):
        run = runs[early]
        trace = [tuple(t[:S] for t in it) for it in run["trace"]]
        ref = run["ref11"]
        want, iters = M.lockstep_inputs(trace, S, NB, L_MAX, early)
        for G in (1, 2, 3):
            try:
                res = M.schedule(trace, S, NB, G, L_MAX, early, mutate=mutation)
                assert torch.equal(res["seq"], ref), "sequences differ"
                M.check_log(res, S, G, want, iters)
            except (AssertionError, IndexError) as e:
                rejected.append((early, G, str(e)[:60]))
    print(f"ROLLBEAM mutation {mutation} rejected by {len(rejected)} of 6 cases: {rejected[:2]}")
    assert rejected, f"no case rejects {mutation}"
