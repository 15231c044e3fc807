"""GPU-less checks of tests/rolling_sample_reference.py, the contract of rolling-batch sampling in numpy: the result does not depend
on the number of decoder rows and is the lock-step ``sample()``'s; ``top_k = 1`` is the greedy schedule; the n hypotheses of a feature
row read that row's image key / value; and every named mutation - a wrong rule an implementation could follow - is told from the
rule by these checks."""
import numpy as np
import pytest

import rolling_reference as M
import rolling_sample_reference as RS

S, N, L, SEED = 4, 3, 9, 1234
Q = S * N
FILTER = dict(temperature=0.8, top_k=8, top_p=0.9)
ROWS = (1, 3, Q, Q + 5)


@pytest.fixture(scope="module")
def lock():
    ids, lp, lens = RS.lock_step(S, N, L, SEED, **FILTER)
    # something to roll: ragged lengths, one sequence cut at max_length, hypotheses of one feature row that differ
    assert len(set(lens.tolist())) >= 3 and int(lens.max()) == L and int(lens.min()) <= 4, lens.tolist()
    assert any(len({tuple(ids[s * N + j]) for j in range(N)}) > 1 for s in range(S))
    return ids, lp, lens


@pytest.fixture(scope="module")
def rolled():
    return {R: RS.run(S, N, R, L, SEED, **FILTER) for R in ROWS}


def _equal(got, lock):
    ids, lp, lens = got[0], got[1], got[2]
    return np.array_equal(ids, lock[0]) and np.array_equal(lp[:Q], lock[1]) and not lp[Q:].any() and np.array_equal(lens, lock[2])


@pytest.mark.parametrize("R", ROWS)
def test_ids_and_logprobs_do_not_depend_on_the_rows_and_equal_lock_step(lock, rolled, R):
    ids, lp, lens, steps, _ = rolled[R]
    assert np.array_equal(ids, lock[0]) and np.array_equal(lens, lock[2])
    assert np.array_equal(lp[:Q], lock[1]) and not lp[Q:].any()          # the same float64 bits, nothing outside the sequences' rows
    assert (lp <= 0).all() and (lp[:, 0] == 0).all()
    for q in range(Q):
        assert (ids[q, lens[q]:] == M.PAD).all() and (lp[q, lens[q]:] == 0).all()   # (a live log-prob may be 0 too: one kept token)
    work = int((lens - 1).sum())
    assert max(int(lens.max()) - 1, -(-work // R)) <= steps <= M.step_bound(Q, R, L)
    if Q <= R:
        assert steps == int(lens.max()) - 1


def test_top_k_1_is_the_greedy_schedule():
    lengths, toks = RS.greedy_lengths_and_tokens(S, N, L)
    assert len(set(lengths)) >= 2
    for R in ROWS:
        want_ids, want_lens, want_steps, _, _ = M.run_schedule(lengths, R, L, token=lambda s, j: toks[s][j])
        ids, lp, lens, steps, _ = RS.run(S, N, R, L, SEED, top_k=1)
        assert np.array_equal(ids, want_ids[:, :L]) and np.array_equal(lens, want_lens) and steps == want_steps
        # one kept token - or several tied ones - per draw: log-prob -log(ties) <= 0
        assert (lp <= 0).all() and (lp[:, 0] == 0).all()
        other, _, _, _, _ = RS.run(S, N, R, L, SEED + 1, top_k=1)
        assert np.array_equal(other, ids)                                  # no random word enters


def test_a_sequence_reads_the_image_row_of_its_feature_row(rolled):
    for R in ROWS:
        trace = rolled[R][4]
        assert [seq for seq, _ in trace] == list(range(Q))                 # handed out once each, in order
        assert all(feature == seq // N for seq, feature in trace)


# which of the row counts must show a mutation: the first two coincide with the rule where no row is ever refilled (R >= Q)
SHOWS = {"counter_row": (1, 3), "counter_global_step": (1, 3), "counter_off_by_one": ROWS, "lp_at_row": (1, 3), "ukv_mod": ROWS}


@pytest.mark.parametrize("mut", RS.MUTATIONS)
def test_named_mutations_are_rejected(lock, mut):
    got = {R: RS.run(S, N, R, L, SEED, mut=mut, **FILTER) for R in ROWS}
    for R in SHOWS[mut]:
        assert not _equal(got[R], lock), f"{mut} is not told from the rule at R = {R}"
    if mut in ("counter_row", "counter_global_step"):
        # ... and they are what makes a result depend on R: lock step at R >= Q, something else below
        assert _equal(got[Q], lock) and not np.array_equal(got[1][0], got[3][0])
    if mut == "lp_at_row":
        assert all(np.array_equal(got[R][0], lock[0]) for R in ROWS)       # the ids are right: only the log-probs' place is wrong
    if mut == "ukv_mod":
        assert any(feature != seq // N for seq, feature in got[Q][4])
