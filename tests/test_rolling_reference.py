"""GPU-less checks of tests/rolling_reference.py, the numpy model the retire / refill kernel is tested against
(tests/test_gpu_rolling_kernels.py): the model produces what any schedule must produce, within the host loop's step bound; and every
named mutation - a wrong rule a kernel could implement - is told from the rule by the cases the GPU test runs."""
import numpy as np
import pytest

import rolling_reference as M


def _lengths(seed, S, max_length):
    """Natural lengths between 2 (EOS as the first token) and max_length + 3 (cut at max_length without an EOS)."""
    return np.random.default_rng(seed).integers(2, max_length + 4, size=S)


SCHEDULES = [(11, 4, 12), (11, 1, 6), (70, 33, 8), (140, 129, 6), (5, 9, 7), (1, 1, 2), (64, 64, 5), (200, 7, 3), (33, 32, 16)]


@pytest.mark.parametrize("S,R,L", SCHEDULES)
def test_schedule_produces_every_sequence_within_the_step_bound(S, R, L):
    for seed in range(4):
        lengths = _lengths(100 * seed + S, S, L)
        ids, lens, steps, trace, st = M.run_schedule(lengths, R, L)
        want_ids, want_lens = M.expected_ids(lengths, L)
        assert st["shared"][M.UNFINISHED] == 0 and st["shared"][M.NEXT] == S
        assert np.array_equal(ids[:, :L], want_ids) and np.array_equal(lens, want_lens)
        assert (ids[:, L] == M.PAD).all(), "a token behind max_length"
        assert (st["seq"] == -1).all() and (st["tok"] == M.BOS).all() and (st["step"] == 0).all() and (st["pos"] == 0).all()
        assert steps <= M.step_bound(S, R, L)
        # no less than the work and the longest sequence allow
        assert steps >= max(int(want_lens.max()) - 1, -(-int((want_lens - 1).sum()) // R))
        # every sequence is handed out once, in order, and a step's refills go to ascending rows
        handed = [seq for step in trace for _, seq in step]
        assert handed == list(range(S))
        assert all([r for r, _ in step] == sorted(r for r, _ in step) for step in trace)


def test_worst_case_schedule_meets_the_bound_with_little_room():
    """Every sequence runs to max_length: ceil(S / R) * (max_length - 1) steps, one sequence's worth below the bound."""
    S, R, L = 9, 4, 6
    _, lens, steps, _, _ = M.run_schedule([L + 5] * S, R, L)
    assert (lens == L).all() and steps == 3 * (L - 1) == M.step_bound(S, R, L) - (L - 1)


def test_rows_idle_from_the_start_and_lock_step_when_rows_cover_the_sequences():
    ids, lens, steps, trace, _ = M.run_schedule([4, 2, 9], 8, 7)
    assert trace[0] == [(0, 0), (1, 1), (2, 2)] and all(t == [] for t in trace[1:])
    assert steps == 6 and list(lens) == [4, 2, 7]


def _run_case(case, mut=None):
    name, S, R, L, st, arg = case
    st = {k: v.copy() for k, v in st.items()}
    ids, lens = M.sentinel_output(S, L + 1)
    refills = M.roll_step(st, arg, ids, lens, L, mut)
    return st, ids, lens, refills


def _same(a, b):
    return (all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and a[3] == b[3])


# the case of tests/test_gpu_rolling_kernels.py that must tell the mutation from the rule
CATCHES = {"descending_rows": "all_end_fewer_pending", "retire_late": "max_length_without_eos", "eos_not_appended": "eos_first_token",
           "idle_writes": "idle_rows_stay_idle", "next_by_free": "all_end_fewer_pending"}


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_named_mutations_are_rejected_by_the_kernel_cases(mut):
    cases = {c[0]: c for c in M.hook_cases()}
    case = cases[CATCHES[mut]]
    assert not _same(_run_case(case), _run_case(case, mut)), f"{mut} is not told from the rule by {case[0]}"
    caught = [n for n, c in cases.items() if not _same(_run_case(c), _run_case(c, mut))]
    assert CATCHES[mut] in caught


def test_mutations_show_in_what_they_break():
    cases = {c[0]: c for c in M.hook_cases()}
    good, bad = _run_case(cases["all_end_fewer_pending"]), _run_case(cases["all_end_fewer_pending"], "descending_rows")
    assert good[3] == [(0, 5), (1, 6)] and bad[3] == [(4, 5), (3, 6)]
    assert list(good[0]["seq"]) == [5, 6, -1, -1, -1]
    bad = _run_case(cases["all_end_fewer_pending"], "next_by_free")
    assert good[0]["shared"][M.NEXT] == 7 and bad[0]["shared"][M.NEXT] == 10
    good, bad = _run_case(cases["max_length_without_eos"]), _run_case(cases["max_length_without_eos"], "retire_late")
    assert list(good[2][:3]) == [5, -1, 5] and list(bad[2][:3]) == [-1, -1, 5] and bad[0]["seq"][0] == 0
    good, bad = _run_case(cases["eos_first_token"]), _run_case(cases["eos_first_token"], "eos_not_appended")
    assert good[2][0] == 2 and good[1][0, 1] == M.EOS and bad[1][0, 1] == -1   # (visible on the sentinel-filled buffer only)
    good, bad = _run_case(cases["idle_rows_stay_idle"]), _run_case(cases["idle_rows_stay_idle"], "idle_writes")
    assert not np.array_equal(good[1], bad[1]) and list(good[0]["seq"]) == [0, -1, -1, -1, 1]


def test_whole_schedules_reject_the_mutations_too():
    lengths = [3, 9, 2, 5, 9, 4, 2]
    want_ids, want_lens = M.expected_ids(lengths, 6)
    for mut in M.MUTATIONS:
        if mut == "eos_not_appended":   # EOS = PAD: invisible in a PAD-filled output; the kernel case runs on a sentinel-filled one
            continue
        ids, lens, steps, trace, st = M.run_schedule(lengths, 3, 6, mut)
        ok = (np.array_equal(ids[:, :6], want_ids) and (ids[:, 6] == M.PAD).all() and np.array_equal(lens, want_lens)
              and st["shared"][M.NEXT] == len(lengths) and all([r for r, _ in s] == sorted(r for r, _ in s) for s in trace))
        assert not ok, mut
