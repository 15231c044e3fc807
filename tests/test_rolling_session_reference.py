"""The numpy model of a rolling session (tests/rolling_session_reference.py) against the one-shot model it is built on
(tests/rolling_reference.py), and the named mutations against the cases the GPU tests run.  No GPU."""
import numpy as np
import pytest

import rolling_reference as M
import rolling_session_reference as S


@pytest.mark.parametrize("case", S.schedule_cases(), ids=lambda c: c[0])
def test_every_schedule_delivers_expected_ids(case):
    name, lengths, R, C, n, L, ops = case
    s, log = S.play(lengths, R, C, n, L, ops)
    total = sum(op[1] for op in ops if op[0] in ("submit", "stream")) * n
    assert s.violations == []
    assert S.correct(s, total), (name, sorted(s.results))
    assert s.watermark == total and s.unfinished == 0 and s.drained
    for op, entry in zip(ops, log):
        if op[0] == "refused":
            assert entry and "capacity" in entry and "room" in entry, (name, op, entry)


def test_all_at_once_equals_run_schedule():
    for lengths, R, L in ((S.LENGTHS_12, 4, 12), (S._ragged(150, 5), 70, 9), (S._ragged(9, 6), 16, 10)):
        total = len(lengths)
        s, _ = S.play(lengths, R, 2 * total, 1, L, [("submit", total)])
        ids, lens, steps, trace, st = M.run_schedule(lengths, R, L)
        assert S.correct(s, total)
        assert s.device_steps == steps
        # the same hand-outs step for step; the session's host loop runs idle steps behind the last retirement (the late poll)
        assert s.trace[:len(trace)] == trace and all(not t for t in s.trace[len(trace):]) and len(s.trace) >= len(trace)
        assert np.array_equal(s.ids[:total, :L], ids[:, :L]) and np.array_equal(s.lens[:total], lens)
        assert (s.ids[:, L] == -1).all()            # the spare column: no sequence ran past max_length


def test_case_1_is_the_sequence_of_calls_the_gpu_test_makes():
    s, log = S.play(S.LENGTHS_12, 4, 6, 1, 12, S.CASE_1_OPS)
    assert log[0] == range(0, 5) and isinstance(log[1], str)          # 5 in a ring of 6, 3 more refused
    assert log[2] == 2 and log[3] == [1, 2]                            # two steps: lengths 3 and 2 have ended, 0 is running
    assert isinstance(log[4], str) and log[5] == range(5, 6)           # the watermark is still 0: 2 refused, 1 fits
    assert sorted(log[7]) == [0, 3, 4, 5]
    assert log[8] == range(6, 11)                                      # ring rows 0 .. 4 again
    assert s.watermark == 11 and S.correct(s, 11)


def test_handout_only_pass_leaves_active_rows_alone():
    for case in S.hook_cases():
        name, C, n, S_before, submit, handout, retire, R, L, st0, arg = case
        if not handout or retire:
            continue
        st = {k: v.copy() for k, v in st0.items()}
        ids, lens = M.sentinel_output(C, L + 1)
        a, b = S.session_step(st, arg, ids, lens, None, C, n, S_before, submit, handout, retire, L)
        active = st0["seq"] >= 0
        for k in S.ROW_KEYS:
            assert np.array_equal(st[k][active], st0[k][active]), (name, k)
        assert (ids == -1).all() and (lens == -1).all() and b == []
        assert st["shared"][S.STEPS] == st0["shared"][S.STEPS]
        assert [q for _, q, _ in a] == list(range(int(st0["shared"][S.NEXT]), int(st["shared"][S.NEXT])))


def test_idle_session_launches_nothing():
    s = S.Session(S.LENGTHS_12, 4, 8, 1, 12)
    assert s.advance(None) == 0 and s.advance(5) == 0
    s.submit(3)
    s.advance(None)
    steps = s.device_steps
    assert s.drained and s.advance(None) == 0 and s.advance(7) == 0 and s.device_steps == steps
    s.submit(2)
    assert not s.drained and s.advance(None) > 0 and s.collect() == [0, 1, 2, 3, 4] and S.correct(s, 5)


def test_release_refuses_an_unfinished_sequence():
    s = S.Session(S.LENGTHS_12, 4, 6, 1, 12)
    s.submit(5)
    s.advance(2)
    with pytest.raises(ValueError, match="has not finished"):
        s.release(2)            # 0 is still running
    assert s.collect() == [1, 2] and s.watermark == 0


def _rejected_by_schedules(mut):
    hits = []
    for name, lengths, R, C, n, L, ops in S.schedule_cases():
        total = sum(op[1] for op in ops if op[0] in ("submit", "stream")) * n
        try:
            s, log = S.play(lengths, R, C, n, L, ops, mut)
            ok = S.correct(s, total) and s.watermark == total and s.unfinished == 0
            ok = ok and all(bool(e) for op, e in zip(ops, log) if op[0] == "refused")
            ref, _ = S.play(lengths, R, C, n, L, ops)
            ok = ok and s.launched == ref.launched and s.device_steps == ref.device_steps
        except (S.RingFull, ValueError, AssertionError, IndexError):
            ok = False
        if not ok:
            hits.append(name)
    return hits


def _rejected_by_hook_cases(mut):
    hits = []
    for name, C, n, S_before, submit, handout, retire, R, L, st0, arg in S.hook_cases():
        outs = []
        for m in (None, mut):
            st = {k: v.copy() for k, v in st0.items()}
            ids, lens = M.sentinel_output(max(C, S_before + submit + 1), L + 1)   # rows behind C show a slot without the modulo
            refills = S.session_step(st, arg, ids, lens, None, C, n, S_before, submit, handout, retire, L, m)
            outs.append((st, ids, lens, refills))
        same = all(np.array_equal(outs[0][0][k], outs[1][0][k]) for k in outs[0][0]) and np.array_equal(outs[0][1], outs[1][1]) and \
            np.array_equal(outs[0][2], outs[1][2]) and outs[0][3] == outs[1][3]
        if not same:
            hits.append(name)
    return hits


@pytest.mark.parametrize("mut", S.MUTATIONS)
def test_every_mutation_is_rejected_by_a_case_the_gpu_tests_run(mut):
    end_to_end, kernel = _rejected_by_schedules(mut), _rejected_by_hook_cases(mut)
    print(f"SESSIONMUT {mut}: end to end {end_to_end}, kernel level {kernel}")
    assert end_to_end or kernel, mut
    if mut in ("release_past_unfinished", "unfinished_not_raised"):
        assert end_to_end          # the host's rules show end to end only
    else:
        assert kernel, mut         # a device rule must show at the kernel level too
