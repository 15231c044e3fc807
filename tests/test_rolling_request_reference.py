"""The numpy model of a rolling session's requests (tests/rolling_request_reference.py): the schedules the GPU tests run deliver what
every request asks for, the step bound holds under each of them, and each named mutation is rejected by one of them.  CPU only."""
import os
import re

import numpy as np
import pytest

import rolling_request_reference as Q
import rolling_session_reference as S
from conftest import REPO
from rgrg_amd import _hip

EOS = PAD = Q.EOS
L12 = S.LENGTHS_12
NEW_ENTRIES = ("rgrg_decoder_roll_submit_req", "rgrg_decoder_roll_cancel", "rgrg_debug_roll_session_step_req", "rgrg_debug_roll_sample_req")


def _requests(ops):
    """{sequence: request keywords} of the submits of ``ops`` that go through (n = 1)."""
    out, q = {}, 0
    for op in ops:
        if op[0] == "submit":
            for _ in range(op[1]):
                out[q] = op[2] if len(op) > 2 else {}
                q += 1
    return out


def _check(s, ops, lengths, cut=None, seed=0):
    """Every submitted sequence was delivered once with the row its request asks for; no ring row was written for another sequence."""
    reqs, cut = _requests(ops), cut or {}
    assert not s.violations and s.unfinished == 0 and s.watermark == s.S == len(reqs) and sorted(s.results) == list(range(s.S))
    assert s.cancelled == set(cut)
    first, q = {}, 0
    for op in ops:   # the first sequence of the submit a sequence came with
        if op[0] == "submit":
            for i in range(op[1]):
                first[q + i] = q
            q += op[1]
    for q, kw in reqs.items():
        own = "seed" in kw
        want = Q.expected_row(lengths[q], kw.get("max_length", s.L), s.L, kw["seed"] if own else seed, q - first[q] if own else q,
                              kw.get("stop", ()), cut.get(q))
        assert np.array_equal(s.results[q], want), (q, s.results[q], want)


@pytest.mark.parametrize("name", sorted(Q.LIMITS_OPS))
def test_limits_per_submit(name):
    s, log = Q.play(L12, 4, 6, 1, 12, Q.LIMITS_OPS[name])
    _check(s, Q.LIMITS_OPS[name], L12)
    assert all(isinstance(e, str) for op, e in zip(Q.LIMITS_OPS[name], log) if op[0] == "refused")
    # a limit decides: sequence 0 (natural length 12) ends at its submit's limit without an EOS
    ml = _requests(Q.LIMITS_OPS[name])[0]["max_length"]
    assert int((s.results[0][1:] != PAD).sum()) == ml - 1 and EOS not in s.results[0][1:ml].tolist()      # (BOS, EOS and PAD are one id)


def test_cancel_schedule():
    s, log = Q.play(L12, 4, 8, 1, 12, Q.CANCEL_OPS)
    _check(s, Q.CANCEL_OPS, L12, cut=Q.CANCEL_CUT)
    assert s.cancelled == {0, 6} and 1 not in s.cancelled
    assert all(isinstance(e, str) for op, e in zip(Q.CANCEL_OPS, log) if op[0] == "bad_cancel")
    # the step that cuts 0 hands its row (row 0) to the pending sequence 6 in the same pass: the refill list of that step
    step3 = s.trace[2 + 2]            # two submits' hand-outs and two steps lie in front
    assert (0, 6) in step3
    # the collect behind that step delivers the cut 0 together with 1, 2 and 5, and the watermark moves to 3
    assert log[6] == [0, 1, 2, 5] and log[9] == [6]


def test_stop_tokens_end_a_sequence_with_the_stop_token_last():
    stop = Q.draw_token(0, 3, 2)       # the second generated token of sequence 3
    ops = [("submit", 3, {}), ("advance", 1), ("submit", 2, dict(stop=[5, 7, stop])), ("advance", None), ("collect",), ("submit", 2, dict(stop=[stop]))]
    s, _ = Q.play(L12, 4, 8, 1, 12, ops)
    _check(s, ops, L12)
    assert s.results[3][:4].tolist() == [Q.BOS, Q.draw_token(0, 3, 1), stop, PAD]
    assert all(stop not in s.results[q].tolist() for q in range(7) if q != 3)


def test_a_seeded_submit_draws_what_a_session_of_its_own_draws():
    """The counter rule: under seed s, sequence q of a submit that starts at q0 draws row q - q0."""
    ops = [("submit", 3, {}), ("advance", 2), ("submit", 3, dict(seed=77, max_length=8)), ("advance", 3), ("collect",), ("submit", 2, dict(seed=5))]
    s, _ = Q.play(L12, 4, 8, 1, 12, ops, seed=1234)
    _check(s, ops, L12, seed=1234)
    alone, _ = Q.play(L12[3:6], 4, 8, 1, 8, [("submit", 3, {})], seed=77)
    for i in range(3):
        assert np.array_equal(s.results[3 + i][:8], alone.results[i]) and (s.results[3 + i][8:] == PAD).all()
    assert not np.array_equal(s.results[0], Q.play(L12[:3], 4, 8, 1, 12, [("submit", 3, {})], seed=77)[0].results[0])


SCHEDULES = [("limits_case_1", Q.LIMITS_OPS["case_1"], 6, None), ("limits_idle", Q.LIMITS_OPS["idle_and_reuse"], 6, None),
             ("cancel", Q.CANCEL_OPS, 8, Q.CANCEL_CUT)]


@pytest.mark.parametrize("name,ops,C,cut", SCHEDULES)
def test_the_step_bound_holds(name, ops, C, cut):
    """advance(None) is bounded by the session's max_length over what is unfinished: requests only shorten sequences, a cut frees its
    row, so no schedule may need more - checked at every advance(None) of the schedules and for the whole run."""
    s = Q.Session(L12, 4, C, 1, 12)
    for op in ops:
        if op[0] == "submit":
            s.submit(op[1], **op[2])
        elif op[0] == "cancel":
            s.cancel(op[1])
        elif op[0] == "advance":
            bound = s.bound()
            launched = s.advance(op[1])
            assert launched <= bound and (op[1] is not None or s.unfinished == 0)
        elif op[0] == "collect":
            s.collect()
    bound = s.bound()
    assert s.advance(None) <= bound and s.unfinished == 0
    assert s.device_steps <= S.M.step_bound(s.S, 4, 12)


def _mutant_fails(mut):
    """-> the names of the GPU tests' cases that tell the mutation from the rule."""
    caught = []
    for name, ops, C, cut in SCHEDULES:
        s, _ = Q.play(L12, 4, C, 1, 12, ops, mut)
        try:
            _check(s, ops, L12, cut=cut)
        except AssertionError:
            caught.append(name)
    stop = Q.draw_token(0, 3, 2)
    ops = [("submit", 3, {}), ("advance", 1), ("submit", 2, dict(stop=[5, 7, stop])), ("advance", None), ("collect",)]
    s, _ = Q.play(L12, 4, 8, 1, 12, ops, mut)
    try:
        _check(s, ops, L12)
    except AssertionError:
        caught.append("stop")
    ops = [("submit", 3, {}), ("advance", 2), ("submit", 3, dict(seed=77, max_length=8))]
    s, _ = Q.play(L12, 4, 8, 1, 12, ops, mut, seed=1234)
    try:
        _check(s, ops, L12, seed=1234)
    except AssertionError:
        caught.append("seed")
    for R in (5, 260):
        for case in Q.hook_cases(R):
            name, C, n, S_before, submit, handout, retire, R_, L, st, arg, ring, ended = case
            outs = []
            for m in (None, mut):
                st2 = {k: v.copy() for k, v in st.items()}
                ids, lens = np.full((C, L + 1), -1, dtype=np.int64), np.full(C, -99, dtype=np.int32)
                for q, ln in ended.items():
                    lens[q % C] = ln
                rf = Q.session_step_req(st2, arg, ids, lens, None, C, n, S_before, submit, handout, retire, L, ring, m)
                outs.append((st2, ids, lens, rf))
            (a, ia, la, ra), (b, ib, lb, rb) = outs
            if not (all(np.array_equal(a[k], b[k]) for k in a) and np.array_equal(ia, ib) and np.array_equal(la, lb) and ra == rb):
                caught.append(f"hook_{name}_{R}")
    return caught


@pytest.mark.parametrize("mut", Q.MUTATIONS)
def test_every_mutation_is_rejected_by_a_case_the_gpu_tests_run(mut):
    caught = _mutant_fails(mut)
    print(f"REQUESTS mutation {mut}: rejected by {caught}")
    assert caught, mut
    want = {"limit_from_session": "limits_case_1", "stop_not_appended": "stop", "cancel_appends": "cancel", "cancelled_pending_lost": "cancel",
            "counter_row_q": "seed"}[mut]
    assert want in caught
    if mut != "counter_row_q":      # the retire pass alone shows it too, in both sizes of the kernel test
        assert any(c.startswith("hook_") and c.endswith("_5") for c in caught) and any(c.endswith("_260") for c in caught)


def test_hook_cases_cover_what_they_name():
    for R in (5, 260):
        cases = {c[0]: c for c in Q.hook_cases(R)}
        assert sorted(cases) == ["cancel_three_ways", "fourth_stop_id", "limits_mixed", "stop_beside_eos"]
        for name, C, n, S_before, submit, handout, retire, R_, L, st, arg, ring, ended in cases.values():
            assert R_ == R == st["seq"].shape[0] == arg.shape[0] and ring.shape == (C,) and ring.dtype.itemsize == 40
            assert int(st["seq"].max()) < S_before <= C
            lens = np.full(C, -99, dtype=np.int32)
            for q, ln in ended.items():
                lens[q % C] = ln
            ids = np.full((C, L + 1), -1, dtype=np.int64)
            st2 = {k: v.copy() for k, v in st.items()}
            _, rf = Q.session_step_req(st2, arg, ids, lens, None, C, n, S_before, submit, handout, retire, L, ring)
            F = R - 5
            assert (st2["seq"][:F] == np.arange(F)).all() and (lens[:F] == -99).all()     # the rows in front go on
            if name == "limits_mixed":
                assert lens[F:F + 4].tolist() == [2, L - 1, -99, 4] and st2["len"][F + 2] == L - 1
            elif name == "stop_beside_eos":
                assert lens[F:F + 4].tolist() == [4, 3, -99, -99] and ids[F + 1, 2] == 4242 and ids[F + 2, 4] == 4242
            elif name == "fourth_stop_id":
                assert lens[F:F + 5].tolist() == [-99, 3, -99, 2, 6] and ids[F + 1, 2] == 31 and ids[F + 3, 1] == 50000
            else:
                assert lens[F:F + 7].tolist() == [5, -4, -1, 7, -99, -99, -99] and (ids[F + 1] == -1).all() and (ids[F + 2] == -1).all()
                assert [(r - F, q - F) for r, q, _ in rf] == [(0, 5), (1, 6)] and st2["len"][F] == 1    # 5 is flagged and NOT cut in this pass


def test_ring_entry_layout_is_the_headers():
    assert [(n, Q.REQ_DTYPE.fields[n][1]) for n in Q.REQ_DTYPE.names] == [("seed", 0), ("inv_T", 8), ("top_k", 12), ("top_p", 16),
                                                                         ("max_length", 20), ("q0", 24), ("stop", 28), ("flags", 36)]
    header = open(os.path.join(REPO, "include", "rgrg_hip.h")).read()
    assert "0 uint64 seed | 8 float 1 / temperature | 12 int32 top_k | 16 float top_p | 20 int32 max_length | 24 int32 q0 |" in header
    assert "28 uint16 stop[4] (65535 = unused) | 36 uint32 flags (bit 0: cancelled)" in header


def test_new_entries_in_header_binding_and_library():
    header = open(os.path.join(REPO, "include", "rgrg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load()
    for name in NEW_ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_hip.SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.SIGNATURES[name][1]
    assert _hip.ABI_VERSION == 28 and lib.rgrg_abi_version() == 28      # new entries change no signature
    for word in ("Counter rule", "Cancel rule", "Length word"):
        assert word in header
