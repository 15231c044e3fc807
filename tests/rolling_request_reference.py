"""Numpy model of the requests of a rolling session (rgrg_amd/csrc/decoder_roll.hip) on top of
``rolling_session_reference``, which is imported and used as it is: every submit carries its own max_length, stop tokens and - in a
sampling session - its own seed, and a submitted sequence can be cancelled.  No GPU, no torch.

Device side, on plain arrays (what rgrg_debug_roll_session_step_req runs; ``session_step_req`` is its model):
  the REQUEST RING ``req`` [C] (REQ_DTYPE: the 40-byte entries of include/rgrg_hip.h), entry q % C for sequence q
  retire_pass_req  roll_step with the limit and the stop tokens of the row's sequence; a sequence whose cancel flag is set is CUT: the
                   token is not appended, lens = -len, the row is free in the same pass.  Only rows that hold a sequence on entry look at
                   the flag, so a cancelled pending sequence takes a row and is cut in that row's next pass, as BOS alone.
  the hand-out-only pass and the submit-init are those of rolling_session_reference (the ring is the caller's in the hook).
The length word: > 0 ended, < 0 cut (minus the tokens kept), 0 not finished.

Host side, ``Session``: rolling_session_reference.Session with ``submit(m, max_length=, stop=, seed=)``, ``cancel(qs)`` and
``cancelled``.  A cancel takes effect in the next retire pass that runs (it is enqueued in front of the next step).  In a sampling
session the "arg-max" of a row is a function of the seed and the Philox counter (q - q0, len - 1) of the draw, so that a wrong
counter row shows in the tokens.

MUTATIONS are wrong rules an implementation could have; tests/test_rolling_request_reference.py shows that the cases the GPU tests
run reject each of them.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

import rolling_reference as M
import rolling_session_reference as S

BOS = EOS = PAD = M.BOS
NEXT, UNFINISHED, REFILLS, STEPS = M.NEXT, M.UNFINISHED, M.REFILLS, M.STEPS
MUTATIONS = ("limit_from_session", "stop_not_appended", "cancel_appends", "cancelled_pending_lost", "counter_row_q")
NO_STOP, CANCEL = 0xFFFF, 1
REQ_DTYPE = np.dtype([("seed", "<u8"), ("inv_T", "<f4"), ("top_k", "<i4"), ("top_p", "<f4"), ("max_length", "<i4"), ("q0", "<i4"),
                      ("stop", "<u2", (4,)), ("flags", "<u4")])
assert REQ_DTYPE.itemsize == 40


def new_ring(C: int, max_length: int, seed: int = 0, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> np.ndarray:
    """What rgrg_decoder_roll_submit writes for every sequence: the session's values, q0 = 0, no stop token, not cancelled."""
    ring = np.zeros(C, dtype=REQ_DTYPE)
    ring["seed"], ring["inv_T"], ring["top_k"], ring["top_p"] = seed, np.float32(1.0) / np.float32(temperature), top_k, top_p
    ring["max_length"], ring["stop"] = max_length, NO_STOP
    return ring


def set_request(ring, q: int, *, max_length=None, stop=(), seed=None, q0=0, temperature=None, top_k=None, top_p=None, cancel=False):
    e = ring[q % ring.shape[0]:q % ring.shape[0] + 1]
    if max_length is not None:
        e["max_length"] = max_length
    e["stop"][0, :] = NO_STOP
    e["stop"][0, :len(stop)] = list(stop)
    if seed is not None:
        e["seed"], e["q0"] = seed, q0
    if temperature is not None:
        e["inv_T"] = np.float32(1.0) / np.float32(temperature)
    if top_k is not None:
        e["top_k"] = top_k
    if top_p is not None:
        e["top_p"] = top_p
    e["flags"] = CANCEL if cancel else 0


def counter_row(q: int, q0: int, mut: Optional[str] = None) -> int:
    """The Philox counter row of sequence q's draws."""
    return q if mut == "counter_row_q" else q - q0


def roll_step_req(st: Dict[str, np.ndarray], arg: np.ndarray, ids: np.ndarray, lens: np.ndarray, C: int, S_: int, max_length: int,
                  req: np.ndarray, mut: Optional[str] = None, writes=None) -> List[Tuple[int, int]]:
    """One retire-and-refill step with the request ring IN PLACE on st / ids [C][..] / lens [C] -> the refill list [(row, sequence)]."""
    assert mut is None or mut in MUTATIONS, mut
    writes = [] if writes is None else writes
    R = st["seq"].shape[0]
    nxt = int(st["shared"][NEXT])
    free, any_active = [], False
    for r in range(R):
        seq = int(st["seq"][r])
        if seq < 0:
            free.append(r)
            continue
        any_active = True
        slot = seq % C
        e = req[slot]
        tok, ln = int(arg[r]), int(st["len"][r])
        limit = max_length if mut == "limit_from_session" else min(int(e["max_length"]), max_length)
        stop_hit = any(int(t) != NO_STOP and int(t) == tok for t in e["stop"])
        writes.append((seq, slot))
        if int(e["flags"]) & CANCEL:
            if mut == "cancel_appends":
                ids[slot, ln] = tok
                ln += 1
            if not (mut == "cancelled_pending_lost" and ln == 1):
                lens[slot] = -ln
            free.append(r)
            continue
        if not (mut == "stop_not_appended" and stop_hit):
            ids[slot, ln] = tok
            ln += 1
        if tok == EOS or stop_hit or ln >= limit:
            lens[slot] = ln
            free.append(r)
        else:
            st["len"][r], st["tok"][r], st["pos"][r], st["step"][r] = ln, tok, ln - 1, ln - 1
    given = min(len(free), S_ - nxt)
    refills = []
    for k, r in enumerate(free):
        seq = nxt + k if k < given else -1
        st["seq"][r], st["len"][r] = seq, 1 if seq >= 0 else 0
        st["tok"][r], st["pos"][r], st["step"][r] = BOS, 0, 0
        if seq >= 0:
            refills.append((r, seq))
    nxt += given
    st["shared"][NEXT] = nxt
    st["shared"][REFILLS] = given
    st["shared"][UNFINISHED] = (S_ - nxt) + int((st["seq"] >= 0).sum())
    st["shared"][STEPS] += 1 if any_active else 0
    return refills


def session_step_req(st, arg, ids, lens, lp, C, n, S_before, submit, handout, retire, max_length, req, mut=None):
    """rgrg_debug_roll_session_step_req IN PLACE -> the refills of the hand-out pass and of the retire pass, each (row, sequence, ukv
    ring row).  req None: rolling_session_reference.session_step."""
    if req is None:
        return S.session_step(st, arg, ids, lens, lp, C, n, S_before, submit, handout, retire, max_length)
    S_ = S.submit_init(st, ids, lens, lp, C, S_before, submit, max_length) if submit else S_before
    a = S.handout_pass(st, arg, ids, lens, C, S_, max_length) if handout else []
    b = roll_step_req(st, arg, ids, lens, C, S_, max_length, req, mut) if retire else []
    tag = lambda rf: [(r, q, S.ukv_row(q, n, C)) for r, q in rf]   # noqa: E731
    return tag(a), tag(b)


# ------------------------------------------------------------------------------------------------ the host
def draw_token(seed: int, row: int, col: int) -> int:
    """The stand-in for a draw under (seed; counter row, column): never EOS, different for every triple the tests use."""
    return 1000 + 997 * (seed % 41) + 7 * row + col


class Session(S.Session):
    """rolling_session_reference.Session with requests.  ``lengths[q]`` is the natural length of sequence q (EOS at that length); the
    token of a row that holds q with len tokens is draw_token(seed, counter row of q, len), so a greedy session (seed 0, q0 0) has
    rolling_session_reference's default tokens shifted by nothing but the constant."""

    def __init__(self, lengths, R: int, C: int, n: int, max_length: int, mut: Optional[str] = None, seed: int = 0):
        assert mut is None or mut in MUTATIONS, mut
        super().__init__(lengths, R, C, n, max_length, None)
        self.rmut = mut
        self.seed = seed
        self.req = new_ring(C, max_length, seed)
        self.ids[:], self.lens[:] = -1, 0     # (the length word is signed here: 0, not -1, is "not finished")
        self.cancelled = set()

    def submit(self, m: int, max_length: Optional[int] = None, stop=(), seed: Optional[int] = None) -> range:
        if max_length is not None and not 2 <= max_length <= self.L:
            raise ValueError(f"max_length {max_length}, 2 .. {self.L} are possible")
        if len(stop) > 4:
            raise ValueError(f"{len(stop)} stop token ids, up to 4 are possible")
        count, q0 = m * self.n, self.S
        if q0 + count > self.watermark + self.C:
            raise S.RingFull(f"capacity {self.C // self.n} feature rows, room for {(self.watermark + self.C - q0) // self.n}")
        for q in range(q0, q0 + count):
            set_request(self.req, q, max_length=self.L if max_length is None else max_length, stop=stop,
                        seed=self.seed if seed is None else seed, q0=0 if seed is None else q0)
        return super().submit(m)

    def cancel(self, qs) -> None:
        qs = [qs] if isinstance(qs, int) else list(qs)
        for q in qs:
            if not self.watermark <= q < self.S:
                raise ValueError(f"sequence {q}, {self.watermark} .. {self.S - 1} can be cancelled")
        for q in qs:
            self.req["flags"][q % self.C] |= CANCEL

    def _arg(self) -> np.ndarray:
        arg = np.zeros(self.R, dtype=np.int32)
        for r in range(self.R):
            s, ln = int(self.st["seq"][r]), int(self.st["len"][r])
            if 0 <= s < len(self.lengths):
                e = self.req[s % self.C]
                arg[r] = EOS if ln + 1 == int(self.lengths[s]) else draw_token(int(e["seed"]), counter_row(s, int(e["q0"]), self.rmut), ln)
        return arg

    def advance(self, steps: Optional[int] = None) -> int:
        limit = self.bound() if steps is None else steps
        launched = 0
        if not self.drained and limit > 0:
            polls, seen = 0, [1, 1]
            for t in range(limit):
                writes: List[Tuple[int, int]] = []
                refills = roll_step_req(self.st, self._arg(), self.ids, self.lens, self.C, self.S, self.L, self.req, self.rmut, writes)
                self._check_writes(writes)
                self._check_refills(refills)
                self.trace.append(refills)
                launched += 1
                if (t & 15) == 15 and t + 1 < limit:
                    if polls > 0 and seen[(polls - 1) & 1] == 0:
                        break
                    seen[polls & 1] = int(self.st["shared"][UNFINISHED])
                    polls += 1
        if launched > 0 or not self.drained:
            self.unfinished = int(self.st["shared"][UNFINISHED])
            self.drained = self.unfinished == 0
            self.h_len = self.lens.astype(np.int32).copy()
        self.launched += launched
        return launched

    def finished(self) -> List[int]:
        return [q for q in range(self.watermark, self.S) if self.h_len[q % self.C] != 0]

    def collect(self) -> List[int]:
        new = [q for q in self.finished() if q not in self.collected]
        for q in new:
            k = int(self.h_len[q % self.C])
            row = np.full(self.L, PAD, dtype=np.int64)
            row[:abs(k)] = self.ids[q % self.C, :abs(k)]
            self.results[q] = row
            self.collected.add(q)
            self.delivered.add(q)
            if k < 0:
                self.cancelled.add(q)
        wm = self.watermark
        while wm in self.collected:
            wm += 1
        self.collected = {q for q in self.collected if q >= wm}
        self.release(wm)
        return new


def expected_row(length: int, limit: int, max_length: int, seed: int, row: int, stop=(), cut: Optional[int] = None) -> np.ndarray:
    """What any schedule must deliver for a sequence of natural length ``length`` under its request: the draws of (seed, row), ended by
    EOS, by the first stop token or at ``limit`` tokens, or - cut - its first ``cut`` tokens."""
    out = np.full(max_length, PAD, dtype=np.int64)
    out[0] = BOS
    for j in range(1, min(length, limit)):
        out[j] = EOS if j == length - 1 else draw_token(seed, row, j)
        if int(out[j]) in stop:
            break
    if cut is not None:
        out[cut:] = PAD
    return out


def play(lengths, R, C, n, max_length, ops, mut=None, seed=0):
    """Runs ``ops`` - ("submit", m, dict of request keywords) / ("refused", m, dict) / ("cancel", qs) / ("bad_cancel", qs) /
    ("advance", steps or None) / ("collect",) - and drains, collecting, at the end -> (session, log)."""
    s = Session(lengths, R, C, n, max_length, mut, seed)
    log = []
    for op in ops:
        before = (s.S, s.unfinished, s.watermark)
        if op[0] == "submit":
            log.append(s.submit(op[1], **(op[2] if len(op) > 2 else {})))
        elif op[0] in ("refused", "bad_cancel"):
            try:
                s.submit(op[1], **op[2]) if op[0] == "refused" else s.cancel(op[1])
                log.append(False)
            except (ValueError, S.RingFull) as e:
                log.append(str(e))
            assert (s.S, s.unfinished, s.watermark) == before
        elif op[0] == "cancel":
            log.append(s.cancel(op[1]))
        elif op[0] == "advance":
            log.append(s.advance(op[1]))
        else:
            log.append(s.collect())
    s.advance(None)
    log.append(s.collect())
    return s, log


# ------------------------------------------------------------------------------------------------ what the GPU tests run
# The end-to-end schedules of tests/test_gpu_roll_requests.py: R = 4, C = 6 sequences, L = 12, the natural lengths of the oracle's first
# 11 feature rows (rolling_session_reference.LENGTHS_12 = [12, 3, 2, 12, 7, 2, 12, 5, 2, 12, 3]).
# limits: the arrivals of two of rolling_session_reference's schedule cases - CASE_1 (join, refuse, wrap) and idle_and_reuse - with a
# limit per submit.
LIMITS_OPS = {
    "case_1": [("submit", 5, dict(max_length=6)), ("refused", 3, dict(max_length=8)), ("advance", 2), ("collect",), ("refused", 2, {}),
               ("submit", 1, dict(max_length=8)), ("advance", None), ("collect",), ("submit", 5, {}), ("advance", None), ("collect",)],
    "idle_and_reuse": [("submit", 3, dict(max_length=8)), ("advance", None), ("collect",), ("advance", None),
                       ("submit", 2, dict(max_length=6)), ("advance", 1), ("submit", 2, {})],
}
# cancel (C = 8): 0 .. 4 submitted on 4 rows (4 pending); two steps (2, then 1 have ended, 4 took row 2, row 1 idles, rows 0 and 3 hold 0
# and 3 with 3 tokens); 5 and 6 arrive - 5 takes row 1, 6 is pending; then cancel 0 (running: cut at 3 tokens), 6 (pending: BOS alone) and
# 1 (ended: intact).  The next step cuts 0 and ends 5, and 6 takes row 0 in the same pass; the step after cuts 6.
CANCEL_OPS = [("submit", 5, {}), ("advance", 2), ("submit", 2, {}), ("cancel", [0, 6, 1]), ("bad_cancel", [7]), ("advance", 1), ("collect",),
              ("bad_cancel", [0]), ("advance", 1), ("collect",), ("submit", 2, {}), ("advance", None), ("collect",)]
CANCEL_CUT = {0: 3, 6: 1}     # sequence -> the tokens it keeps


# The cases of the kernel test (tests/test_gpu_roll_request_kernels.py) for rgrg_debug_roll_session_step_req at R rows, the five rows
# under test being the LAST five (R = 260: row 255 ends the first 256-row pass of the workgroup, 256 .. 259 are the second), the rows
# in front of them running sequences that go on: (name, C, n, S_before, submit, handout, retire, R, max_length, state, arg, ring,
# {sequence: the length word it has on entry}).
def hook_cases(R: int):
    T, L, F = 777, 9, R - 5          # F ordinary rows in front hold sequences 0 .. F - 1

    def case(name, rows, pending, arg, requests, ended=None):
        """rows: the (sequence offset, len) of the five rows, offset -1 = idle; sequences F + offset; `pending` more are submitted
        behind the highest one; requests: {offset: set_request keywords}; ended: {offset: length word} of sequences no row holds."""
        top = max(o for o, _ in rows) + 1
        S_ = F + top + pending
        C = S_ + 3
        st = M.new_state(R, S_)
        for r in range(F):
            st["seq"][r], st["len"][r], st["tok"][r], st["pos"][r], st["step"][r] = r, 2 + r % 3, 1000 + r, 1 + r % 3, 1 + r % 3
        for i, (o, ln) in enumerate(rows):
            if o >= 0:
                r = F + i
                st["seq"][r], st["len"][r], st["tok"][r], st["pos"][r], st["step"][r] = F + o, ln, 1000 + r, ln - 1, ln - 1
        st["shared"][:] = (F + top, pending + F + sum(1 for o, _ in rows if o >= 0), 0, 3)
        ring = new_ring(C, L)
        for o, kw in requests.items():
            set_request(ring, F + o, **kw)
        return (name, C, 1, S_, 0, 0, 1, R, L, st, np.array([T] * F + list(arg), dtype=np.int32), ring,
                {F + o: ln for o, ln in (ended or {}).items()})

    return [
        # limits 2 (retires on its first token), L - 1 and L in one pass: rows at 1, L - 2 and L - 2 tokens; only the last goes on
        case("limits_mixed", [(0, 1), (1, L - 2), (2, L - 2), (3, 3), (-1, 0)], 2, [T, T, T, T, T],
             {0: dict(max_length=2), 1: dict(max_length=L - 1), 2: dict(max_length=L), 3: dict(max_length=4)}),
        # a stop token in the same step as another row's EOS; the same token is no stop token for the row beside it
        case("stop_beside_eos", [(0, 3), (1, 2), (2, 4), (-1, 0), (3, 2)], 1, [EOS, 4242, 4242, T, T], {1: dict(stop=[4242])}),
        # four stop ids, the hit on the fourth; the third row has three of them and goes on
        case("fourth_stop_id", [(0, 3), (1, 2), (2, 4), (3, 1), (4, 5)], 3, [T, 31, 31, 50000, EOS],
             {1: dict(stop=[5, 7, 11, 31]), 2: dict(stop=[5, 7, 11]), 3: dict(stop=[50000, 5, 50001, 65534])}),
        # cancel: a running row (cut, -len, the token not appended); a pending sequence that takes its row in THIS pass (not cut yet);
        # a sequence that ended in the previous pass (its length word stays); the freed rows take the pending ones
        case("cancel_three_ways", [(1, 4), (2, 1), (-1, 0), (3, 6), (4, 2)], 2, [T, T, T, EOS, T],
             {0: dict(cancel=True), 1: dict(cancel=True), 2: dict(cancel=True), 5: dict(cancel=True)}, ended={0: 5}),
    ]
