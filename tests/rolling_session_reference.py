"""Numpy model of a rolling session (rgrg_amd/csrc/decoder_roll.hip) on top of ``rolling_reference.roll_step``, which
is imported and used as it is: S grows between steps, a submit ends in a hand-out-only pass, the output and the image key / value
rows live in rings, and the host advances, collects and releases as rgrg_decoder_roll_* do.  No GPU, no torch.

Device side, on plain arrays (what rgrg_debug_roll_session_step runs; ``session_step`` is its model):
  submit_init      the new sequences' ring rows -> BOS, PAD, log-probs 0, length 0; S and the unfinished word grow
  handout_pass     roll_step over the IDLE rows only: they take pending sequences in ascending row order, a row that holds a sequence
                   is not touched, no step is counted
  retire_pass      roll_step as it is, its writes going through the ring
Sequence q uses output row q % C and ukv row (q // n) % (C // n).

Host side, ``Session``: the watermark (a submit whose last sequence would reach watermark + C is refused), the advance rule (the
unfinished word polled every 16 steps and 16 steps late; nothing launched when the last poll said 0 and no submit came since),
collect and release.  The model records a VIOLATION whenever a write lands in a ring row that belongs to another sequence, a submit
takes the ring row of a sequence that has not been delivered, or a refill reads a ukv row that holds another feature row.

MUTATIONS are wrong rules an implementation could have; tests/test_rolling_session_reference.py shows that the cases the GPU tests
run reject each of them.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

import rolling_reference as M

BOS = EOS = PAD = M.BOS
NEXT, UNFINISHED, REFILLS, STEPS = M.NEXT, M.UNFINISHED, M.REFILLS, M.STEPS
MUTATIONS = ("slot_without_modulo", "release_past_unfinished", "handout_appends", "submit_resets_rows", "unfinished_not_raised",
             "ukv_by_sequence")
ROW_KEYS = ("seq", "len", "tok", "pos", "step")


class RingFull(Exception):
    pass


class _Ids:
    """What roll_step sees as ids [S][..]: row q is ring row slot(q) of the store."""

    def __init__(self, store, S, slot, writes):
        self.store, self.shape, self.slot, self.writes = store, (S, store.shape[1]), slot, writes

    def __setitem__(self, key, value):
        seq, col = key
        row = self.slot(int(seq))
        self.writes.append((int(seq), row))
        if 0 <= row < self.store.shape[0]:
            self.store[row, col] = value


class _Lens:
    def __init__(self, store, slot, writes):
        self.store, self.slot, self.writes = store, slot, writes

    def __setitem__(self, seq, value):
        row = self.slot(int(seq))
        self.writes.append((int(seq), row))
        if 0 <= row < self.store.shape[0]:
            self.store[row] = value


def _slot(C: int, mut: Optional[str]):
    return (lambda q: q) if mut == "slot_without_modulo" else (lambda q: q % C)


def ukv_row(q: int, n: int, C: int, mut: Optional[str] = None) -> int:
    Cf = C // n
    return q % Cf if mut == "ukv_by_sequence" else (q // n) % Cf


def submit_init(st, ids, lens, lp, C: int, S_before: int, count: int, max_length: int, mut: Optional[str] = None) -> int:
    """-> the new S.  Writes columns 0 .. max_length - 1 of the new rows only."""
    slot = _slot(C, mut)
    for q in range(S_before, S_before + count):
        r = slot(q)
        if 0 <= r < ids.shape[0]:
            ids[r, :max_length] = PAD
            ids[r, 0] = BOS
            lens[r] = 0
            if lp is not None:
                lp[r, :max_length] = 0.0
    if mut != "unfinished_not_raised":
        st["shared"][UNFINISHED] += count
    if mut == "submit_resets_rows":
        st["seq"][:], st["len"][:], st["tok"][:], st["pos"][:], st["step"][:] = -1, 0, BOS, 0, 0
    return S_before + count


def handout_pass(st, arg, ids, lens, C: int, S: int, max_length: int, mut: Optional[str] = None, writes=None) -> List[Tuple[int, int]]:
    """The hand-out-only pass -> [(row, sequence)] in hand-out order."""
    writes = [] if writes is None else writes
    slot = _slot(C, mut)
    if mut == "handout_appends":
        return M.roll_step(st, arg, _Ids(ids, S, slot, writes), _Lens(lens, slot, writes), max_length)
    idle = np.flatnonzero(st["seq"] < 0)
    sub = {k: st[k][idle].copy() for k in ROW_KEYS}
    sub["shared"] = st["shared"].copy()
    refills = M.roll_step(sub, np.zeros(len(idle), dtype=np.int32), _Ids(ids, S, slot, writes), _Lens(lens, slot, writes), max_length)
    for k in ROW_KEYS:
        st[k][idle] = sub[k]
    st["shared"][NEXT], st["shared"][REFILLS] = sub["shared"][NEXT], sub["shared"][REFILLS]
    if mut != "unfinished_not_raised":
        st["shared"][UNFINISHED] = (S - int(sub["shared"][NEXT])) + int((st["seq"] >= 0).sum())
    return [(int(idle[r]), q) for r, q in refills]


def retire_pass(st, arg, ids, lens, C: int, S: int, max_length: int, mut: Optional[str] = None, writes=None) -> List[Tuple[int, int]]:
    writes = [] if writes is None else writes
    slot = _slot(C, mut)
    return M.roll_step(st, arg, _Ids(ids, S, slot, writes), _Lens(lens, slot, writes), max_length)


def session_step(st, arg, ids, lens, lp, C, n, S_before, submit, handout, retire, max_length, mut=None):
    """rgrg_debug_roll_session_step IN PLACE -> the refills of the hand-out pass and of the retire pass, each (row, sequence, ukv ring row)."""
    S = submit_init(st, ids, lens, lp, C, S_before, submit, max_length, mut) if submit else S_before
    a = handout_pass(st, arg, ids, lens, C, S, max_length, mut) if handout else []
    b = retire_pass(st, arg, ids, lens, C, S, max_length, mut) if retire else []
    tag = lambda rf: [(r, q, ukv_row(q, n, C, mut)) for r, q in rf]   # noqa: E731
    return tag(a), tag(b)


# ------------------------------------------------------------------------------------------------ the host
class Session:
    """The whole session for sequences that end at given natural lengths: ``lengths[q]`` for sequence q (as run_schedule: the arg-max
    of a row that holds q with len tokens is EOS when len + 1 == lengths[q], else token(q, len))."""

    def __init__(self, lengths, R: int, C: int, n: int, max_length: int, mut: Optional[str] = None, token=lambda s, j: 1000 + 7 * s + j):
        assert mut is None or mut in MUTATIONS, mut
        assert C % n == 0
        self.lengths, self.R, self.C, self.n, self.L, self.mut, self.token = list(lengths), R, C, n, max_length, mut, token
        self.st = M.new_state(R, 0)
        self.ids, self.lens = M.sentinel_output(C, max_length + 1)     # one spare column, as run_schedule has
        self.S = 0
        self.watermark = 0
        self.unfinished = 0          # the host's: as of the last synchronisation, plus what was submitted since
        self.drained = True
        self.h_len = np.zeros(C, dtype=np.int32)
        self.owner = np.full(C, -1, dtype=np.int64)        # the sequence a ring row was last given to
        self.ukv_owner = np.full(C // n, -1, dtype=np.int64)
        self.delivered, self.collected = set(), set()
        self.results: Dict[int, np.ndarray] = {}
        self.violations: List[str] = []
        self.trace: List[List[Tuple[int, int]]] = []
        self.launched = 0

    # -- bookkeeping of the checks
    def _check_writes(self, writes):
        for q, row in writes:
            if not 0 <= row < self.C:
                self.violations.append(f"write for sequence {q} outside the ring (row {row})")
            elif self.owner[row] != q:
                self.violations.append(f"write for sequence {q} in ring row {row}, which belongs to sequence {int(self.owner[row])}")

    def _check_refills(self, refills):
        for _, q in refills:
            row = ukv_row(q, self.n, self.C, self.mut)
            if self.ukv_owner[row] != q // self.n:
                self.violations.append(f"sequence {q} reads ukv row {row}, which holds feature row {int(self.ukv_owner[row])}")

    # -- the calls
    def submit(self, m: int) -> range:
        count = m * self.n
        q0 = self.S
        if q0 + count > self.watermark + self.C:
            raise RingFull(f"capacity {self.C // self.n} feature rows, room for {(self.watermark + self.C - q0) // self.n}")
        assert q0 + count <= len(self.lengths), "the test's list of lengths is too short"
        for q in range(q0, q0 + count):
            row = q % self.C
            if self.owner[row] >= 0 and int(self.owner[row]) not in self.delivered:
                self.violations.append(f"sequence {q} takes ring row {row} of sequence {int(self.owner[row])}, which was not delivered")
            self.owner[row] = q
            self.h_len[row] = 0
        for f in range(q0 // self.n, (q0 + count) // self.n):
            self.ukv_owner[f % (self.C // self.n)] = f
        self.S = submit_init(self.st, self.ids, self.lens, None, self.C, q0, count, self.L, self.mut)
        if self.mut != "unfinished_not_raised":   # (the host knows what the word says)
            self.unfinished += count
            self.drained = False
        writes: List[Tuple[int, int]] = []
        refills = handout_pass(self.st, self._arg(), self.ids, self.lens, self.C, self.S, self.L, self.mut, writes)
        self._check_writes(writes)
        self._check_refills(refills)
        self.trace.append(refills)
        return range(q0, q0 + count)

    def _arg(self) -> np.ndarray:
        arg = np.zeros(self.R, dtype=np.int32)
        for r in range(self.R):
            s, ln = int(self.st["seq"][r]), int(self.st["len"][r])
            if 0 <= s < len(self.lengths):
                arg[r] = EOS if ln + 1 == int(self.lengths[s]) else self.token(s, ln)
        return arg

    def bound(self) -> int:
        return ((self.unfinished + self.R - 1) // self.R + 1) * (self.L - 1)

    def advance(self, steps: Optional[int] = None) -> int:
        """-> steps launched.  The host rule of rgrg_decoder_roll_advance."""
        limit = self.bound() if steps is None else steps
        launched = 0
        if not self.drained and limit > 0:
            polls, seen = 0, [1, 1]
            for t in range(limit):
                writes: List[Tuple[int, int]] = []
                refills = retire_pass(self.st, self._arg(), self.ids, self.lens, self.C, self.S, self.L, self.mut, writes)
                self._check_writes(writes)
                self._check_refills(refills)
                self.trace.append(refills)
                launched += 1
                if (t & 15) == 15 and t + 1 < limit:
                    if polls > 0 and seen[(polls - 1) & 1] == 0:
                        break
                    seen[polls & 1] = int(self.st["shared"][UNFINISHED])   # (the copy is read 16 steps later)
                    polls += 1
        if launched > 0 or not self.drained:
            self.unfinished = int(self.st["shared"][UNFINISHED])
            self.drained = self.unfinished == 0
            self.h_len = np.where(self.lens < 0, 0, self.lens).astype(np.int32)
        self.launched += launched
        return launched

    @property
    def device_steps(self) -> int:
        return int(self.st["shared"][STEPS])

    def finished(self) -> List[int]:
        """Sequences at or above the watermark that have ended, as of the last advance."""
        return [q for q in range(self.watermark, self.S) if self.h_len[q % self.C] > 0]

    def release(self, watermark: int) -> None:
        assert self.watermark <= watermark <= self.S
        if self.mut != "release_past_unfinished":
            for q in range(self.watermark, watermark):
                if self.h_len[q % self.C] == 0:
                    raise ValueError(f"sequence {q} below the new watermark {watermark} has not finished")
        self.watermark = watermark

    def collect(self) -> List[int]:
        """Delivers every finished sequence not delivered yet -> their numbers; the watermark moves over the delivered prefix (the
        mutation: behind the last delivered one)."""
        new = [q for q in self.finished() if q not in self.collected]
        for q in new:
            n = int(self.h_len[q % self.C])
            row = np.full(self.L, PAD, dtype=np.int64)
            row[:n] = self.ids[q % self.C, :n]
            self.results[q] = row
            self.collected.add(q)
            self.delivered.add(q)
        wm = self.watermark
        if self.mut == "release_past_unfinished":
            wm = max([wm] + [q + 1 for q in self.collected])
        else:
            while wm in self.collected:
                wm += 1
        self.collected = {q for q in self.collected if q >= wm}
        self.release(wm)
        return new


def play(lengths, R, C, n, max_length, ops, mut=None):
    """Runs ``ops`` - ("submit", m) / ("refused", m) / ("advance", steps or None) / ("collect",) / ("stream", total, m, steps) - and drains, collecting, at the
    end -> (session, log), log holding one entry per op: the range of a submit, the steps of an advance, the sequences of a collect."""
    s = Session(lengths, R, C, n, max_length, mut)
    log = []
    for op in ops:
        if op[0] == "submit":
            log.append(s.submit(op[1]))
        elif op[0] == "refused":
            try:
                s.submit(op[1])
                log.append(False)
            except RingFull as e:
                log.append(str(e))
        elif op[0] == "advance":
            log.append(s.advance(op[1]))
        elif op[0] == "stream":   # (total, m, steps): until `total` feature rows are in - submit up to m as they fit, advance, collect
            rounds = 0
            while s.S < op[1] * n and rounds < 100 * op[1]:
                m = min(op[2], op[1] - s.S // n, (s.watermark + C - s.S) // n)
                if m > 0:
                    s.submit(m)
                s.advance(op[3])
                s.collect()
                rounds += 1
            log.append(rounds)
        else:
            log.append(s.collect())
    s.advance(None)
    log.append(s.collect())
    return s, log


def correct(s: Session, total: int) -> bool:
    """Every one of the first ``total`` sequences was delivered with expected_ids' row, and nothing was violated."""
    want, _ = M.expected_ids(s.lengths[:total], s.L, s.token)
    return (not s.violations and s.S == total and sorted(s.results) == list(range(total)) and
            all(np.array_equal(s.results[q], want[q]) for q in range(total)))


# ------------------------------------------------------------------------------------------------ what the GPU tests run
# The end-to-end schedules of tests/test_gpu_roll_session.py as (name, lengths, R, C, n, max_length, ops).  LENGTHS_12 are the oracle's
# lengths of the first 11 feature rows at max_length 12 (tests/test_gpu_rolling.py).
LENGTHS_12 = [12, 3, 2, 12, 7, 2, 12, 5, 2, 12, 3]
CASE_1_OPS = [("submit", 5), ("refused", 3), ("advance", 2), ("collect",), ("refused", 2), ("submit", 1), ("advance", None), ("collect",),
              ("submit", 5), ("advance", None), ("collect",)]


def _ragged(S, seed):
    return [int(v) for v in np.random.default_rng(seed).choice([2, 3, 5, 7, 12], size=S)]


def schedule_cases():
    every3 = lambda S, m: sum(([("submit", m), ("advance", 3), ("collect",)] for _ in range(S // m)), [])   # noqa: E731
    return [
        ("case_1", LENGTHS_12, 4, 6, 1, 12, CASE_1_OPS),
        ("turnover", _ragged(70, 1), 33, 40, 1, 8, every3(70, 10)),
        ("more_rows_than_ring", _ragged(30, 2), 8, 4, 1, 6, [("stream", 30, 3, 1)]),
        ("all_at_once", LENGTHS_12, 4, 16, 1, 12, [("submit", 11)]),
        ("sampling_n2", _ragged(18, 3), 4, 8, 2, 12, [("submit", 4), ("advance", 4), ("collect",), ("advance", None), ("collect",), ("submit", 3),
                                                     ("advance", 5), ("collect",), ("advance", None), ("collect",), ("submit", 2)]),
        ("idle_and_reuse", LENGTHS_12, 4, 8, 1, 12, [("submit", 3), ("advance", None), ("collect",), ("advance", None), ("submit", 2)]),
    ]


# The cases of the kernel test (tests/test_gpu_roll_session_kernels.py) for rgrg_debug_roll_session_step:
# (name, C, n, S_before, submit, handout, retire, R, max_length, state, arg).
def hook_cases():
    T = 777

    def case(name, C, n, S_before, submit, handout, retire, max_length, rows, nxt, arg, steps=3):
        R = len(rows)
        st = M.new_state(R, S_before)
        for r, (seq, ln) in enumerate(rows):
            st["seq"][r], st["len"][r] = seq, ln
            if seq >= 0:
                st["tok"][r], st["pos"][r], st["step"][r] = 1000 + r, ln - 1, ln - 1
        st["shared"][:] = (nxt, (S_before - nxt) + sum(1 for seq, _ in rows if seq >= 0), 0, steps)
        return name, C, n, S_before, submit, handout, retire, R, max_length, st, np.array(arg, dtype=np.int32)

    many = [((r - 1 - r // 5) + 2000, 1 + r % 8) if r % 5 else (-1, 0) for r in range(600)]
    return [
        # sequences 6 .. 10 live in a ring of 5: the hand-out gives 8, 9, 10 -> ring rows 3, 4, 0 in ONE pass; then 6 ends
        case("slots_wrap_in_one_handout", 5, 1, 8, 3, 1, 1, 8, [(6, 3), (-1, 0), (7, 2), (-1, 0), (-1, 0)], 8, [EOS, T, T, T, T]),
        # sequences 3 .. 9 pass through: 3 and 4 end, 7 and 8 take their rows, 9 stays pending
        case("ring_of_5_retire", 5, 1, 7, 3, 1, 1, 6, [(3, 2), (4, 5), (5, 1), (6, 2)], 7, [EOS, T, T, T]),
        # n = 2, three ukv ring rows: feature rows 3 and 4 arrive (ukv rows 0 and 1); 6, 7, 8 go to idle rows, 9 to the row 4 leaves
        case("two_per_feature_row", 6, 2, 6, 4, 1, 1, 8, [(4, 2), (5, 3), (-1, 0), (-1, 0), (-1, 0)], 6, [EOS, T, T, T, T]),
        # the hand-out-only pass alone over active and idle rows (arg holds EOS everywhere: it must not be read)
        case("handout_only_mixed", 8, 1, 9, 0, 1, 0, 6, [(4, 3), (-1, 0), (6, 5), (-1, 0), (5, 1), (-1, 0)], 7, [EOS] * 6),
        case("handout_only_nothing_pending", 8, 1, 7, 0, 1, 0, 6, [(4, 3), (-1, 0), (6, 5)], 7, [EOS] * 3),
        # the submit-init alone: exactly the new rows (13 -> ring row 5, 14 -> 6, 15 -> 7, 16 -> 0)
        case("submit_init_only", 8, 1, 13, 4, 0, 0, 6, [(11, 3), (-1, 0), (12, 5)], 13, [T] * 3),
        # three passes of the 256-thread workgroup, every fifth row idle, sequence numbers beyond the ring of 1024
        case("many_rows", 1024, 1, 2800, 100, 1, 1, 9, many, 2480, [EOS if r % 3 == 0 else T for r in range(600)]),
    ]
