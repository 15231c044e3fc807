"""Numpy model of rolling-batch greedy decoding (rgrg_amd/csrc/decoder_roll.hip): the retire-and-refill rule of one step, and a
whole schedule driven by given per-sequence lengths.  No GPU, no torch.

State of R decoder rows (int32 arrays [R]): ``seq`` the sequence a row holds (-1 = idle), ``len`` its tokens so far (BOS included),
``tok`` / ``pos`` / ``step`` the token, embedding position and step of the row's next decode step.  ``shared`` (int32 [4]): the next
pending sequence, the unfinished sequences, the refills of the last step, the steps that had an active row.

One step, after the arg-max ``arg`` [R] of the decode step just run:
  an active row appends arg[r] at ids[seq][len]; it retires when that token is EOS or was the max_length-th token of the sequence
  (lens[seq] = the length, the EOS included); otherwise token, position = step = len - 1 are its next input;
  free rows - retired in this step, or idle - take the pending sequences in ASCENDING ROW ORDER while there are any (BOS, position 0,
  step 0, len 1; (row, sequence) is listed for the slot-0 copy); a free row without a sequence idles with the BOS state and writes
  nothing; ``next`` advances by the sequences handed out.

MUTATIONS are wrong rules a kernel could implement; tests/test_rolling_reference.py shows that the cases the GPU test runs tell
each of them from the rule.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

BOS = EOS = PAD = 50256
NEXT, UNFINISHED, REFILLS, STEPS = 0, 1, 2, 3
MUTATIONS = ("descending_rows", "retire_late", "eos_not_appended", "idle_writes", "next_by_free")


def new_state(R: int, S: int) -> Dict[str, np.ndarray]:
    """Every row idle, nothing handed out (what roll_begin_kernel leaves)."""
    z = lambda v: np.full(R, v, dtype=np.int32)   # noqa: E731
    return {"seq": z(-1), "len": z(0), "tok": z(BOS), "pos": z(0), "step": z(0), "shared": np.array([0, S, 0, 0], dtype=np.int32)}


def new_output(S: int, max_length: int, ld: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    ids = np.full((S, ld or max_length), PAD, dtype=np.int64)
    ids[:, 0] = BOS
    return ids, np.zeros(S, dtype=np.int32)


def sentinel_output(S: int, ld: int) -> Tuple[np.ndarray, np.ndarray]:
    """An output buffer that shows every write: EOS and PAD are one token id, so in new_output() an EOS that is NOT appended looks
    like one that is.  The kernel cases run on this."""
    return np.full((S, ld), -1, dtype=np.int64), np.full(S, -1, dtype=np.int32)


def roll_step(st: Dict[str, np.ndarray], arg: np.ndarray, ids: np.ndarray, lens: np.ndarray, max_length: int,
              mut: Optional[str] = None) -> List[Tuple[int, int]]:
    """One retire-and-refill step IN PLACE on st / ids / lens.  -> the refill list [(row, sequence)] in hand-out order."""
    assert mut is None or mut in MUTATIONS, mut
    R, S = st["seq"].shape[0], ids.shape[0]
    nxt = int(st["shared"][NEXT])
    free, any_active = [], False
    for r in range(R):
        seq = int(st["seq"][r])
        if seq < 0:
            if mut == "idle_writes":
                ids[min(nxt, S - 1), 1] = arg[r]
            free.append(r)
            continue
        any_active = True
        tok, ln = int(arg[r]), int(st["len"][r])
        if not (mut == "eos_not_appended" and tok == EOS):
            ids[seq, ln] = tok
        ln += 1
        limit = max_length + 1 if mut == "retire_late" else max_length
        if tok == EOS or ln >= limit:
            lens[seq] = ln
            free.append(r)
        else:
            st["len"][r], st["tok"][r], st["pos"][r], st["step"][r] = ln, tok, ln - 1, ln - 1
    given = min(len(free), S - nxt)
    order = list(reversed(free)) if mut == "descending_rows" else free
    refills = []
    for k, r in enumerate(order):
        seq = nxt + k if k < given else -1
        st["seq"][r], st["len"][r] = seq, 1 if seq >= 0 else 0
        st["tok"][r], st["pos"][r], st["step"][r] = BOS, 0, 0
        if seq >= 0:
            refills.append((r, seq))
    nxt += len(free) if mut == "next_by_free" else given
    st["shared"][NEXT] = nxt
    st["shared"][REFILLS] = given
    st["shared"][UNFINISHED] = (S - nxt) + int((st["seq"] >= 0).sum())
    st["shared"][STEPS] += 1 if any_active else 0
    return refills


def step_bound(S: int, R: int, max_length: int) -> int:
    """What the host loop allows: a sequence takes at most max_length - 1 steps and no row waits while a sequence is pending."""
    return ((S + R - 1) // R + 1) * (max_length - 1)


def expected_ids(lengths, max_length: int, token=lambda s, j: 1000 + 7 * s + j) -> Tuple[np.ndarray, np.ndarray]:
    """What any schedule must produce for sequences of the given natural lengths (BOS and EOS included; a sequence longer than
    max_length is cut there without an EOS): ids [S, max_length], lens [S]."""
    S = len(lengths)
    ids, lens = new_output(S, max_length)
    for s, n in enumerate(lengths):
        n = int(n)
        assert n >= 2
        for j in range(1, min(n, max_length)):
            ids[s, j] = EOS if j == n - 1 else token(s, j)
        lens[s] = min(n, max_length)
    return ids, lens


def run_schedule(lengths, R: int, max_length: int, mut: Optional[str] = None, token=lambda s, j: 1000 + 7 * s + j):
    """The whole call for sequences that end at the given natural lengths: the arg-max of a row that holds sequence s with len
    tokens is EOS when len + 1 == lengths[s], else token(s, len).  -> (ids [S, max_length + 1], lens, steps with an active row, trace
    of refill lists, state).
    Stops at step_bound + 1 steps (a mutation may never finish); ``unfinished`` of the last step is in the returned state."""
    S = len(lengths)
    st = new_state(R, S)
    ids, lens = new_output(S, max_length, max_length + 1)   # one spare column: a mutation that retires late writes there
    trace = [roll_step(st, np.zeros(R, dtype=np.int32), ids, lens, max_length, mut)]   # every row idle: the first hand-out
    steps = 0
    while st["shared"][UNFINISHED] > 0 and steps <= step_bound(S, R, max_length):
        arg = np.zeros(R, dtype=np.int32)
        for r in range(R):
            s, ln = int(st["seq"][r]), int(st["len"][r])
            if 0 <= s < S:
                arg[r] = EOS if ln + 1 == int(lengths[s]) else token(s, ln)
        trace.append(roll_step(st, arg, ids, lens, max_length, mut))
        steps += 1
    return ids, lens, int(st["shared"][STEPS]), trace, st


# The cases of the retire / refill kernel test (tests/test_gpu_rolling_kernels.py): (name, S, R, max_length, state overrides, arg).
# A state is given as rows (seq, len) - tok / pos / step follow - plus the next pending sequence.
def hook_cases():
    def case(name, S, R, max_length, rows, nxt, arg):
        st = new_state(R, S)
        for r, (seq, ln) in enumerate(rows):
            st["seq"][r], st["len"][r] = seq, ln
            if seq >= 0:
                st["tok"][r], st["pos"][r], st["step"][r] = 1000 + r, ln - 1, ln - 1
        st["shared"][:] = (nxt, (S - nxt) + sum(1 for seq, _ in rows if seq >= 0), 0, 3)
        return name, S, R, max_length, st, np.array(arg, dtype=np.int32)
    T = 777   # any token that is not EOS
    return [
        case("all_end_fewer_pending", 7, 5, 8, [(0, 3), (1, 2), (2, 4), (3, 1), (4, 5)], 5, [EOS] * 5),
        case("nothing_pending", 4, 4, 8, [(0, 3), (1, 2), (2, 4), (3, 1)], 4, [EOS, T, EOS, T]),
        case("max_length_without_eos", 6, 3, 5, [(0, 4), (1, 3), (2, 4)], 3, [T, T, EOS]),
        case("eos_first_token", 5, 3, 6, [(0, 1), (1, 1), (2, 2)], 3, [EOS, T, T]),
        case("one_row", 3, 1, 4, [(0, 2)], 1, [EOS]),
        case("more_rows_than_sequences", 2, 6, 6, [(-1, 0)] * 6, 0, [T] * 6),
        case("idle_rows_stay_idle", 3, 5, 6, [(0, 2), (-1, 0), (2, 3), (-1, 0), (1, 1)], 3, [T, T, EOS, T, T]),
        # three passes of the kernel's 256-thread workgroup; every fifth row idle although sequences are pending (the first hand-out)
        case("many_rows", 900, 600, 9, [(r - 1 - r // 5, 1 + r % 8) if r % 5 else (-1, 0) for r in range(600)], 480,
             [EOS if r % 3 == 0 else T for r in range(600)]),
    ]
