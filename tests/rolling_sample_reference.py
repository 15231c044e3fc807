"""Numpy model of rolling-batch sampling (rgrg_decoder_sample_rolling): the retire-and-refill rule of
tests/rolling_reference.py driven by the reference sampler of tests/sample_reference.py.  No GPU, no torch.

A call decodes Q = S * n sequences, n hypotheses per feature row: sequence q = s * n + j belongs to feature row q // n, whose image
key / value a refill copies into slot 0 of the decoder row that takes q.  The rule that makes the result independent of the number
of decoder rows R: SEQUENCE q DRAWS THE TOKEN OF COLUMN c FROM THE PHILOX COUNTER (q, c - 1) - the counter of the lock-step
``sample()`` for its row q at step c - 1 - and the log-prob goes to lp[q][c].  Neither the decoder row nor the step of the call
enters.

The model's "decoder" is a toy: the logits of a row are a deterministic function of (the feature row whose key / value the row
holds, the tokens so far) over V columns; column 0 is EOS.  ``lock_step`` is ``sample()``: row q, step t, counter (q, t), PAD and
log-prob 0 behind EOS.

MUTATIONS are wrong rules an implementation could follow; tests/test_rolling_sample_reference.py shows that the checks tell each of
them from the rule.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

import rolling_reference as M
import sample_reference as sr

EOS = M.EOS
V = 24
MUTATIONS = ("counter_row", "counter_global_step", "counter_off_by_one", "lp_at_row", "ukv_mod")


def token_of(col: int) -> int:
    """Column 0 of the toy vocabulary is EOS; column j > 0 is token j."""
    return EOS if col == 0 else int(col)


def toy_logits(feature: int, history) -> np.ndarray:
    """fp32 [V]: a deterministic function of the feature row and the tokens behind BOS; EOS likely enough for ragged lengths."""
    rng = np.random.default_rng([7, int(feature)] + [int(t) for t in history])
    x = rng.normal(0.0, 1.5, V).astype(np.float32)
    x[0] += np.float32(1.0)
    return x


def lock_step(S: int, n: int, max_length: int, seed: int, temperature=1.0, top_k=0, top_p=1.0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``sample()``: every sequence q in a row of its own, step t under the counter (q, t) -> ids [Q, max_length] (BOS, tokens, PAD),
    log-probs float64 [Q, max_length] (0 in the BOS column and under PAD), lens [Q]."""
    Q = S * n
    ids, lens = M.new_output(Q, max_length)
    lp = np.zeros((Q, max_length))
    for q in range(Q):
        ln = 1
        while ln < max_length:
            col, logq = sr.Row(toy_logits(q // n, ids[q, 1:ln]), temperature, top_k, top_p).draw(seed, q, ln - 1)
            ids[q, ln], lp[q, ln] = token_of(col), logq
            ln += 1
            if col == 0:
                break
        lens[q] = ln
    return ids, lp, lens


def greedy_lengths_and_tokens(S: int, n: int, max_length: int):
    """The arg-max sequences of the toy decoder (first occurrence): natural lengths cut at max_length and the token table."""
    toks, lengths = [], []
    for q in range(S * n):
        row = [EOS]
        while len(row) < max_length:
            col = int(np.argmax(toy_logits(q // n, row[1:])))
            row.append(token_of(col))
            if col == 0:
                break
        toks.append(row)
        lengths.append(len(row) if row[-1] == EOS and len(row) > 1 else max_length + 1)
    return lengths, toks


def run(S: int, n: int, R: int, max_length: int, seed: int, temperature=1.0, top_k=0, top_p=1.0, mut: Optional[str] = None):
    """The whole rolling call -> (ids [Q, max_length], log-probs float64 [Q', max_length], lens [Q], steps with an active row,
    ukv trace [(sequence, feature row copied)]).  Q' = max(Q, R) rows so that the ``lp_at_row`` mutation has somewhere to write."""
    assert mut is None or mut in MUTATIONS, mut
    Q = S * n
    st = M.new_state(R, Q)
    ids, lens = M.new_output(Q, max_length)
    lp = np.zeros((max(Q, R), max_length))
    held = np.full(R, -1, dtype=np.int64)     # the feature row whose image key / value is in slot 0 of a decoder row
    trace: List[Tuple[int, int]] = []

    def refill(pairs):
        for r, seq in pairs:
            held[r] = seq % S if mut == "ukv_mod" else seq // n
            trace.append((seq, int(held[r])))

    refill(M.roll_step(st, np.zeros(R, dtype=np.int32), ids, lens, max_length))   # every row idle: the first hand-out
    t_global = 0
    while st["shared"][M.UNFINISHED] > 0 and t_global <= M.step_bound(Q, R, max_length):
        arg = np.zeros(R, dtype=np.int32)
        for r in range(R):
            seq, ln = int(st["seq"][r]), int(st["len"][r])
            if seq < 0:
                continue   # an idle row draws nothing and writes nothing
            row = sr.Row(toy_logits(held[r], ids[seq, 1:ln]), temperature, top_k, top_p)
            counter = {None: (seq, ln - 1), "lp_at_row": (seq, ln - 1), "ukv_mod": (seq, ln - 1), "counter_row": (r, ln - 1),
                       "counter_global_step": (seq, t_global), "counter_off_by_one": (seq, ln)}[mut]
            col, logq = row.draw(seed, *counter)
            arg[r] = token_of(col)
            lp[r if mut == "lp_at_row" else seq, ln] = logq
        refill(M.roll_step(st, arg, ids, lens, max_length))
        t_global += 1
    return ids, lp, lens, int(st["shared"][M.STEPS]), trace
