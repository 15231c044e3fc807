"""Host model of the rolling beam session (rgrg_decoder_beam_roll_*) for the tests, on top of the schedule model of
rolling beam search (tests/rolling_beam_reference.py: its constants, its bound, the oracle's ``BeamHypotheses``; ``schedule`` itself
is what the all-at-once case is compared with).  No GPU.

Like that model it is fed with the per-region candidate traces of ``oracle.language_model.beam_generate(..., return_trace=True)``
over a pool of feature rows: the candidates a region ranks at ITS k-th iteration are ``trace[k][..][f]`` for the pool row f whose
image key / value the region's slot holds - whichever step and slot runs that iteration.

What is modelled:
  arrivals     an op list - ("submit", m), ("refused", m), ("advance", k or None), ("collect",) - played by ``play``
  the ring     image key / value rows [capacity], row q % capacity, written by submit, read when a slot is seated; the watermark;
               a submit whose last region would reach watermark + capacity is refused (``RingFull``) and changes nothing
  seating      free slots take the pending regions in ascending slot order, only in front of a step that is launched
  advance      up to k steps (None: until drained); nothing is launched when no slot is occupied and nothing is pending
  collect      the finished regions not delivered yet, ascending; the delivered PREFIX is released
and per call the counts the host reports: ``launched`` (advance's return), ``unfinished``, ``steps``.

A VIOLATION (AssertionError) is raised when a slot reads a ring row that does not hold its region's feature row or reads outside the
ring, when a submit overwrites the ring row of a region that is not released, and when a release passes an unfinished region.

``Session(..., mutate=NAME)`` applies one named defect; tests/test_rolling_beam_session_reference.py shows that the cases the GPU
tests run (``CASES``) reject every one of them."""
import torch

import rolling_beam_reference as M
from oracle.beam_scorer import BeamHypotheses

BOS = EOS = PAD = M.BOS
MUTATIONS = ("ukv_row_without_modulo", "stale_heap", "slots_bounded_by_first_submit", "step_with_all_idle", "release_past_unfinished",
             "seat_at_tail")


class RingFull(Exception):
    pass


# The cases the GPU tests run, as (rows, num_beams, capacity, max_length, ops).  iterations of the first regions under early
# stopping at max_length 12 (tests/test_rolling_beam_reference.py): 10, 3, 11, 11, 5, 3, 11, 5, 2, 11, 4.
#
# CASE_1: 2 slots, a ring of 3, 7 regions in submits of 1, 3 and 3.  Region 0 alone (slot 1 idles), a refusal (room for 2), a region
# left mid-flight between advances, a drain and an advance on the drained session; regions 1 .. 3 wrap the ring inside ONE submit
# (rows 1, 2, 0); region 1 leaves with the LAST step of advance(3) while 3 is pending, so 3 is seated by the next advance; a
# refusal while 2 and 3 run; regions 4 .. 6 wrap again; 5 finishes before 4, is delivered, and the ring stays full behind 4.
CASE_1_OPS = (("submit", 1), ("advance", 1), ("refused", 3), ("advance", 3), ("collect",), ("advance", None), ("advance", 2),
              ("collect",), ("submit", 3), ("advance", 3), ("collect",), ("refused", 3), ("advance", 1), ("advance", None), ("collect",),
              ("submit", 3), ("advance", 3), ("collect",), ("refused", 1), ("advance", None), ("collect",))
CASE_1 = (8, 4, 3, 12, CASE_1_OPS)
# IDLE_AND_REUSE: nothing submitted yet; a drain; advances on the drained session; a later submit of 3 on 2 slots - slot 1 has
# been idle since the open when it is seated.
IDLE_OPS = (("advance", None), ("advance", 3), ("collect",), ("submit", 1), ("advance", None), ("advance", None), ("advance", 5),
            ("collect",), ("submit", 3), ("advance", 2), ("advance", None), ("collect",))
IDLE_AND_REUSE = (8, 4, 8, 12, IDLE_OPS)
CASES = {"case_1": CASE_1, "idle_and_reuse": IDLE_AND_REUSE}


class Session:
    """The session for regions whose feature rows are pool rows 0, 1, 2, ... in submit order."""

    def __init__(self, trace, nb, R, capacity, max_length, early, keep=1, lp=1.0, mutate=None):
        assert mutate is None or mutate in MUTATIONS, mutate
        assert R >= nb and capacity >= 1
        self.trace, self.nb, self.R, self.capacity, self.L, self.early, self.keep, self.lp, self.mut = (
            trace, nb, R, capacity, max_length, early, keep, lp, mutate)
        self.G = R // nb                                 # fixed for the life of the session
        self._G_fixed = mutate != "slots_bounded_by_first_submit"
        self.submitted = self.watermark = self.next = self.steps = 0
        self.ring = [None] * capacity                    # the pool row whose image key / value a ring row holds
        self.owner = [None] * capacity                   # the region a ring row was last written for
        self.hyps, self.finished, self.delivered = {}, set(), set()
        self.result = {}                                 # region -> int64 [keep, L_q]
        self._new_slots(self.G)
        self.log = []                                    # one entry per call: (op, launched, unfinished, steps)

    def _new_slots(self, G):
        nb = self.nb
        self.region, self.cur_len, self.done = [-1] * G, [1] * G, [False] * G
        self.kv = [None] * G                             # the pool row in slot 0 of the slot's first cache row
        self.last_heap = [None] * G
        self.ids = [[torch.tensor([BOS]) for _ in range(nb)] for _ in range(G)]
        self.scores = [[0.0] * nb for _ in range(G)]
        self.iteration = [0] * G

    @property
    def unfinished(self):
        return (self.submitted - self.next) + sum(r >= 0 for r in self.region)

    # ------------------------------------------------------------------ the calls
    def submit(self, m):
        q0 = self.submitted
        if q0 + m > self.watermark + self.capacity:
            raise RingFull(f"capacity {self.capacity} regions, room for {self.watermark + self.capacity - q0}")
        if not self._G_fixed:
            self.G, self._G_fixed = min(self.R // self.nb, m), True
            self._new_slots(self.G)
        for q in range(q0, q0 + m):
            row = q % self.capacity
            assert self.owner[row] is None or self.owner[row] < self.watermark, f"VIOLATION: region {q} overwrites ring row {row} of region {self.owner[row]}"
            self.ring[row], self.owner[row] = q, q     # region q decodes pool row q
            self.hyps[q] = BeamHypotheses(self.nb, self.lp, self.early)
        self.submitted = q0 + m
        return range(q0, q0 + m)

    def _seat(self, g, refill=True):
        q = self.next
        self.next += 1
        self.region[g], self.cur_len[g], self.done[g], self.iteration[g] = q, 1, False, 0
        self.ids[g] = [torch.tensor([BOS]) for _ in range(self.nb)]
        self.scores[g] = [0.0] + [-1e9] * (self.nb - 1)
        if self.mut == "stale_heap" and self.last_heap[g] is not None:
            self.hyps[q].beams, self.hyps[q].worst_score = list(self.last_heap[g].beams), self.last_heap[g].worst_score
        if refill:
            row = q if self.mut == "ukv_row_without_modulo" else q % self.capacity
            assert 0 <= row < self.capacity, f"VIOLATION: region {q} reads ring row {row} of {self.capacity}"
            self.kv[g] = self.ring[row]
        assert self.kv[g] == q, f"VIOLATION: the slot of region {q} holds the image key / value of pool row {self.kv[g]}"

    def _step(self):
        nb = self.nb
        for g in range(self.G):
            q = self.region[g]
            if q < 0:
                continue
            sc, tk, ix = (t[self.kv[g]] for t in self.trace[self.iteration[g]])
            nscore, ntok, nidx = [], [], []
            for rank in range(2 * nb):
                if int(tk[rank]) == EOS:
                    if rank >= nb:
                        continue
                    self.hyps[q].add(self.ids[g][int(ix[rank])].clone(), sc[rank].item())
                else:
                    nscore.append(float(sc[rank])); ntok.append(int(tk[rank])); nidx.append(int(ix[rank]))
                if len(ntok) == nb:
                    break
            assert len(ntok) == nb
            self.done[g] = self.done[g] or self.hyps[q].is_done(sc.max().item(), self.cur_len[g])
            self.ids[g] = [torch.cat([self.ids[g][nidx[j]], torch.tensor([ntok[j]])]) for j in range(nb)]
            self.scores[g] = nscore
            self.cur_len[g] += 1
            self.iteration[g] += 1
        for g in range(self.G):
            q = self.region[g]
            if q < 0 or (not self.done[g] and self.cur_len[g] < self.L):
                continue
            if not self.done[g]:                          # BeamSearchScorer.finalize: the open beams of an undone region
                for j in range(nb):
                    self.hyps[q].add(self.ids[g][j], self.scores[g][j])
            self.finished.add(q)
            self.last_heap[g] = self.hyps[q]
            self.region[g] = -1
        self.steps += 1

    def advance(self, k=None):
        """-> steps launched."""
        bound = (-(-self.unfinished // self.G) + 1) * (self.L - 1)
        limit = bound if k is None else k
        launched = 0
        while launched < limit and (self.unfinished > 0 or (self.mut == "step_with_all_idle" and k is not None)):
            for g in range(self.G):
                if self.region[g] < 0 and self.next < self.submitted:
                    self._seat(g)
            occupied = any(r >= 0 for r in self.region)
            self._step()
            if not occupied:
                self.steps -= 1                           # (the device counts steps that had an occupied slot)
            launched += 1
        if self.mut == "seat_at_tail":                    # the one-shot loop's order: seated behind the step, the refill list lost
            for g in range(self.G):
                if self.region[g] < 0 and self.next < self.submitted:
                    self._seat(g, refill=False)
        assert k is not None or self.unfinished == 0, "regions unfinished after the bound"
        return launched

    def best(self, q):
        """int64 [keep, L_q] - what beam_write_best writes for a call over region q alone."""
        ranked = sorted(self.hyps[q].beams, key=lambda x: x[0])
        assert len(ranked) >= self.keep
        rows = [ranked.pop()[1] for _ in range(self.keep)]
        width = min(max(len(b) for b in rows) + 1, self.L)
        out = torch.full((self.keep, width), PAD, dtype=torch.int64)
        for i, b in enumerate(rows):
            out[i, :len(b)] = b
            if len(b) < self.L:
                out[i, len(b)] = EOS
        return out

    def release(self, wm):
        assert self.watermark <= wm <= self.submitted
        for q in range(self.watermark, wm):
            assert q in self.finished, f"VIOLATION: release past the unfinished region {q}"
            del self.hyps[q]
        self.watermark = wm

    def collect(self):
        """-> the regions delivered, ascending."""
        new = [q for q in range(self.watermark, self.submitted) if q in self.finished and q not in self.delivered]
        for q in new:
            self.result[q] = self.best(q)
            self.delivered.add(q)
        wm = self.watermark
        if self.mut == "release_past_unfinished":
            wm = max([wm] + [q + 1 for q in new])
            for q in range(self.watermark, wm):
                self.hyps.pop(q, None)
            self.watermark = wm
            return new
        while wm in self.delivered:
            wm += 1
        self.release(wm)
        return new


def play(ses, ops):
    """Runs ops on the model -> one (op, value, unfinished, steps, watermark) per op: value = the range of a submit, "refused", the
    steps an advance launched, the regions a collect delivered.  A "refused" op whose submit is accepted is an AssertionError."""
    out = []
    for op in ops:
        if op[0] == "submit":
            val = ses.submit(op[1])
        elif op[0] == "refused":
            try:
                ses.submit(op[1])
            except RingFull:
                val = "refused"
            else:
                raise AssertionError(f"a submit of {op[1]} regions that does not fit was accepted")
        elif op[0] == "advance":
            val = ses.advance(op[1])
        else:
            val = ses.collect()
        out.append((op, val, ses.unfinished, ses.steps, ses.watermark))
    return out


def table(result, regions, keep, pad_to=None):
    """The delivered regions as one call returns them: [len(regions) * keep, widest], PAD behind a region's own width."""
    width = max(result[q].shape[1] for q in regions)
    out = torch.full((len(regions) * keep, pad_to or width), PAD, dtype=torch.int64)
    for i, q in enumerate(regions):
        out[i * keep:(i + 1) * keep, :result[q].shape[1]] = result[q]
    return out
