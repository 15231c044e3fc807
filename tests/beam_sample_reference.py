"""The beam-sampling ranking's contract (include/rgrg_hip.h "Beam-search sampling") restated in float64, the
acceptance rule a device result is judged by, the fixed inputs of the ranking tests and a CPU beam-sample loop over the oracle's
logits.  TEST INFRASTRUCTURE ONLY.  Only inv_T, w_i = lp_i * inv_T, s_i = beam_score + w_i and u are formed in fp32, as the kernel
forms them (u = (n + 0.5) 2^-24 is a 25-bit number that the kernel never rounds, so float64 holds what the kernel holds);
everything else - the log-probability, the noise g = -log(-log u), the key s + g - is float64.

Acceptance rule (derived from this reference alone, in the style of tests/sample_reference.py).  For an item with K = 2 num_beams:
a returned candidate set is accepted iff it holds K distinct kept entries, every one of them has a float64 key >= (the (K+1)-th
largest float64 key of the item) - band, every kept entry that was NOT returned has a key <= (the K-th largest) + band, and the
returned order is non-increasing in s up to band (exactly equal returned scores: ascending flat index).  The returned scores must
be the entries' s up to band.  band = 8 x the largest |fp32 evaluation - float64 evaluation| of a key + one fp32 ulp at the key's
magnitude; 8 is the margin used throughout the repository.  The maximum runs over the entries that can reach the boundary - the
K + 1 largest keys and every kept entry within 1 of the (K+1)-th - not over the whole item: the rows of a first step carry beam
score -1e9, their keys are 1e9 below the boundary and carry an fp32 error of 32, which would make the band useless.  The band
used is therefore never wider than one taken over the whole item.

An item is a coin flip, not a test of the ranking, when its K-th and (K+1)-th keys lie within band of each other, or when a
row's top-p threshold is a coin flip by the sampler's rule (sample_reference.Row.is_coin_flip): the generators redraw such items
(tests/test_beam_sample_reference.py pins the redraw rate below 1 %)."""
from __future__ import annotations

import itertools
from typing import Optional

import numpy as np
import torch

import sample_reference as sr

MARGIN = sr.MARGIN
f32, f64 = np.float32, np.float64
KINDS = sr.KINDS
V_MODEL, LD_MODEL = sr.V_MODEL, sr.LD_MODEL
MIN_GAP = 2e-3   # the repository's bound for fp32 last-step logits against the oracle (tests/group_beam_reference.py)


# ------------------------------------------------------------------------------------------------ noise
def philox4x32_10_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over broadcastable uint64 arrays holding 32-bit values -> the four output words."""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


def noise_words(seed: int, r, t: int, V: int, c3: int = 1):
    """word_i of row(s) r at step t for tokens 0 .. V-1: output word i & 3 of Philox4x32-10(key = seed, counter (r, t, i >> 2, c3)).
    r: an int or an array [R] -> uint64 [V] or [R, V]."""
    seed &= 0xFFFFFFFFFFFFFFFF
    r = np.asarray(r, dtype=np.uint64)
    blocks = np.arange((V + 3) // 4, dtype=np.uint64)
    w = philox4x32_10_np(r[..., None], np.uint64(t), blocks, np.uint64(c3), seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=-1).reshape(r.shape + (-1,))[..., :V]


def gumbel64(words):
    """g = -log(-log u), u = ((word >> 8) + 0.5) 2^-24 exactly, in float64 (log1p above one half, where the kernel takes it too)."""
    n = (np.asarray(words, dtype=np.uint64) >> np.uint64(8)).astype(f64)
    u = (n + 0.5) * 2.0 ** -24
    a = np.where(n < 2.0 ** 23, -np.log(u), -np.log1p(-(2.0 ** 24 - n - 0.5) * 2.0 ** -24))
    return -np.log(a)


def gumbel32(words):
    """The kernel's evaluation order in fp32 (each logarithm rounded once): what the band is measured with."""
    n = (np.asarray(words, dtype=np.uint64) >> np.uint64(8)).astype(f64)
    lo = ((n + 0.5) * 2.0 ** -24).astype(f32)                       # exact for n < 2^23
    hi = ((2.0 ** 24 - n - 0.5) * 2.0 ** -24).astype(f32)           # exact for n >= 2^23
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(n < 2.0 ** 23, -np.log(lo), -np.log1p(-hi)).astype(f32)
        return (-np.log(a)).astype(f32)


# ------------------------------------------------------------------------------------------------ one row, one item
class BeamRow:
    """Everything the contract defines for one beam row; ``mut`` names one deliberate mutation (tests)."""

    def __init__(self, x, beam_score, temperature=1.0, top_k=0, top_p=1.0, seed=0, r=0, t=0, mut=None):
        x = np.asarray(x, dtype=f32)
        V = x.shape[0]
        self.x, self.V, self.mut = x, V, mut
        inv_T = f32(1.0) / f32(temperature)
        min_keep = 1 if mut == "min_keep_1" else 2
        k_eff = int(top_k) if (top_k <= 0 or top_k >= min_keep) else min_keep
        self.row = row = sr.Row(x, temperature, k_eff, top_p)   # the sampler's filters (min_tokens_to_keep = 1), on x with inv_T
        finite = x > -np.inf
        keep = row.keep.copy()
        if min_keep == 2 and row.above is not None and V >= 2:   # top-p keeps the two largest logits and the ties of the second
            second = np.partition(x, V - 2)[V - 2]
            keep |= row._top_k_keep() & (x >= second)
        self.keep = keep & finite
        m = x[finite].max().astype(f64)
        with np.errstate(invalid="ignore"):
            lp = (x.astype(f64) - m) - np.log(np.exp(x[finite].astype(f64) - m).sum())
        bs = f32(beam_score)
        if mut == "warp_after_score":      # transformers 4.19.2: the warpers see log-prob + beam score
            self.s = ((bs.astype(f64) + lp) * f64(inv_T)).astype(f32)
        else:
            w = (lp * f64(inv_T)).astype(f32)
            self.s = (bs + w).astype(f32)
        words = noise_words(seed, r, t, V, c3=0 if mut == "sampler_counter" else 1)
        g = np.zeros(V) if mut == "no_noise" else gumbel64(words)
        with np.errstate(invalid="ignore"):
            self.key = np.where(self.keep, self.s.astype(f64) + g, -np.inf)
            # the fp32 evaluation of the same key, operation by operation as the kernel orders them
            m32 = f32(m)
            ls32 = np.log(np.exp((x[finite] - m32).astype(f32)).astype(f32).sum(dtype=f32)).astype(f32)
            s32 = (bs + (((x - m32).astype(f32) - ls32).astype(f32) * inv_T).astype(f32)).astype(f32)
            key32 = (s32 + gumbel32(words)).astype(f32)
            every = np.abs(key32.astype(f64) - (self.s.astype(f64) + g))
            self.err = np.where(self.keep, every, 0.0)
            self.err_row = float(every[finite].max())   # over every finite token, kept or not: the fp32 error of the row's key expression
        self.s = np.where(self.keep, self.s, f32(-np.inf))


class Item:
    """The nb rows of one item: flat index = beam * V + token."""

    def __init__(self, rows):
        self.rows, self.nb, self.V = rows, len(rows), rows[0].V
        self.K = 2 * self.nb
        self.key = np.concatenate([r.key for r in rows])
        self.s = np.concatenate([r.s for r in rows])
        self.keep = np.concatenate([r.keep for r in rows])
        err = np.concatenate([r.err for r in rows])
        order = np.lexsort((np.arange(self.key.size), -self.key))   # key descending, flat ascending
        self.order = order
        nk = int(self.keep.sum())
        self.kth = self.key[order[self.K - 1]] if nk >= self.K else -np.inf          # K-th largest key
        self.kth1 = self.key[order[self.K]] if nk >= self.K + 1 else -np.inf         # (K+1)-th
        near = self.keep & (self.key >= (self.kth1 if np.isfinite(self.kth1) else self.kth) - 1.0)
        near[order[:min(self.K + 1, nk)]] = True
        big = np.abs(self.key[near]).max()
        self.band = MARGIN * float(err[near].max()) + float(np.spacing(f32(big)))

    def select(self, mut=None):
        """-> (score f32 [K], token [K], beam [K]) of the contract: the K largest keys, emitted by s descending."""
        top = self.order[:self.K]
        top = top[np.isfinite(self.key[top])]
        if mut != "order_by_key":
            top = top[np.lexsort((top, -self.s[top].astype(f64)))]
        return self.s[top], (top % self.V).astype(np.int32), (top // self.V).astype(np.int32)

    def is_coin_flip(self):
        if np.isfinite(self.kth1) and self.kth - self.kth1 <= self.band:
            return True
        return any(r.row.is_coin_flip() for r in self.rows)

    def accept(self, score, tok, beam):
        """The acceptance rule -> (ok, message)."""
        score = np.asarray(score, dtype=f32)
        tok, beam = np.asarray(tok, dtype=np.int64), np.asarray(beam, dtype=np.int64)
        if not (score.shape == tok.shape == beam.shape == (self.K,)):
            return False, f"{score.shape[0]} candidates returned, K = {self.K}"
        if ((tok < 0) | (tok >= self.V) | (beam < 0) | (beam >= self.nb)).any():
            return False, f"candidate outside the item: tokens {tok.tolist()} beams {beam.tolist()}"
        flat = beam * self.V + tok
        if len(set(flat.tolist())) != self.K:
            return False, f"an entry is returned twice: {flat.tolist()}"
        if not self.keep[flat].all():
            return False, f"entries {flat[~self.keep[flat]].tolist()} are not in the kept set"
        low = self.key[flat] < self.kth1 - self.band
        if low.any():
            return False, (f"entries {flat[low].tolist()} have keys {self.key[flat][low].tolist()} below the (K+1)-th key {self.kth1!r} "
                           f"- band {self.band:.3e}")
        out = self.keep.copy()
        out[flat] = False
        high = out & (self.key > self.kth + self.band)
        if high.any():
            return False, (f"entries {np.flatnonzero(high).tolist()} with keys {self.key[high].tolist()} above the K-th key {self.kth!r} "
                           f"+ band {self.band:.3e} were not returned")
        s = self.s[flat].astype(f64)
        if not (np.abs(score.astype(f64) - s) <= self.band).all():
            return False, f"returned scores {score.tolist()} are not the entries' s {s.tolist()} (band {self.band:.3e})"
        if not (s[:-1] >= s[1:] - self.band).all():
            return False, f"returned order is not non-increasing in s: {s.tolist()} (band {self.band:.3e})"
        tie = score[:-1] == score[1:]
        if (tie & (flat[:-1] >= flat[1:])).any():
            return False, f"equal scores not in ascending flat index: {score.tolist()} {flat.tolist()}"
        return True, ""


# ------------------------------------------------------------------------------------------------ fixed inputs
def beam_scores_for(pattern: str, nb: int, rng) -> np.ndarray:
    """'first': the first step's [0, -1e9, ...]; 'late': running scores of a search some steps in."""
    if pattern == "first":
        b = np.full(nb, -1e9, f32)
        b[0] = 0
        return b
    return np.sort(-rng.uniform(0.5, 6.0, nb))[::-1].astype(f32)


def make_items(kind, S, nb, seed, temperature, top_k, top_p, V=V_MODEL, pattern="late", noise_seed=0, step=0, row0=0):
    """S items of nb rows of ``kind``, coin-flip items rejected and redrawn -> (x f32 [S * nb, V], beam_scores f32 [S * nb],
    [Item], rejected count).  Row s * nb + j draws its noise with the counter row row0 + s * nb + j."""
    rng = np.random.default_rng(seed)
    xs, bss, items, rejected = [], [], [], 0
    while len(items) < S:
        s = len(items)
        x = np.stack([sr.make_row(kind, rng, V) if V >= 64 else rng.normal(0.0, 1.5, V).astype(f32) for _ in range(nb)])
        bs = beam_scores_for(pattern, nb, rng)
        item = Item([BeamRow(x[j], bs[j], temperature, top_k, top_p, noise_seed, row0 + s * nb + j, step) for j in range(nb)])
        if item.is_coin_flip():
            rejected += 1
            assert rejected <= 10 * S + 10
            continue
        xs.append(x)
        bss.append(bs)
        items.append(item)
    return np.concatenate(xs), np.concatenate(bss), items, rejected


def rank_cases():
    """(name, kind, V, ld, nb, S, temperature, top_k, top_p, pattern) of the ranking test: every shape and parameter the issue names.
    top_p < 1 over a flat 50 257-token row is a coin flip by construction (tests/sample_reference.py), so flat rows meet top_p only
    behind a top-k.  The first step's scores [0, -1e9, ...] go with the cases whose first row keeps at least K + 1 tokens: where it
    keeps fewer (V = 3 and 5; a peaked row under top-p) the K-th key lies among the -1e9 rows, whose fp32 keys are 64 apart and tie
    - a coin flip by the rule above, every time."""
    big = (V_MODEL, LD_MODEL)
    cases = []
    for i, kind in enumerate(KINDS):     # the model's shape: every kind, both score patterns, nb 2 / 4 / 16, 1 and 3 items
        nb, S = ((2, 3), (4, 1), (16, 1), (4, 3), (2, 1))[i]
        cases.append((f"{kind}_plain", kind, *big, nb, S, 1.0, 0, 1.0, "first" if i % 2 == 0 else "late"))
        cases.append((f"{kind}_filters", kind, *big, 4, 1, 0.7, 50, 0.9, "late"))
    cases += [
        ("peaked_topk1", "peaked", *big, 4, 1, 1.0, 1, 1.0, "late"),            # top_k = 1 acts as 2
        ("ties_topk2", "ties", *big, 2, 3, 1.0, 2, 1.0, "late"),                # the second value is tied: more than two kept
        ("flat_topk_all", "flat", *big, 2, 1, 4.0, V_MODEL, 1.0, "late"),       # top_k >= V: off
        ("dominant_topp_forced", "dominant", *big, 4, 1, 1.0, 0, 1e-6, "late"), # top_p keeps only the forced two
        ("neg_inf_cold", "neg_inf", *big, 16, 3, 0.25, 0, 0.5, "late"),
        ("unaligned_257", "peaked", 257, 259, 4, 3, 1.0, 0, 1.0, "first"),      # ld % 4 != 0: the scalar load path
        ("unaligned_257_topp", "ties", 257, 261, 16, 1, 2.0, 40, 0.8, "late"),
        ("tiny_3", "flat", 3, 3, 2, 3, 1.0, 0, 1.0, "late"),
        ("tiny_3_nb16", "flat", 3, 4, 16, 1, 1.0, 1, 1.0, "late"),
        ("tiny_5", "flat", 5, 8, 4, 3, 0.5, 3, 0.7, "late"),
        ("tiny_5_nb2", "flat", 5, 5, 2, 1, 1.0, 5, 1e-6, "late"),
    ]
    return cases


CASE_SEED0, CASE_NOISE_SEED, CASE_STEP, CASE_ROW0 = 3000, 0x1234ABCD5678, 5, 7


def case_items(index):
    name, kind, V, ld, nb, S, T, k, p, pattern = rank_cases()[index]
    return make_items(kind, S, nb, CASE_SEED0 + index, T, k, p, V=V, pattern=pattern, noise_seed=CASE_NOISE_SEED, step=CASE_STEP,
                      row0=CASE_ROW0)


# ------------------------------------------------------------------------------------------------ Plackett-Luce
PL_SCORES = np.array([[-0.4, -1.6, -2.3], [-1.1, -1.9, -3.0]])   # nb = 2, V = 3: s of the six continuations
PL_ITEMS, PL_SEED, PL_BOUND = 16384, 1234, 54.64                # 54.64: the 1e-6 upper quantile of chi-square with 14 degrees of freedom


def pl_inputs():
    """Logits and beam scores whose s (temperature 1, no filter) are PL_SCORES: x = log-probabilities of a row, beam score = the
    row's log-sum.  -> (x f32 [PL_ITEMS * 2, 3], beam_scores f32 [PL_ITEMS * 2])."""
    lse = np.log(np.exp(PL_SCORES).sum(1))
    x = np.tile((PL_SCORES - lse[:, None]).astype(f32), (PL_ITEMS, 1))
    return x, np.tile(lse.astype(f32), PL_ITEMS)


def pl_exact():
    """Probability of every unordered 4-of-6 set under sequential draws without replacement, enumerated over ordered draws, with
    the weights the inputs of ``pl_inputs`` really carry (their fp32 s)."""
    x, bs = pl_inputs()
    s = np.concatenate([BeamRow(x[j], bs[j]).s for j in range(2)]).astype(f64)
    w = np.exp(s)
    prob = {}
    for perm in itertools.permutations(range(6), 4):
        p, rest = 1.0, w.sum()
        for i in perm:
            p *= w[i] / rest
            rest -= w[i]
        key = tuple(sorted(perm))
        prob[key] = prob.get(key, 0.0) + p
    return prob


def pl_chi_square(sets):
    """``sets``: per item the 4 chosen flat indices [PL_ITEMS, 4] -> chi-square of the 15 set counts against ``pl_exact``."""
    prob = pl_exact()
    counts = {k: 0 for k in prob}
    for row in np.sort(np.asarray(sets), axis=1).tolist():
        counts[tuple(row)] += 1
    n = len(sets)
    return sum((counts[k] - n * prob[k]) ** 2 / (n * prob[k]) for k in prob)


def pl_reference_sets(seed=PL_SEED, step=0):
    """The reference's own selection on the inputs of ``pl_inputs`` (vectorised over the items) -> flat indices [PL_ITEMS, 4]."""
    x, bs = pl_inputs()
    s = np.stack([BeamRow(x[j], bs[j]).s for j in range(2)]).astype(f64)             # [2, 3]
    g = gumbel64(noise_words(seed, np.arange(2 * PL_ITEMS), step, 3)).reshape(PL_ITEMS, 2, 3)
    key = (s[None] + g).reshape(PL_ITEMS, 6)
    return np.argsort(-key, axis=1, kind="stable")[:, :4]


# ------------------------------------------------------------------------------------------------ the CPU loop
def _margin_hyps(base, sink):
    """An ``oracle.beam_scorer.BeamHypotheses`` like ``base`` that appends to ``sink`` how close each of its comparisons came (the
    decisions are the oracle's own)."""
    from oracle.beam_scorer import BeamHypotheses

    class Recording(BeamHypotheses):
        def add(self, hyp, sum_logprobs):
            if len(self) >= self.num_beams:
                sink.append(abs(sum_logprobs / (hyp.shape[-1] ** self.length_penalty) - self.worst_score))
            super().add(hyp, sum_logprobs)

        def is_done(self, best_sum_logprobs, cur_len):
            if len(self) >= self.num_beams and not self.early_stopping:
                sink.append(abs(self.worst_score - best_sum_logprobs / cur_len ** self.length_penalty))
            return super().is_done(best_sum_logprobs, cur_len)

    return Recording(base.num_beams, base.length_penalty, base.early_stopping)


@torch.no_grad()
def beam_sample(sd, image_hidden_states: torch.Tensor, max_length: int, num_beams: int, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                early_stopping: bool = False, num_return_sequences: int = 1, input_ids: Optional[torch.Tensor] = None,
                attention_mask: Optional[torch.Tensor] = None, stop_below: float = 0.0):
    """Beam-search sampling over ``oracle.language_model._lm_forward_beams`` and ``oracle.beam_scorer.BeamSearchScorer``: the loop
    of ``prompt_beam_reference.beam_search`` with the top-k of the scores replaced by ``Item.select``.  Row r ranks with the
    counter (r, cur_len - 1).  -> (int64 [S * num_return_sequences, L], margins) where margins = dict(key=, s=, scorer=): the
    smallest K-th against (K+1)-th key gap, the smallest gap of adjacent s among the chosen, and the smallest distance of a
    comparison of the scorer (is_done, heap insertion, the final order of an item's hypotheses) over the run - unfinished items
    only.  ``stop_below``: give up - (None, margins) - as soon as a key or s margin falls below it."""
    from oracle import language_model as o_lm
    from oracle.beam_scorer import BeamSearchScorer
    from prompt_beam_reference import expand
    from prompt_reference import positions_from_mask
    EOS = PAD = o_lm.EOS
    S, nb = image_hidden_states.shape[0], int(num_beams)
    if input_ids is None:
        input_ids = torch.full((S, 1), EOS, dtype=torch.int64)
        attention_mask = torch.ones((S, 1), dtype=torch.int64)
    scorer = BeamSearchScorer(batch_size=S, num_beams=nb, length_penalty=1.0, do_early_stopping=early_stopping,
                              num_beam_hyps_to_keep=num_return_sequences)
    sink = []
    scorer._beam_hyps = [_margin_hyps(h, sink) for h in scorer._beam_hyps]
    ids = expand(input_ids.clone(), nb)
    attn = expand(attention_mask.clone().to(torch.int64), nb)
    beam_scores = torch.zeros((S, nb), dtype=torch.float)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    past, cur_len = None, ids.shape[1]
    margins = dict(key=float("inf"), s=float("inf"), scorer=float("inf"))
    while True:
        pos = positions_from_mask(attn)
        inp = ids if past is None else ids[:, -1:]
        if past is not None:
            pos = pos[:, -1:]
        logits, past = o_lm._lm_forward_beams(sd, inp, attn, image_hidden_states, past, pos, nb, "language_model.")
        x = logits[:, -1, :].numpy()
        K = 2 * nb
        scores = torch.zeros((S, K), dtype=torch.float)
        tokens = torch.zeros((S, K), dtype=torch.int64)
        indices = torch.zeros((S, K), dtype=torch.int64)
        for b in range(S):
            if scorer._done[b]:
                continue   # process ignores the candidates of a finished item
            item = Item([BeamRow(x[b * nb + j], beam_scores[b * nb + j].item(), temperature, top_k, top_p, seed, b * nb + j, cur_len - 1)
                         for j in range(nb)])
            sc, tk, bm = item.select()
            margins["key"] = min(margins["key"], float(item.kth - item.kth1))
            margins["s"] = min(margins["s"], float(np.min(sc[:-1].astype(f64) - sc[1:].astype(f64))))
            scores[b], tokens[b], indices[b] = torch.from_numpy(sc.copy()), torch.from_numpy(tk.astype(np.int64)), torch.from_numpy(bm.astype(np.int64))
        if min(margins["key"], margins["s"]) < stop_below:
            return None, margins
        out = scorer.process(ids, scores, tokens, indices, pad_token_id=PAD, eos_token_id=EOS)
        beam_scores = out["next_beam_scores"]
        beam_tok, beam_idx = out["next_beam_tokens"], out["next_beam_indices"]
        ids = torch.cat([ids[beam_idx, :], beam_tok.unsqueeze(-1)], dim=-1)
        attn = torch.cat([attn, attn.new_ones((attn.shape[0], 1))], dim=-1)
        past = [(k.index_select(0, beam_idx), v.index_select(0, beam_idx)) for k, v in past]
        cur_len += 1
        if scorer.is_done or cur_len >= max_length:
            break
    seq = scorer.finalize(ids, beam_scores, tokens, indices, pad_token_id=PAD, eos_token_id=EOS, max_length=max_length)["sequences"]
    for h in scorer._beam_hyps:   # the order finalize returned the hypotheses in
        sc = sorted(s for s, _ in h.beams)
        sink.extend(b - a for a, b in zip(sc[:-1], sc[1:]))
    margins["scorer"] = min(sink) if sink else float("inf")
    return seq, margins


E2E = dict(profile="ragged", feats_seed=4242, S=2, nb=4, L=12, keep=4, temperature=0.8, top_k=40, top_p=0.95, seed0=112, max_walk=40)
_E2E_REF = {}


def e2e_reference(synth_sd, early: bool):
    """The seed walk of the end-to-end test, once per session: from E2E['seed0'] upwards, the first seed at which every decision of
    the CPU run has a margin >= MIN_GAP -> dict(seed, seq, margins, feats, tried)."""
    if early not in _E2E_REF:
        c = E2E
        feats = torch.randn((c["S"], 1024), generator=torch.Generator().manual_seed(c["feats_seed"]))
        sd = synth_sd(c["profile"])
        for i in range(c["max_walk"]):
            seed = c["seed0"] + i
            seq, mg = beam_sample(sd, feats, c["L"], c["nb"], c["temperature"], c["top_k"], c["top_p"], seed, early, c["keep"],
                                  stop_below=MIN_GAP)
            if seq is not None and min(mg.values()) >= MIN_GAP:
                _E2E_REF[early] = dict(seed=seed, seq=seq, margins=mg, feats=feats, tried=i + 1)
                break
        else:
            raise AssertionError(f"no seed in {c['seed0']} .. {c['seed0'] + c['max_walk'] - 1} has every margin >= {MIN_GAP}")
    return _E2E_REF[early]
