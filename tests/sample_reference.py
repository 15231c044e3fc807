"""The token sampler's contract (include/rgrg_hip.h "Sampling") restated in float64, the acceptance rule a
device result is judged by, and the fixed inputs of the sampler tests.  Only z_i = x_i * inv_T and u are formed in fp32, as the
kernel forms them; everything else is float64.

Acceptance rule (derived from this reference alone, as tests/attn_reference.py derives its bound).  F_j is the float64
normalised CDF over the kept set in vocabulary order.  A returned token j is accepted iff it is kept and
u in [F_{j-1} - band, F_j + band), band = 8 x max_j |fp32 left-to-right evaluation of F_j - F_j| + 2^-24: 8 is the margin used
everywhere in this repository, 2^-24 the resolution of u.  The returned log-prob must lie within
8 x |fp32 evaluation of log q_j - float64 one| + one fp32 ulp of the largest magnitude that enters it (z_j - max z, the log of
the kept total, 1): an fp32 evaluation subtracts two such numbers and cannot do better than the spacing there.

A row is a coin flip about set membership, not a test of the sampler, when some token's mass-above lies within `band` of
top_p: the generators reject such a row and redraw it (test_sample_reference.py pins the rejection rate below 1 %).
"""
from __future__ import annotations

import math

import numpy as np

MARGIN = 8.0
V_MODEL = 50257
LD_MODEL = 50272           # the decoder's logits pitch (3142 column tiles of 16)
ROWS_PER_CASE, GRID_SEED0 = 6, 1000   # make_rows(kind, ROWS_PER_CASE, GRID_SEED0 + index in parameter_grid(), ...)


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = (int(c) & 0xFFFFFFFF for c in ctr)
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c3 ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c0, c1, c2, c3]


def uniform(seed: int, r: int, t: int, *, word: int = 0, swap: bool = False) -> float:
    """u = (w >> 8) * 2^-24, w = word 0 of Philox4x32-10(key = seed, counter = (r, t, 0, 0)) (word / swap: mutations)."""
    seed &= 0xFFFFFFFFFFFFFFFF
    ctr = (t, r, 0, 0) if swap else (r, t, 0, 0)
    return (philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[word] >> 8) * 2.0 ** -24


class Row:
    """Everything the contract defines for one logits row; `mut` names one deliberate mutation (tests)."""

    def __init__(self, x, temperature=1.0, top_k=0, top_p=1.0, mut=None):
        x = np.asarray(x, dtype=np.float32)
        V = x.shape[0]
        self.x, self.V, self.top_k, self.mut = x, V, int(top_k), mut
        inv_T = np.float32(1.0) / np.float32(temperature)
        if mut == "no_temperature":
            inv_T = np.float32(1.0)
        self.top_p = float(top_p) if isinstance(top_p, np.float64) else float(np.float32(top_p))   # np.float64: taken as is (tests)
        self.z = (x * inv_T).astype(np.float32)
        zmax = self.z.max()
        with np.errstate(invalid="ignore"):
            self.d32 = np.where(self.z == zmax, np.float32(0), self.z - zmax).astype(np.float32)   # what an fp32 evaluation exponentiates
        e_all = np.exp(self.z.astype(np.float64) - np.float64(zmax))
        e_all[self.z == zmax] = 1.0
        self.e_all = e_all
        keep = np.ones(V, dtype=bool)
        if mut == "topp_first":
            keep &= self._top_p_keep(keep)
            keep &= self._top_k_keep()
        else:
            keep &= self._top_k_keep()
            keep &= self._top_p_keep(keep)
        self.keep = keep
        self.e = np.where(keep, e_all, 0.0)
        self.total = float(self.e.sum())
        self.F = np.cumsum(self.e) / self.total
        # the fp32 left-to-right evaluation (np.cumsum is sequential)
        e32 = np.where(keep, np.exp(self.d32), np.float32(0)).astype(np.float32)
        c32 = np.cumsum(e32, dtype=np.float32)
        self.total32 = c32[-1]
        self.band = MARGIN * float(np.abs((c32 / c32[-1]).astype(np.float64) - self.F).max()) + 2.0 ** -24

    def _top_k_keep(self):
        k = self.top_k
        if k <= 0 or k >= self.V:
            return np.ones(self.V, dtype=bool)
        kth = np.partition(self.x, self.V - k)[self.V - k]
        return (self.x > kth) if self.mut == "topk_strict" else (self.x >= kth)

    def mass_above(self, keep):
        """Per token: total probability (re-normalised over `keep`) of the kept tokens with a strictly greater logit."""
        e = np.where(keep, self.e_all, 0.0)
        order = np.argsort(-self.x.astype(np.float64), kind="stable")
        xs, es = self.x[order], e[order]
        excl = np.cumsum(es) - es
        start = np.r_[True, xs[1:] != xs[:-1]]                 # first element of every group of tied logits
        group_first = np.maximum.accumulate(np.where(start, np.arange(self.V), 0))
        above = np.empty(self.V)
        above[order] = excl[group_first]
        return above / e.sum()

    def _top_p_keep(self, keep):
        if self.top_p >= 1.0:
            self.above = None
            return np.ones(self.V, dtype=bool)
        self.above = self.mass_above(keep)
        return (self.above < self.top_p) if self.mut == "topp_strict" else (self.above <= self.top_p)

    # ------------------------------------------------------------------ the draw
    def draw(self, seed, r, t):
        """-> (token, log-prob) of the contract (or of the mutation)."""
        u = 0.0 if self.top_k == 1 else uniform(seed, r, t, word=1 if self.mut == "second_word" else 0, swap=self.mut == "swap_counter")
        if self.mut == "sorted_cdf":
            order = np.argsort(-self.x.astype(np.float64), kind="stable")
            Fs = np.cumsum(self.e[order]) / self.total
            j = int(order[np.searchsorted(Fs, u, side="right")])
        else:
            j = int(np.searchsorted(self.F, u, side="right"))     # first index whose running sum exceeds u x total (F rises at kept tokens only)
        lp = math.log(self.e[j] / self.total)
        if self.mut == "unfiltered_logprob":
            lp = math.log(self.e_all[j] / self.e_all.sum())
        return j, lp

    def accept(self, seed, r, t, tok, logprob):
        """The acceptance rule -> (ok, message)."""
        tok = int(tok)
        u = 0.0 if self.top_k == 1 else uniform(seed, r, t)
        if not (0 <= tok < self.V) or not self.keep[tok]:
            return False, f"token {tok} is not in the kept set"
        lo = (self.F[tok - 1] if tok > 0 else 0.0) - self.band
        hi = self.F[tok] + self.band
        if not (lo <= u < hi):
            return False, f"token {tok}: u = {u!r} outside [{lo!r}, {hi!r}) (band {self.band:.3e})"
        if self.top_k == 1 and tok != int(np.argmax(self.x)):
            return False, f"top_k = 1: token {tok} is not the first-occurrence arg-max {int(np.argmax(self.x))}"
        if logprob is not None:
            lp64 = math.log(self.e[tok] / self.total)
            log_t32 = np.log(np.float32(self.total32))
            lp32 = np.float32(self.d32[tok]) - log_t32
            big = max(abs(float(self.d32[tok])), abs(float(log_t32)), 1.0)
            tol = MARGIN * abs(float(lp32) - lp64) + float(np.spacing(np.float32(big)))
            if not abs(float(logprob) - lp64) <= tol:
                return False, f"token {tok}: log-prob {float(logprob)!r} vs {lp64!r}, |diff| {abs(float(logprob) - lp64):.3e} > {tol:.3e}"
        return True, ""

    def is_coin_flip(self):
        return self.above is not None and bool((np.abs(self.above - self.top_p) <= self.band).any())


# ---------------------------------------------------------------------- fixed inputs
KINDS = ("flat", "peaked", "dominant", "neg_inf", "ties")


def make_row(kind: str, rng: np.random.Generator, V: int = V_MODEL) -> np.ndarray:
    if kind == "flat":
        return rng.normal(0.0, 0.5, V).astype(np.float32)
    if kind in ("peaked", "neg_inf", "ties"):
        x = rng.normal(-8.0, 1.0, V).astype(np.float32)
        hot = rng.choice(V, 20, replace=False)
        x[hot] = rng.uniform(8.0, 14.0, 20).astype(np.float32)
        if kind == "neg_inf":
            x[rng.choice(V, V // 3, replace=False)] = -np.inf
            x[hot[:10]] = rng.uniform(8.0, 14.0, 10).astype(np.float32)
        if kind == "ties":   # exact ties at the 2nd and at the 50th value, spread over the vocabulary
            srt = np.sort(x)[::-1]
            x[rng.choice(np.flatnonzero(x < srt[60]), 3, replace=False)] = srt[1]
            x[rng.choice(np.flatnonzero(x < srt[60]), 4, replace=False)] = srt[49]
        return x
    if kind == "dominant":
        x = rng.normal(0.0, 1.0, V).astype(np.float32)
        x[int(rng.integers(V))] = 40.0
        return x
    raise ValueError(kind)


def make_rows(kind, n, seed, temperature, top_k, top_p, V=V_MODEL):
    """n rows of `kind` for these parameters, coin-flip rows rejected and redrawn -> (x [n,V] fp32, [Row], rejected count)."""
    rng = np.random.default_rng(seed)
    xs, rows, rejected = [], [], 0
    while len(rows) < n:
        x = make_row(kind, rng, V)
        row = Row(x, temperature, top_k, top_p)
        if row.is_coin_flip():
            rejected += 1
            assert rejected <= 10 * n + 10
            continue
        xs.append(x)
        rows.append(row)
    return np.stack(xs), rows, rejected


def parameter_grid():
    """(kind, temperature, top_k, top_p) of the kernel test: every value the contract names, each kind with each filter.
    top_p < 1 over a flat 50 257-token row is a coin flip by construction (neighbouring mass-above values are closer than the
    fp32 noise of the CDF), so flat rows meet top_p only behind a top-k."""
    V = V_MODEL
    grid = []
    for kind in KINDS:
        for k in (0, 1, 2, 50, V, V + 1):
            grid.append((kind, 1.0, k, 1.0))
        for p in (0.9, 0.5, 1e-6):
            grid.append((kind, 1.0, 50 if kind == "flat" else 0, p))
        for T in (0.25, 4.0):
            grid.append((kind, T, 0, 1.0))
        grid.append((kind, 0.25 if kind == "flat" else 4.0, 50, 0.9))
    return grid
