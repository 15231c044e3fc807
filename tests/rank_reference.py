"""References, input builders and comparisons for the rank and arg-max kernels of greedy and plain beam search, each run alone
through its ``rgrg_debug_*`` hook (tests/test_gpu_rank_kernels.py): ``beam_row_topk_kernel<8,1024>`` / ``<16,1024>`` / ``<32,512>``,
``beam_row_topk_wide_kernel``, ``beam_merge_kernel``, ``beam_merge_wide_kernel`` (decoder_beam.hip), ``logits_candidates_kernel`` and
``argmax_update_kernel`` with ``record_step_token`` (decoder.hip).  TEST INFRASTRUCTURE ONLY.

Contracts (include/rgrg_hip.h):
  row ranking   tokens = ``np.argsort(-x[:V], kind="stable")[:K]`` (value descending, lower token on ties, +0.0 == -0.0), values
                as the bits read, ``row_max`` exact, ``row_logsum`` = log(sum(exp(x - max))) to the project's fp32 bound
                (``attn_reference.compare``: MARGIN * max|ref32 - ref64| + 2^-23 max|ref|, ref32 = plain float32 max / exp / sum / log);
                a -inf logit is zero mass;
  item merge    ``group_beam_reference.merge_reference`` with G = 1 and penalty 0 (``x - 0.0`` keeps the bits; the plain kernel's
                expression ``((v - max) - logsum) + beam_score`` has no multiply a compiler could contract): bits;
  candidates    per 32-column tile the maximum and the FIRST column that holds it, columns >= V left out;
  arg-max       the ``cand_idx`` of the largest ``cand_val`` (lower ``cand_idx`` on ties; a row of -inf ties everywhere: its lowest
                index) and the bookkeeping of ``record_step_token`` over one whole step.

The ``emulate_*`` functions restate the kernels' structure in numpy (strided per-thread candidate lists, per-stride partial sums,
tiles) with a ``mistake`` switch: tests/test_rank_reference.py shows, without a GPU, that the comparisons below reject each one on
the inputs the GPU test uses."""
import numpy as np
import torch

import attn_reference as AR
import group_beam_reference as gbr

f32 = np.float32
V_MODEL = 50257
LD_MODEL = 50272           # the decoder's logits pitch
BEAM_K = gbr.BEAM_K        # width of a candidate row for K <= 32
EOS = PAD = 50256
PAD_VALUE = f32(3e38)      # what the builders put in columns V .. ld - 1: larger than any logit
NO_TOKEN = 0x7fffffff
ARGMAX_U = 13              # candidates a thread of argmax_update_kernel requests up front (256 threads: 3328, a tail loop beyond)
NARROW_K = (2, 8, 10, 16, 18, 32)
WIDE_K = (34, 66)


def instantiation(K):
    """-> (LIST, THREADS) of the kernel the decoder picks for K = 2 num_beams; LIST None: the wide form (no list)."""
    if K <= 8:
        return 8, 1024
    if K <= 16:
        return 16, 1024
    if K <= 32:
        return 32, 512
    return None, 1024


def row_width(K, wide=False):
    return K if (K > BEAM_K or wide) else BEAM_K


def ld_of(V, extra=0):
    return (LD_MODEL if V == V_MODEL else (V + 31) // 32 * 32) + extra


def pad_rows(x, ld, fill=PAD_VALUE):
    """[R, V] -> [R, ld] with the padding columns at ``fill``."""
    R, V = x.shape
    out = np.full((R, ld), fill, f32)
    out[:, :V] = x
    return out


# ---------------------------------------------------------------------------------------------- row ranking: reference
def row_reference(x, V, K):
    """x f32 [R, ld] -> dict(tok i32 [R, K], val f32 [R, K], row_max f32 [R], logsum64 f64 [R], logsum32 f32 [R])."""
    xv = np.ascontiguousarray(x[:, :V])
    R = xv.shape[0]
    tok = np.zeros((R, K), np.int32)
    val = np.zeros((R, K), f32)
    for r in range(R):
        order = np.argsort(-xv[r], kind="stable")[:K]
        tok[r], val[r] = order, xv[r, order]
    m = xv.max(1)
    x64 = xv.astype(np.float64)
    ls64 = np.log(np.exp(x64 - m[:, None].astype(np.float64)).sum(1))
    ls32 = np.log(np.exp(xv - m[:, None], dtype=f32).sum(1, dtype=f32), dtype=f32)
    return dict(tok=tok, val=val, row_max=m.astype(f32), logsum64=ls64, logsum32=ls32)


def judge_rows(got, ref, K):
    """got: dict(tok, val, row_max, row_logsum) of R rows (tok / val at least K wide).  -> (failures [str], figures of the
    ``row_logsum`` comparison).  Tokens, value BITS and row_max (as a value: the two zeros are one maximum) must be equal."""
    fails = []
    if not np.array_equal(got["tok"][:, :K], ref["tok"]):
        r = int(np.flatnonzero((got["tok"][:, :K] != ref["tok"]).any(1))[0])
        fails.append(f"tokens differ, first in row {r}: got {got['tok'][r, :K].tolist()} want {ref['tok'][r].tolist()}")
    if not np.array_equal(np.ascontiguousarray(got["val"][:, :K]).view(np.int32), ref["val"].view(np.int32)):
        fails.append("value bits differ")
    if not np.array_equal(got["row_max"], ref["row_max"]):
        fails.append(f"row_max differs: got {got['row_max'].tolist()} want {ref['row_max'].tolist()}")
    fig = AR.compare(torch.from_numpy(np.asarray(got["row_logsum"], f32)), torch.from_numpy(ref["logsum64"]), torch.from_numpy(ref["logsum32"]))
    if not fig["ok"]:
        fails.append(f"row_logsum: err {fig['err']:.3e} exceeds {fig['bound']:.3e} (noise {fig['noise']:.3e})")
    return fails, fig


def emulate_row_topk(x, V, K, mistake=None, wide=False):
    """The kernels' structure in numpy float32: thread c of THREADS owns columns c, c + THREADS, ...; the register-list forms keep
    its LIST best (ties: the earlier column), the block ranks the kept entries (value descending, lower token on ties); the sum of
    exponentials is the sum of the threads' partial sums.  -> dict(tok, val [R, row_width], row_max, row_logsum).
    mistake: None | "tie_high" (a tie goes to the higher token) | "short_list" (lists of K - 1 entries) | "drop_stride" (one
    thread's share of the sum is lost) | "no_mask" (the padding columns V .. ld - 1 take part)."""
    LIST, T = instantiation(K)
    if wide:
        LIST, T = None, 1024
    if mistake == "short_list":
        LIST = K - 1
    R, ld = x.shape
    n = ld if mistake == "no_mask" else V
    W = row_width(K, wide)
    tok = np.full((R, W), NO_TOKEN, np.int32)
    val = np.full((R, W), -np.inf, f32)
    row_max = np.zeros(R, f32)
    row_logsum = np.zeros(R, f32)
    trips = (n + T - 1) // T
    sign = -1 if mistake == "tie_high" else 1
    for r in range(R):
        xp = np.full(trips * T, -np.inf, f32)
        xp[:n] = x[r, :n]
        idx = np.arange(trips * T)
        if LIST is not None and LIST < trips:
            m2, i2 = xp.reshape(trips, T), idx.reshape(trips, T)
            if sign < 0:
                m2, i2 = m2[::-1], i2[::-1]
            keep = np.argsort(-m2, axis=0, kind="stable")[:LIST]
            cv, ci = np.take_along_axis(m2, keep, 0).ravel(), np.take_along_axis(i2, keep, 0).ravel()
        else:
            cv, ci = xp, idx
        live = cv > -np.inf
        cv, ci = cv[live], ci[live]
        order = np.lexsort((sign * ci, -cv))[:K]
        tok[r, :len(order)], val[r, :len(order)] = ci[order], cv[order]
        m = xp.max()
        part = np.exp(xp - m, dtype=f32).reshape(trips, T).sum(0, dtype=f32)
        if mistake == "drop_stride":
            part[5] = 0
        row_max[r] = m
        row_logsum[r] = np.log(part.sum(dtype=f32), dtype=f32)
    return dict(tok=tok, val=val, row_max=row_max, row_logsum=row_logsum)


# ---------------------------------------------------------------------------------------------- row ranking: builders
def _base(R, V, seed, lo=-3.0, hi=-2.0):
    """Distinct-looking background well below what the builders plant."""
    return np.random.default_rng(seed).uniform(lo, hi, (R, V)).astype(f32)


def rows_flat(R, V, seed):
    """Uniform in [-0.5, 0.5]: every column carries the same order of mass."""
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (R, V)).astype(f32)


def rows_peaked(R, V, seed):
    """One logit per row holds half of the row's mass (the others N(0, 1)); the peak of the last row sits in column V - 1."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (R, V)).astype(f32)
    for r in range(R):
        hot = V - 1 if r == R - 1 else int(rng.integers(V))
        x[r, hot] = -np.inf
        x[r, hot] = f32(np.log(np.exp(x[r].astype(np.float64)).sum()))
    return x


def tie_plan(V, K):
    """What rows_ties plants in its five rows: (kind, the two tied columns)."""
    T = instantiation(K)[1]
    a = 7 if V > 200 else 1
    half = V // 2
    return (("lanes", (a, a + 1)), ("waves", (a, a + 64) if V > a + 64 else (a, a + 2)),
            ("halves", (a + 3, a + 3 + half)), ("zeros", (a + 5, min(a + 5 + T, V - 1))), ("many", None))


def rows_ties(V, K, seed):
    """Five rows, each with an exact tie the ranking has to break by token:
      lanes / waves / halves  K - 1 distinct winners, then ONE value in two columns (neighbouring lanes; the same lane of two waves;
                              the two halves of the row): ranks K - 1 and K, only the lower column is a winner; and (K >= 4) the
                              values at ranks 1 and 2, in two random columns, are equal too;
      zeros                   positive winners and the pair -0.0 (lower column) / +0.0 (higher column) at ranks K - 2 and K - 1
                              (K = 2: ranks 1 and 2, so only -0.0 is a winner), everything else negative;
      many                    K + 3 columns spread over the row hold the row's maximum."""
    rng = np.random.default_rng(seed)
    x = _base(5, V, seed)
    for r, (kind, pair) in enumerate(tie_plan(V, K)):
        if kind == "many":
            cols = np.sort(rng.choice(V, K + 3, replace=False))
            x[r, cols] = f32(1.5)
            continue
        free = np.setdiff1d(np.arange(V), np.asarray(pair))
        if kind == "zeros":
            inside = K >= 4
            nwin = K - 2 if inside else K - 1
            win = rng.choice(free, nwin, replace=False)
            x[r, win] = (1.0 + np.arange(nwin) * 0.25).astype(f32)
            x[r, pair[0]], x[r, pair[1]] = f32(-0.0), f32(0.0)
            continue
        win = rng.choice(free, K - 1, replace=False)
        x[r, win] = (1.0 + np.arange(K - 1) * 0.25).astype(f32)
        x[r, pair[0]] = x[r, pair[1]] = f32(0.5)
        if K >= 4:
            x[r, win[-3]] = x[r, win[-2]]      # ranks 1 and 2 (win[-1] is rank 0)
    return x


def rows_list_limit(R, V, K, seed, threads=None):
    """All K winners of a row in ONE thread's stride: columns j * THREADS + c, j = 0 .. K - 1, values in shuffled order; the row's
    (K + 1)-th value follows in the same stride when the row is long enough.  A list shorter than K loses a winner."""
    T = threads or instantiation(K)[1]
    assert K * T <= V, (K, T, V)
    rng = np.random.default_rng(seed)
    x = _base(R, V, seed)
    for r in range(R):
        c = int(rng.integers(0, min(T, V - (K - 1) * T)))
        cols = np.arange(K) * T + c
        x[r, cols] = rng.permutation((1.0 + np.arange(K) * 0.125).astype(f32))
        if K * T + c < V:
            x[r, K * T + c] = f32(0.75)
    return x


def rows_last_column(R, V, K, seed):
    """The maximum in column V - 1 and the K-th value in column V - 2 (the columns next to the padding)."""
    rng = np.random.default_rng(seed)
    x = _base(R, V, seed)
    for r in range(R):
        win = rng.choice(V - 2, K - 2, replace=False) if K > 2 else np.zeros(0, np.int64)
        x[r, win] = (1.0 + np.arange(K - 2) * 0.25).astype(f32)
        x[r, V - 1] = f32(2.0 + 0.25 * K)
        x[r, V - 2] = f32(0.5)
    return x


def rows_neg_inf(R, V, K, seed, threads=None):
    """Flat rows (uniform in [-0.5, 0.5]) with -inf entries where the one-pass sum meets them FIRST: in a third of the threads the
    first owned column (c < THREADS) is -inf, in half of those the second one too, and a later column of the same thread is finite;
    a sixth of the columns from 3 THREADS on is -inf as well.  Where the row is longer than 4 THREADS, the last row is -inf
    everywhere but in K + 1 columns, one of them the third column of a thread whose first two are -inf.  Every row keeps at least
    K finite entries."""
    T = threads or instantiation(K)[1]
    assert V - T >= T // 3, (V, T)
    rng = np.random.default_rng(seed)
    x = rows_flat(R, V, seed + 1)
    for r in range(R):
        lead = rng.choice(min(T, V - T), T // 3, replace=False)
        x[r, lead] = -np.inf
        two = lead[: len(lead) // 2]
        two = two[two + 2 * T < V]
        x[r, two + T] = -np.inf
        if V > 4 * T:
            rest = np.arange(3 * T, V)
            x[r, rng.choice(rest, len(rest) // 6, replace=False)] = -np.inf
            if r == R - 1:
                keep = np.concatenate([rng.choice(rest, K, replace=False), [two[0] + 2 * T]])
                vals = rng.uniform(-0.5, 0.5, K + 1).astype(f32)
                x[r] = -np.inf
                x[r, keep] = vals
    return x


def leading_neg_inf_threads(x, V, T):
    """Per row: how many threads meet -inf in their first column and a finite value later."""
    n = []
    for r in range(x.shape[0]):
        trips = (V + T - 1) // T
        xp = np.full(trips * T, -np.inf, f32)
        xp[:V] = x[r, :V]
        m = xp.reshape(trips, T)
        n.append(int((np.isinf(m[0]) & np.isfinite(m[1:]).any(0)).sum()))
    return n


ROW_BUILDERS = ("ties", "list_limit", "last_column", "peaked", "flat", "neg_inf")


def row_cases():
    """(builder, K, V, extra pitch) of the GPU test: every builder at least once per instantiation (K = 2, 8 | 10, 16 | 18, 32 | the
    wide form at 34, 66), V = 1000 (fewer columns than threads), 8192 (whole trips of 8 x 1024 / 8 x 512), 8193 (one past) and 50257;
    the list limit wherever K x THREADS columns fit; rows of the sampler's builders; one case on a pitch that is no multiple of 4."""
    cases = []
    for K in NARROW_K + WIDE_K:
        T = instantiation(K)[1]
        first = K in (8, 16, 32, 34)      # the two K of an instantiation take the shapes in turn
        cases += [("ties", K, V_MODEL, 0), ("ties", K, 1000 if first else 8193, 0)]
        cases += [("list_limit", K, V, 0) for V in (V_MODEL, 8192) if K * T <= V]
        cases += [("last_column", K, 8193 if first else 1000, 0), ("last_column", K, V_MODEL, 0)]
        cases += [("peaked", K, V_MODEL if first else 1000, 0), ("flat", K, 8192 if first else V_MODEL, 0), ("neg_inf", K, V_MODEL, 0)]
        if first:
            cases.append(("neg_inf", K, 8193, 0))
    cases += [("neg_inf", 18, 1000, 0), ("ties", 8, 1000, 37), ("sampler_neg_inf", 16, V_MODEL, 0), ("sampler_ties", 32, V_MODEL, 0),
              ("sampler_ties", 34, V_MODEL, 0)]
    return cases


_ROWS = {}


def build_rows(builder, K, V, extra=0):
    """-> x f32 [R, ld] of a case, padding at 3e38 (built once per session, read-only)."""
    key = (builder, K, V, extra)
    if key not in _ROWS:
        seed = 100000 * ROW_SEEDS[builder] + 100 * K + V % 97
        if builder == "ties":
            x = rows_ties(V, K, seed)
        elif builder == "list_limit":
            x = rows_list_limit(4, V, K, seed)
        elif builder == "last_column":
            x = rows_last_column(3, V, K, seed)
        elif builder == "peaked":
            x = rows_peaked(3, V, seed)
        elif builder == "flat":
            x = rows_flat(3, V, seed)
        elif builder == "neg_inf":
            x = rows_neg_inf(4, V, K, seed)
        else:
            import sample_reference as sr
            rng = np.random.default_rng(seed)
            x = np.stack([sr.make_row(builder[len("sampler_"):], rng, V) for _ in range(3)])
        x = pad_rows(x, ld_of(V, extra))
        x.setflags(write=False)
        _ROWS[key] = x
    return _ROWS[key]


ROW_SEEDS = {"ties": 1, "list_limit": 2, "last_column": 3, "peaked": 4, "flat": 5, "neg_inf": 6, "sampler_neg_inf": 7, "sampler_ties": 8}


def first_step_scores(S, nb):
    """Beam scores at the start of a search: 0 in an item's first row, -1e9 in the others."""
    s = np.full((S, nb), -1e9, f32)
    s[:, 0] = 0
    return s.reshape(-1)


# ---------------------------------------------------------------------------------------------- item merge
MERGE_S = 3
NARROW_NB = (1, 2, 4, 5, 8, 16)
WIDE_NB = (17, 33)


def merge_reference(d, S, nb, V):
    return gbr.merge_reference(d["row_max"], d["row_logsum"], d["top_val"], d["top_tok"], d["beam_scores"], S, nb, 1, 0.0, V)


def merge_ties(nb, seed, V=V_MODEL, wide=False):
    """Candidate rows of S = 3 items, K = 2 nb entries sorted (value descending, token ascending) in rows row_width(K) wide, on a
    grid of 1/8 so that sums are exact and scores collide:
      item 0  a first step: every row equal, beam scores [0, -1e9, ...] (the -1e9 rows tie with each other at -1e9 exactly);
      item 1  row 1 is a copy of row 0 with the same beam score - the same token in two beams at equal scores, only the flat index
              beam * V + token separates them - and every other row shares half of row 0's tokens at values shifted by its beam score;
      item 2  equal scores on different tokens inside one row and across rows (values from 12 levels)."""
    rng = np.random.default_rng(1000 * nb + seed)
    S, K = MERGE_S, 2 * nb
    W = row_width(K, wide)
    R = S * nb
    top_val = np.full((R, W), -np.inf, f32)
    top_tok = np.full((R, W), NO_TOKEN, np.int32)
    row_max = np.zeros(R, f32)
    row_logsum = np.zeros(R, f32)
    beam_scores = np.zeros(R, f32)

    def fill(row, vals, toks):
        order = np.lexsort((toks, -np.asarray(vals, np.float64)))
        top_val[row, :K], top_tok[row, :K] = np.asarray(vals, f32)[order], np.asarray(toks)[order]
        row_max[row] = top_val[row, 0]

    pool = rng.choice(V - 1, 3 * K, replace=False)
    pool[0] = V - 1
    v0 = (rng.integers(0, 4 * K, K) / 8).astype(f32)
    t0 = rng.choice(pool, K, replace=False)
    for b in range(nb):          # item 0
        fill(b, v0, t0)
        row_logsum[b] = f32(1.25)
    beam_scores[:nb] = first_step_scores(1, nb)
    for b in range(nb):          # item 1
        r = nb + b
        if b == 1:
            top_val[r], top_tok[r], row_max[r], row_logsum[r], beam_scores[r] = top_val[r - 1], top_tok[r - 1], row_max[r - 1], row_logsum[r - 1], beam_scores[r - 1]
            continue
        if b == 0:
            fill(r, (rng.integers(0, 4 * K, K) / 8).astype(f32), rng.choice(pool, K, replace=False))
            row_logsum[r] = f32(2.5)
            beam_scores[r] = f32(-0.5)
            continue
        shift = f32(rng.integers(1, 5) / 8)
        toks = np.concatenate([top_tok[nb, :nb], rng.choice(np.setdiff1d(pool, top_tok[nb, :K]), K - nb, replace=False)])
        vals = np.concatenate([top_val[nb, :nb] + shift, (rng.integers(0, 4 * K, K - nb) / 8).astype(f32)])
        fill(r, vals, toks)
        row_max[r] = row_max[nb] + shift
        row_logsum[r] = f32(2.5)
        beam_scores[r] = f32(-0.5)
    for b in range(nb):          # item 2
        r = 2 * nb + b
        vals = (rng.integers(0, 12, K) / 8).astype(f32)
        if nb == 1:
            vals[1] = vals[0]      # one beam, two candidates: the tie is inside the row
        fill(r, vals, rng.choice(pool, K, replace=False))
        row_logsum[r] = f32(rng.integers(4, 8) / 8)
        beam_scores[r] = f32(-rng.integers(0, 3) / 8)
    return dict(row_max=row_max, row_logsum=row_logsum, top_val=top_val, top_tok=top_tok, beam_scores=beam_scores)


def merge_random(nb, seed, V=V_MODEL, wide=False):
    """Unquantised values, log-sums and beam scores (every operation of the score rounds), tokens shared between rows."""
    rng = np.random.default_rng(2000 * nb + seed)
    S, K = MERGE_S, 2 * nb
    W = row_width(K, wide)
    R = S * nb
    d = dict(row_max=np.zeros(R, f32), row_logsum=(1 + 3 * rng.random(R)).astype(f32), top_val=np.full((R, W), -np.inf, f32),
             top_tok=np.full((R, W), NO_TOKEN, np.int32), beam_scores=(-4 * rng.random(R)).astype(f32))
    pool = rng.choice(V, 2 * K, replace=False)
    for r in range(R):
        vals = (rng.standard_normal(K) * 2 + 6).astype(f32)
        toks = rng.choice(pool, K, replace=False)
        order = np.lexsort((toks, -vals.astype(np.float64)))
        d["top_val"][r, :K], d["top_tok"][r, :K] = vals[order], toks[order]
        d["row_max"][r] = f32(vals.max() + abs(rng.standard_normal()))
    return d


def merge_tie_stats(d, S, nb, V):
    """What a merge input contains among each item's winners and the first loser: pairs of equal scores in different beams, and of
    those, pairs that carry the same token."""
    K = 2 * nb
    cross = same_tok = 0
    for s in range(S):
        c = []
        for b in range(nb):
            r = s * nb + b
            for k in range(K):
                sc = f32(f32(f32(d["top_val"][r, k] - d["row_max"][r]) - d["row_logsum"][r]) + d["beam_scores"][r])
                c.append((-float(sc), b * V + int(d["top_tok"][r, k]), b, int(d["top_tok"][r, k])))
        c.sort()
        for a, b_ in zip(c[:K], c[1:K + 1]):
            if a[0] == b_[0] and a[2] != b_[2]:
                cross += 1
                same_tok += int(a[3] == b_[3])
    return dict(cross_beam=cross, same_token=same_tok)


def judge_merge(got, ref):
    """got / ref: (score, token, beam).  Scores as bits."""
    fails = []
    if not np.array_equal(got[1], ref[1]):
        fails.append(f"tokens differ: got {got[1].tolist()} want {ref[1].tolist()}")
    if not np.array_equal(got[2], ref[2]):
        fails.append(f"beams differ: got {got[2].tolist()} want {ref[2].tolist()}")
    if not np.array_equal(np.ascontiguousarray(got[0]).view(np.int32), ref[0].view(np.int32)):
        fails.append("score bits differ")
    return fails


def emulate_merge(d, S, nb, V, mistake=None):
    """The merge in numpy float32.  mistake: None | "tie_high" (equal scores go to the higher flat index)."""
    K = 2 * nb
    out_s, out_t, out_b = np.zeros((S, K), f32), np.zeros((S, K), np.int32), np.zeros((S, K), np.int32)
    sign = -1 if mistake == "tie_high" else 1
    for s in range(S):
        rows = np.arange(s * nb, (s + 1) * nb)
        sc = (((d["top_val"][rows, :K] - d["row_max"][rows, None]).astype(f32) - d["row_logsum"][rows, None]).astype(f32)
              + d["beam_scores"][rows, None]).astype(f32).ravel()
        tok = d["top_tok"][rows, :K].astype(np.int64).ravel()
        beam = np.repeat(np.arange(nb), K)
        order = np.lexsort((sign * (beam * V + tok), -sc.astype(np.float64)))[:K]
        out_s[s], out_t[s], out_b[s] = sc[order], tok[order], beam[order]
    return out_s, out_t, out_b


# ---------------------------------------------------------------------------------------------- candidates pass
CAND_ROWS = 35


def cand_rows(V, seed, extra=0):
    """35 logits rows [35, ld], padding at 3e38: row r < 32 has every tile's maximum at position min(r, valid - 1) of the tile (the last
    tile of V = 50257 has 17 valid columns: rows 16 .. 31 put it in the LAST valid column); row 32 repeats every tile's maximum at a
    second, later position (another 16-byte piece where the tile is wide enough, else the next column); row 33 is constant; row 34
    is -inf in a third of its columns and in all of tile 0."""
    rng = np.random.default_rng(seed)
    ld = ld_of(V, extra)
    NT = (V + 31) // 32
    x = rng.uniform(-0.5, 0.5, (CAND_ROWS, V)).astype(f32)
    valid = np.minimum(32, V - 32 * np.arange(NT))
    for r in range(32):
        x[r, 32 * np.arange(NT) + np.minimum(r, valid - 1)] = f32(2.0) + rng.random(NT).astype(f32)
    for t in range(NT):
        n = int(valid[t])
        if n < 2:
            continue
        p = int(rng.integers(0, n - 1))
        q = p + 1 if (t % 2 or p + 4 >= n) else int(rng.integers(p + 4, n))
        x[32, 32 * t + p] = x[32, 32 * t + q] = f32(3.0)
    x[33] = f32(0.25)
    x[34, rng.choice(V, V // 3, replace=False)] = -np.inf
    x[34, :min(32, V)] = -np.inf
    return pad_rows(x, ld)


def candidates_reference(x, V):
    """-> (cand_val f32 [R, NT], cand_idx i32 [R, NT]): per tile the maximum over its columns < V and the first column holding it
    (column 32 * tile when the tile holds nothing above -inf)."""
    R = x.shape[0]
    NT = (V + 31) // 32
    xp = np.full((R, NT * 32), -np.inf, f32)
    xp[:, :V] = x[:, :V]
    t = xp.reshape(R, NT, 32)
    pos = t.argmax(2)
    return t.max(2), (pos + 32 * np.arange(NT)[None, :]).astype(np.int32)


def emulate_candidates(x, V, mistake=None):
    """mistake: None | "last_max" (the LAST maximum of a tile wins) | "no_mask" (columns >= V take part)."""
    R, ld = x.shape
    NT = (V + 31) // 32
    xp = np.full((R, NT * 32), -np.inf, f32)
    n = min(NT * 32, ld) if mistake == "no_mask" else V
    xp[:, :n] = x[:, :n]
    t = xp.reshape(R, NT, 32)
    pos = 31 - t[:, :, ::-1].argmax(2) if mistake == "last_max" else t.argmax(2)
    return t.max(2), (pos + 32 * np.arange(NT)[None, :]).astype(np.int32)


def judge_candidates(got, ref):
    fails = []
    if not np.array_equal(np.ascontiguousarray(got[0]).view(np.int32), ref[0].view(np.int32)):
        fails.append("cand_val bits differ")
    if not np.array_equal(got[1], ref[1]):
        bad = np.argwhere(got[1] != ref[1])[0]
        fails.append(f"cand_idx differs, first at row {bad[0]} tile {bad[1]}: got {got[1][tuple(bad)]} want {ref[1][tuple(bad)]}")
    return fails


# ---------------------------------------------------------------------------------------------- arg-max and bookkeeping
ARGMAX_NT = (1, 197, 256, 257, 1571, 3142, 3328, 3329, 3400)
ARGMAX_S = (1, 5, 300)


def argmax_inputs(S, NT, seed, all_finish=False):
    """cand_val f32 / cand_idx i32 [S, NT] (cand_idx = 32 * position + an offset in 0 .. 31: increasing, as the product's), and the
    step's state.  Row s plants, by s % 6:
      0  the maximum twice, in neighbouring threads (positions p, p + 1);
      1  ... in two waves (p, p + 64);
      2  ... in two trips of one thread (p, p + 256), the later one in the tail loop beyond 13 x 256 when NT reaches it;
      3  every candidate -inf, indices as the candidates pass leaves them for such tiles (32 * position): token 0;
      4  the maximum at the candidate whose index is EOS (position 1570 where the row is long enough, else the last position);
      5  the maximum in the last two positions (NT - 2, NT - 1).
    Rows are finished (PAD whatever the candidates say) for s % 3 == 1 when S > 1.  ``all_finish``: every unfinished row gets the
    EOS plant, so the step finishes the batch and done_len is due."""
    rng = np.random.default_rng(seed + 7 * NT + 1000 * S)
    cv = rng.uniform(-0.5, 0.5, (S, NT)).astype(f32)
    ci = (32 * np.arange(NT)[None, :] + rng.integers(0, 32, (S, NT))).astype(np.int32)
    eos_pos = 1570 if NT > 1570 else NT - 1
    ci[:, eos_pos] = EOS          # 32 * 1570 <= EOS < 32 * 1571: still increasing
    finished = np.array([1 if (S > 1 and s % 3 == 1) else 0 for s in range(S)], np.int32)
    plan = []
    for s in range(S):
        kind = 4 if all_finish else s % 6
        hi = f32(1.0 + 0.125 * (s % 5))
        if kind == 3:
            cv[s] = -np.inf
            ci[s] = 32 * np.arange(NT)      # what the candidates pass leaves for tiles without a value above -inf
            plan.append(("all_neg_inf", ()))
        elif kind == 4:
            cv[s, eos_pos] = hi
            plan.append(("eos", (eos_pos,)))
        else:
            gap = {0: 1, 1: 64, 2: 256, 5: 1}[kind]
            if kind == 2 and NT > 256 * ARGMAX_U:
                p = NT - 1 - 256
            elif kind == 5:
                p = NT - 2
            else:
                p = int(rng.integers(0, max(1, NT - gap)))
            q = p + gap
            p, q = max(p, 0), min(q, NT - 1)
            cv[s, p] = cv[s, q] = hi
            plan.append((("threads", "waves", "trips", "", "", "last")[kind], (p, q)))
    return dict(cand_val=cv, cand_idx=ci, finished=finished, plan=plan)


def argmax_reference(cand_val, cand_idx):
    """-> token i64 [S]: cand_idx of the first largest cand_val (cand_idx increases with position, so the first is the lowest).  A row
    of -inf is a tie of all its candidates: cand_idx[0], which is column 0 behind the candidates pass (an empty tile reports its
    first column)."""
    pos = cand_val.argmax(1)
    return cand_idx[np.arange(cand_val.shape[0]), pos].astype(np.int64)


def step_reference(tokens, ids, finished, step, done_len, mistake=None):
    """record_step_token over all rows of one step.  -> (ids, finished, step, done_len, sync word) afterwards.
    mistake: None | "done_len_overwrite" (written even when already set) | "no_pad" (a finished row keeps its arg-max)."""
    t = int(step)
    ids, fin = ids.copy(), finished.copy()
    tok = np.asarray(tokens, np.int64).copy()
    if mistake != "no_pad":
        tok[fin != 0] = PAD
    ids[:, t + 1] = tok
    fin[tok == EOS] = 1
    if (fin != 0).all() and (done_len == 0 or mistake == "done_len_overwrite"):
        done_len = t + 2
    return ids, fin, t + 1, int(done_len), 0


def judge_step(got, ref):
    """got / ref: (ids, finished, step, done_len, sync).  Every column of ids is compared, so columns the step does not own must
    come back as they were."""
    fails = []
    for name, g, r in zip(("ids", "finished", "step", "done_len", "sync"), got, ref):
        if not np.array_equal(np.asarray(g), np.asarray(r)):
            fails.append(f"{name} differs: got {np.asarray(g).tolist() if np.asarray(g).size < 40 else '...'} want "
                         f"{np.asarray(r).tolist() if np.asarray(r).size < 40 else '...'}")
    return fails
