"""The token sampler (rgrg_amd/csrc/sample.hip) alone, through rgrg_sample_logits_f32, against the float64 reference and the
acceptance rule of tests/sample_reference.py (inputs: its fixed, seeded generators)."""
import math

import numpy as np
import pytest
import torch

import sample_reference as sr
from conftest import gpu_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x1234_5678_9ABC_DEF0
S_VALUES = (1, 29, 64, 65, 928)


def _eng():
    return gpu_model("bench").engine()


def _device_rows(x, S, ld):
    """[S, ld] device logits: row s = x[s % len(x)], the pitch padding filled with +inf (the kernel must not read it)."""
    buf = torch.full((S, ld), float("inf"), dtype=torch.float32)
    buf[:, :x.shape[1]] = torch.from_numpy(x)[torch.arange(S) % x.shape[0]]
    return buf.to(DEV)


def test_every_draw_is_accepted_over_the_parameter_grid():
    eng = _eng()
    worst = 0.0
    for gi, (kind, T, k, p) in enumerate(sr.parameter_grid()):
        x, rows, _ = sr.make_rows(kind, sr.ROWS_PER_CASE, sr.GRID_SEED0 + gi, T, k, p)
        S = S_VALUES[gi % len(S_VALUES)]
        ld = sr.V_MODEL if gi % 7 == 3 else sr.LD_MODEL          # mostly the decoder's pitch; the unaligned pitch takes scalar loads
        step, row0 = gi % 5, 3 * gi
        logits = _device_rows(x, S, ld)
        tok, lp = eng.sample_logits(logits, T, k, p, SEED, step=step, row0=row0, ld=ld, vocab=sr.V_MODEL)
        tok2, lp2 = eng.sample_logits(logits, T, k, p, SEED, step=step, row0=row0, ld=ld, vocab=sr.V_MODEL)
        assert torch.equal(tok, tok2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32)), "two equal launches differ"
        tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
        for s in range(S):
            row = rows[s % len(rows)]
            ok, why = row.accept(SEED, row0 + s, step, tok[s], lp[s])
            assert ok, (kind, T, k, p, S, s, why)
            worst = max(worst, abs(float(lp[s]) - math.log(row.e[tok[s]] / row.total)))
        if k == 1:
            assert np.array_equal(tok, np.argmax(x, 1)[np.arange(S) % len(rows)]), (kind, "top_k = 1 is not the arg-max")
    print(f"largest |log-prob - float64| over the grid: {worst:.3e}")


def test_top_k_1_is_bit_identical_to_first_occurrence_argmax_with_ties():
    rng = np.random.default_rng(3)
    x = np.round(rng.normal(0, 2, (64, sr.V_MODEL))).astype(np.float32)     # integers: many exact ties at the maximum
    tok, lp = _eng().sample_logits(_device_rows(x, 64, sr.LD_MODEL), 1.0, 1, 1.0, SEED, ld=sr.LD_MODEL, vocab=sr.V_MODEL)
    assert np.array_equal(tok.cpu().numpy(), np.argmax(x, 1))
    ties = (x == x.max(1, keepdims=True)).sum(1)
    assert ties.max() > 1 and np.allclose(lp.cpu().numpy(), -np.log(ties), rtol=0, atol=1e-6)


def test_seed_step_and_row0_change_the_draws_as_the_reference_says():
    x, rows, _ = sr.make_rows("peaked", 4, 77, 1.0, 0, 1.0)
    eng = _eng()
    logits = _device_rows(x, 29, sr.LD_MODEL)
    seen = []
    for seed, step, row0 in ((SEED, 0, 0), (SEED + 1, 0, 0), (SEED, 1, 0), (SEED, 0, 1), (SEED, 0, 2 ** 20), (2 ** 64 - 1, 1000, 0)):
        tok, lp = eng.sample_logits(logits, 1.0, 0, 1.0, seed, step=step, row0=row0, ld=sr.LD_MODEL, vocab=sr.V_MODEL)
        tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
        for s in range(29):
            ok, why = rows[s % 4].accept(seed, row0 + s, step, tok[s], lp[s])
            assert ok, (seed, step, row0, s, why)
        seen.append(tuple(tok))
    assert len(set(seen)) == len(seen)
    # row0 shifts the counters: rows 4.. of a launch at row0 = 0 are rows 0.. of a launch at row0 = 4 (same logits every 4 rows)
    a, _ = eng.sample_logits(logits, 1.0, 0, 1.0, SEED, step=2, row0=0, ld=sr.LD_MODEL, vocab=sr.V_MODEL)
    b, _ = eng.sample_logits(logits, 1.0, 0, 1.0, SEED, step=2, row0=4, ld=sr.LD_MODEL, vocab=sr.V_MODEL)
    assert torch.equal(a[4:], b[:-4])


def _chi2_quantile(df, q_upper):
    """Upper-tail quantile of chi-square(df) by bisection on the regularised incomplete gamma function (series / Lentz)."""
    def sf(x):
        a, xx = df / 2.0, x / 2.0
        if xx < a + 1:
            term = total = 1.0 / a
            n = a
            while abs(term) > 1e-17 * abs(total):
                n += 1
                term *= xx / n
                total += term
            return 1.0 - total * math.exp(-xx + a * math.log(xx) - math.lgamma(a))
        b, c, d = xx + 1 - a, 1e300, 1.0 / (xx + 1 - a)
        h = d
        for i in range(1, 500):
            an = -i * (i - a)
            b += 2
            d = 1.0 / (an * d + b)
            c = b + an / c
            h *= d * c
        return h * math.exp(-xx + a * math.log(xx) - math.lgamma(a))
    lo, hi = float(df), 50.0 * df
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if sf(mid) > q_upper else (lo, mid)
    return hi


def test_distribution_chi_square():
    """200 000 rows with the same logits, the mass on 20 tokens: the draw counts against the exact float64 probabilities.
    Accepted below the 1 - 1e-6 quantile of chi-square(19); seed and inputs are fixed, so the outcome is deterministic."""
    assert abs(_chi2_quantile(10, 0.05) - 18.307) < 1e-2     # table value
    V, N = 256, 200_000
    rng = np.random.default_rng(9)
    x = np.full(V, -np.inf, dtype=np.float32)
    hot = np.sort(rng.choice(V, 20, replace=False))
    x[hot] = rng.uniform(0.0, 3.0, 20).astype(np.float32)
    row = sr.Row(x, 1.0, 0, 1.0)
    logits = torch.from_numpy(x)[None, :].expand(N, V).contiguous().to(DEV)
    tok, _ = _eng().sample_logits(logits, 1.0, 0, 1.0, SEED, step=7, row0=0)
    counts = np.bincount(tok.cpu().numpy(), minlength=V)
    assert counts.sum() == N and counts[~row.keep].sum() == 0
    prob = row.e[hot] / row.total
    stat = float((((counts[hot] - N * prob) ** 2) / (N * prob)).sum())
    bound = _chi2_quantile(19, 1e-6)
    print(f"chi-square statistic {stat:.2f}, bound {bound:.2f}")
    assert stat < bound, (stat, bound)
