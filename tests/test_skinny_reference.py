"""The reference of tests/skinny_reference.py and the bounds of tests/test_gpu_skinny_gemms.py, checked without a GPU:
  * the host restatements of the layouts (fragment-major activations, both weight packings, the split-K accumulators) equal the
    index formulas of the kernels, element by element;
  * the folded LayerNorm formula equals LayerNorm-then-linear in float64 to 1e-11 relative, and torch's own layer_norm;
  * SENSITIVITY: on the inputs the GPU test uses, every named mutation of the reference, stored as a kernel would store it and
    pushed through the same judge with the same bounds, leaves the bound or breaks the exact check it targets, in EVERY case it
    applies to (the GEMM-value mutations of the vocabulary-sized cases are run on one row tile and 33 rows only: a float64 GEMM
    of 128 x 1024 x 50257 per mutation buys nothing the smaller row counts do not show);
  * the unmutated float32 evaluation - the noise run - passes its own bound in every case.
"""
import pytest
import torch
import torch.nn.functional as F

import skinny_reference as R
from attn_reference import frag_off

F64, F32 = torch.float64, torch.float32
GEMM_MUTATIONS = ("drop_last_chunk_of_wave", "swap_row_halves", "omit_mean_c1", "c1_unrounded_w16", "omit_acc23")


# ------------------------------------------------------------------------------------------------ layouts
def test_fragment_major_layout_is_frag_off():
    for rows, L in ((32, 16), (64, 48), (128, 1024)):
        X = torch.arange(rows * L, dtype=F32).reshape(rows, L)
        flat = R.to_frag(X)
        assert sorted(R.frag_index(rows, L).reshape(-1).tolist()) == list(range(rows * L))   # a permutation
        for r, k in ((0, 0), (15, L - 1), (16, 3), (rows - 1, L - 1), (rows - 17, 5), (rows // 2, L // 2)):
            assert flat[frag_off(r, k, L)] == X[r, k]
        assert torch.equal(R.from_frag(flat, rows, L), X)
    part = R.to_frag(torch.ones(29, 32), tiles=2, fill=-5.0)
    back = R.from_frag(part, 64, 32)
    assert bool((back[:29] == 1).all()) and bool((back[29:] == -5).all())


def test_weight_packings_follow_the_kernels_index_formulas():
    N, K = 37, 64
    W = torch.arange(N * K, dtype=F32).reshape(N, K) + 1.0
    P = R.pack_direct(W).reshape(-1, 4)          # pack_weights16_scaled_kernel: o = (nt * K/16 + kc) * 64 + l
    for o in (0, 5, 63, 64, 200, P.shape[0] - 1):
        l, t = o & 63, o >> 6
        kc, nt = t % (K // 16), t // (K // 16)
        n, k = nt * 16 + (l & 15), kc * 16 + (l >> 4) * 4
        assert torch.equal(P[o], W[n, k:k + 4] if n < N else torch.zeros(4)), o
    P = R.pack_skinny(W).reshape(-1, 4)          # pack_weights_kernel: lane l = (j = l & 31, h = l >> 5)
    for o in (0, 5, 63, 64, 300, P.shape[0] - 1):
        l, t = o & 63, o >> 6
        kc, nt = t % (K // 8), t // (K // 8)
        n, k = nt * 32 + (l & 31), kc * 8 + (l >> 5) * 4
        assert torch.equal(P[o], W[n, k:k + 4] if n < N else torch.zeros(4)), o


def test_accumulator_layout_is_tile_accumulator_half_column_tile():
    M, N = 40, 32
    A0 = torch.arange(M * N, dtype=F32).reshape(M, N) + 1.0
    A1 = -A0
    flat = R.acc_to_flat(A0, A1)
    for row, col, p in ((0, 0, 0), (17, 5, 1), (39, 31, 0), (33, 16, 1)):
        mt, half, lr, nt, lc = row // 32, (row % 32) // 16, row % 16, col // 16, col % 16
        e_in = ((lc >> 2) * 16 + lr) * 4 + (lc & 3)     # skinny_direct.inc: position inside a 16 x 16 fragment block
        off = (((mt * 2 + p) * 2 + half) * (N >> 4) + nt) * 256 + e_in
        assert flat[off] == (A0, A1)[p][row, col]
    b0, b1 = R.acc_from_flat(flat, 2, N)
    assert torch.equal(b0[:M], A0) and torch.equal(b1[:M], A1) and float(b0[M:].abs().max()) == 0.0


def test_prefill_k_split_is_the_decoders():
    assert R.pick_ks(1024, 1024) == 4 and 1024 // (8 * 4 * 8) == 4       # fst0 / fst2: KS = 4, 4 chunks per wave, the reduce kernel
    assert R.pick_ks(16400, 1024) == 1 and R.pick_ks(49152, 1024) == 1   # ukv shapes: 16 chunks per wave
    assert (16400 + 31) // 32 == 513 and 16400 % 32 == 16                # the wide kernel (NT > 512), last tile half valid
    assert (R.VOCAB + 15) // 16 == 3142 and R.VOCAB % 16 == 1 and (R.VOCAB_SMALL + 15) // 16 == 514 and R.VOCAB_SMALL % 16 == 1


# ------------------------------------------------------------------------------------------------ reference against torch
def test_folded_formula_equals_layer_norm_then_linear():
    c = R.fused_case("c_fc", 17)
    x = R.residual_stream(c).double()
    want = F.layer_norm(x, (R.D,), c["g"].double(), c["beta"].double(), eps=R.LN_EPS) @ c["W"].double().t() + c["bias"].double()
    want = F.gelu(want, approximate="tanh")
    got = R.fused_eval(c, F64)["Y"]
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    mean, rstd = R.row_stats(x, F64)
    _, c2 = R.fold_vectors(c["W"], c["g"], c["beta"], c["bias"], F64)
    Wg = c["W"].double() * c["g"].double()          # the identity holds for the exact products; the kernels store fl32(g W)
    folded = F.gelu(rstd * (x @ Wg.t() - mean * Wg.sum(dim=1)) + c2, approximate="tanh")
    assert float((folded - want).abs().max()) <= 1e-11 * float(want.abs().max())


def test_candidates_take_the_lowest_column_and_skip_the_pad_columns():
    Y = torch.tensor([[1.0, 3.0, 3.0, 2.0] + [0.0] * 12 + [-4.0], [5.0] * 16 + [-1.0]])
    val, idx = R.candidates(Y, 17)
    assert val.tolist() == [[3.0, -4.0], [5.0, -1.0]] and idx.tolist() == [[1, 16], [0, 16]]
    _, last = R.candidates(Y, 17, "last_max_wins")
    assert last.tolist() == [[2, 16], [15, 16]]
    val, idx = R.candidates(Y, 17, "pad_columns_in_argmax", torch.tensor([0.0, -2.0]))
    assert val.tolist() == [[3.0, 0.0], [5.0, -1.0]] and idx.tolist() == [[1, 17], [0, 16]]


def test_planted_ties_and_the_low_last_logit_are_in_the_inputs():
    for N, M in ((R.VOCAB_SMALL, 29), (R.VOCAB, 1)):
        c = R.fused_case("lm_head", M, 0, N)
        ev = R.fused_eval(c, F64)
        Y = ev["Y"].float()
        val, idx = R.candidates(Y, N)
        for i, (a, b) in enumerate(R.TIE_PAIRS):
            t = R.TIE_TILE0 + i
            assert torch.equal(Y[:, 16 * t + a], Y[:, 16 * t + b])
            rows = [r for r in range(M) if r != c["const_row"]]
            assert bool((idx[rows, t] == 16 * t + a).all())      # the pair is the tile's maximum, the lower column wins
        assert float(Y[0, N - 1]) < float(ev["vpad"][0]) - 1.0    # a pad column taking part would win the last tile in row 0


# ------------------------------------------------------------------------------------------------ sensitivity and self-check
def _verdict_fused(c, mutations):
    r64, r32 = R.fused_eval(c, F64), R.fused_eval(c, F32)
    own = R.judge_fused(R.as_kernel(c, r32), c, r64, r32)
    assert all(v["ok"] for v in own.values()), (c["name"], own)
    seen = []
    for m in mutations:
        if not R.applies(m, c):
            continue
        ev = r64 if m in ("last_max_wins", "pad_columns_in_argmax") else R.fused_eval(c, F64, m)
        res = R.judge_fused(R.as_kernel(c, ev, m), c, r64, r32)
        assert not all(v["ok"] for v in res.values()), f"{m} stays inside the bound at {c['name']}: {res}"
        seen.append(m)
    return seen


FUSED = list(R.fused_cases())


@pytest.mark.parametrize("form", sorted({f for f, _, _, _ in FUSED}))
def test_fused_mutations_are_rejected_and_the_noise_run_passes(form):
    seen = set()
    for f, M, w16, N in FUSED:
        if f != form:
            continue
        c = R.fused_case(f, M, w16, N)
        big = c["N"] > 8192 and M > 33
        seen.update(_verdict_fused(c, [m for m in R.MUTATIONS if not (big and m in GEMM_MUTATIONS)]))
    want = {m for m in R.MUTATIONS if any(R.applies(m, R.fused_case(f, M, w16, N)) for f, M, w16, N in FUSED if f == form and M <= 33)}
    assert seen >= want, (seen, want)


def test_every_mutation_is_exercised_by_some_form():
    hit = set()
    for f, M, w16, N in FUSED:
        if M not in (33, 65):
            continue
        c = R.fused_case(f, M, w16, N)
        hit.update(m for m in R.MUTATIONS if R.applies(m, c))
    assert hit == set(R.MUTATIONS)
    assert R.MARGIN == 8.0


def test_prefill_mutations_are_rejected_and_the_noise_run_passes():
    for N, K, M, combo in R.prefill_cases():
        if N > 20000:
            continue          # same kernel as N = 16400 at 29 rows: one float64 GEMM of the largest shape is left to the GPU test
        c = R.prefill_case(N, K, M, combo)
        r64, r32 = R.prefill_eval(c, F64), R.prefill_eval(c, F32)
        assert R.compare(r32, r64, r32)["ok"], c["name"]
        for m in ("drop_last_chunk_of_wave", "swap_row_halves"):
            if m == "swap_row_halves" and M <= 16:
                continue
            res = R.compare(R.prefill_eval(c, F64, m).float(), r64, r32)
            assert not res["ok"], f"{m} stays inside the bound at {c['name']}: {res}"


def test_dispatch_expectation_covers_the_three_kernels():
    ran = {(f, M, w16): R.expected_kernel(R.fused_case(f, M, w16, N)) for f, M, w16, N in FUSED if (N or 0) != R.VOCAB_SMALL}
    assert [ran[("attn_proj", M, 0)] for M in R.FUSED_ROWS] == [0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert [ran[("lm_head", M, 0)] for M in (1, 29, 32, 33, 128)] == [2, 2, 2, 0, 0]
    assert all(v == 0 for (f, M, w16), v in ran.items() if f not in ("attn_proj", "lm_head"))
