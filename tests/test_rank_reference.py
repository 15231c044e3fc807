"""The rank and arg-max kernel tests without a GPU: every input builder of tests/rank_reference.py really plants what it is named
for, the numpy emulation of each kernel passes the comparison tests/test_gpu_rank_kernels.py asserts with, and each seeded mistake
(a tie given to the higher index, a list one entry too short, a stride's share of the sum dropped, padding not masked, the last
maximum of a tile winning, done_len overwritten, a finished row not given PAD) is REJECTED by that comparison on the inputs the GPU
test uses.  Also the four hooks' symbols and their refusals, which are decided before any launch."""
import numpy as np
import pytest

import group_beam_reference as gbr
import rank_reference as rr
from rgrg_amd import _hip

f32 = np.float32
V = rr.V_MODEL


# ------------------------------------------------------------------------------------------------ the builders plant what they say
def test_case_table_covers_every_builder_per_instantiation():
    cases = rr.row_cases()
    insts = {}
    for b, K, Vc, extra in cases:
        insts.setdefault(rr.instantiation(K), set()).add(b)
    assert set(insts) == {(8, 1024), (16, 1024), (32, 512), (None, 1024)}
    for inst, names in insts.items():
        assert names >= set(rr.ROW_BUILDERS), (inst, names)
    assert {K for _, K, _, _ in cases} == set(rr.NARROW_K + rr.WIDE_K)
    assert {Vc for _, _, Vc, _ in cases} == {1000, 8192, 8193, V}
    assert any(extra for _, _, _, extra in cases)
    assert rr.ld_of(V) == 50272 and rr.ld_of(1000) == 1024 and rr.ld_of(8193) == 8224


@pytest.mark.parametrize("builder,K,Vc,extra", rr.row_cases())
def test_row_builder_plants_its_property(builder, K, Vc, extra):
    x = rr.build_rows(builder, K, Vc, extra)
    R, ld = x.shape
    assert 3 <= R <= 5 and ld == rr.ld_of(Vc, extra) and (ld > Vc or Vc == 8192)
    xv = x[:, :Vc]
    assert (x[:, Vc:] == rr.PAD_VALUE).all() and float(rr.PAD_VALUE) > float(xv.max())     # padding beats the row maximum
    assert (np.isfinite(xv).sum(1) >= K).all()
    ref = rr.row_reference(x, Vc, K)
    T = rr.instantiation(K)[1]
    if builder == "ties":
        for r, (kind, pair) in enumerate(rr.tie_plan(Vc, K)):
            srt = np.sort(xv[r])[::-1]
            if kind == "many":
                assert srt[0] == srt[K + 2] and (ref["tok"][r] == np.flatnonzero(xv[r] == srt[0])[:K]).all()
                continue
            lo, hi = pair
            assert lo < hi < Vc and xv[r, lo] == xv[r, hi]
            if kind == "zeros":
                assert np.signbit(xv[r, lo]) and not np.signbit(xv[r, hi])
                assert lo in ref["tok"][r] and (K < 4 or hi in ref["tok"][r])     # the pair among the winners
                assert K < 4 or list(ref["tok"][r, -2:]) == [lo, hi]
                continue
            assert srt[K - 1] == srt[K] == xv[r, lo]             # the tie straddles the K-th place
            assert ref["tok"][r, K - 1] == lo and hi not in ref["tok"][r]
            if K >= 4:
                assert srt[1] == srt[2] and ref["tok"][r, 1] < ref["tok"][r, 2]
            if kind == "lanes":
                assert hi == lo + 1 and lo // 64 == hi // 64
            if kind == "waves" and Vc > 200:
                assert hi == lo + 64 and lo % 64 == hi % 64 and lo // T == hi // T
            if kind == "halves":
                assert lo < Vc // 2 <= hi
    if builder == "list_limit":
        for r in range(R):
            assert len(set(int(t) % T for t in ref["tok"][r])) == 1              # the winners share one thread's stride
            assert len(set(int(t) // T for t in ref["tok"][r])) == K
    if builder == "last_column":
        assert (ref["tok"][:, 0] == Vc - 1).all() and (ref["tok"][:, K - 1] == Vc - 2).all()
    if builder == "peaked":
        p = np.exp(xv.astype(np.float64) - xv.max(1, keepdims=True))
        assert np.allclose(p.max(1) / p.sum(1), 0.5, atol=1e-3)
        assert ref["tok"][R - 1, 0] == Vc - 1
    if builder == "flat":
        assert xv.min() >= -0.5 and xv.max() <= 0.5
    if builder == "neg_inf":
        lead = rr.leading_neg_inf_threads(x, Vc, T)
        assert min(lead) >= 1 and max(lead) >= T // 4, lead           # some thread's first element is -inf, a later one finite
        if Vc > 4 * T:
            assert np.isfinite(xv[R - 1]).sum() == K + 1
    if builder == "sampler_neg_inf":
        assert min(rr.leading_neg_inf_threads(x, Vc, T)) >= 1
    if builder == "sampler_ties":
        srt = np.sort(xv, 1)[:, ::-1]
        assert (srt[:, 1] == srt[:, 2]).all()


# ------------------------------------------------------------------------------------------------ row ranking: emulation and mistakes
@pytest.mark.parametrize("builder,K,Vc,extra", [c for c in rr.row_cases() if c[2] != V or c[1] in (8, 16, 32, 34)])
def test_row_emulation_passes_the_comparison(builder, K, Vc, extra):
    x = rr.build_rows(builder, K, Vc, extra)
    ref = rr.row_reference(x, Vc, K)
    fails, fig = rr.judge_rows(rr.emulate_row_topk(x, Vc, K), ref, K)
    assert not fails, fails
    if K == 32:
        fails, _ = rr.judge_rows(rr.emulate_row_topk(x, Vc, K, wide=True), ref, K)
        assert not fails, fails


def _rejected(builder, K, Vc, mistake, word, extra=0):
    x = rr.build_rows(builder, K, Vc, extra)
    ref = rr.row_reference(x, Vc, K)
    fails, fig = rr.judge_rows(rr.emulate_row_topk(x, Vc, K, mistake=mistake), ref, K)
    assert any(word in f for f in fails), (mistake, fails)
    return fig


@pytest.mark.parametrize("K", rr.NARROW_K + rr.WIDE_K)
def test_tie_given_to_the_higher_index_is_rejected(K):
    _rejected("ties", K, V, "tie_high", "tokens differ")


@pytest.mark.parametrize("K", [8, 16, 32])
def test_list_one_entry_too_short_is_rejected(K):
    """LIST = K at these three: the dispatch's limit.  A list of K - 1 loses the K-th winner of the shared stride."""
    _rejected("list_limit", K, V, "short_list", "tokens differ")


@pytest.mark.parametrize("K", [8, 16, 32, 34])
def test_dropped_stride_exceeds_the_logsum_bound_tenfold(K):
    fig = _rejected("flat", K, 8192, "drop_stride", "row_logsum")
    print(f"RANK dropped stride K={K} err={fig['err']:.3e} bound={fig['bound']:.3e}")
    assert fig["err"] >= 10 * fig["bound"], fig
    x = rr.build_rows("flat", 2, V)
    ref = rr.row_reference(x, V, 2)
    _, fig = rr.judge_rows(rr.emulate_row_topk(x, V, 2, mistake="drop_stride"), ref, 2)
    assert fig["err"] >= 10 * fig["bound"], fig


@pytest.mark.parametrize("builder,K,Vc,extra", [("flat", 2, V, 0), ("ties", 8, 1000, 37), ("peaked", 32, V, 0), ("last_column", 34, 8193, 0), ("neg_inf", 16, 8193, 0)])
def test_unmasked_padding_is_rejected(builder, K, Vc, extra):
    _rejected(builder, K, Vc, "no_mask", "tokens differ", extra)


def test_leading_neg_inf_as_nan_is_rejected():
    """What beam_row_topk_kernel computed before its fix: NaN in row_logsum fails the comparison (NaN anywhere fails)."""
    x = rr.build_rows("neg_inf", 8, V)
    ref = rr.row_reference(x, V, 8)
    got = rr.emulate_row_topk(x, V, 8)
    got["row_logsum"][1] = np.nan
    fails, _ = rr.judge_rows(got, ref, 8)
    assert any("row_logsum" in f for f in fails)


# ------------------------------------------------------------------------------------------------ item merge
@pytest.mark.parametrize("nb", rr.NARROW_NB + rr.WIDE_NB)
def test_merge_inputs_tie_and_mistake(nb):
    wide = nb > 16
    d = rr.merge_ties(nb, 0, wide=wide)
    K = 2 * nb
    assert d["top_val"].shape == (rr.MERGE_S * nb, rr.row_width(K)) and d["top_tok"][:, :K].max() < V
    for r in range(rr.MERGE_S * nb):       # sorted (value descending, token ascending), tokens distinct
        v, t = d["top_val"][r, :K], d["top_tok"][r, :K]
        assert len(set(t.tolist())) == K
        assert all(v[i] > v[i + 1] or (v[i] == v[i + 1] and t[i] < t[i + 1]) for i in range(K - 1))
    assert list(d["beam_scores"][:nb]) == [0.0] + [-1e9] * (nb - 1)
    ref = rr.merge_reference(d, rr.MERGE_S, nb, V)
    assert not rr.judge_merge(rr.emulate_merge(d, rr.MERGE_S, nb, V), ref)
    st = rr.merge_tie_stats(d, rr.MERGE_S, nb, V)
    if nb >= 2:
        assert st["cross_beam"] > 0 and st["same_token"] > 0, st        # equal scores in two beams; the same token in two beams
    assert rr.judge_merge(rr.emulate_merge(d, rr.MERGE_S, nb, V, mistake="tie_high"), ref)     # nb = 1: ties inside the row
    d2 = rr.merge_random(nb, 0, wide=wide)
    assert not rr.judge_merge(rr.emulate_merge(d2, rr.MERGE_S, nb, V), rr.merge_reference(d2, rr.MERGE_S, nb, V))


@pytest.mark.parametrize("nb", [2, 4, 16])
def test_group_merge_inputs_fit_the_plain_merge(nb):
    d = gbr.merge_inputs(nb, 1)
    ref = rr.merge_reference(d, gbr.MERGE_S, nb, V)
    assert not rr.judge_merge(rr.emulate_merge(d, gbr.MERGE_S, nb, V), ref)
    assert rr.merge_tie_stats(d, gbr.MERGE_S, nb, V)["cross_beam"] > 0


# ------------------------------------------------------------------------------------------------ candidates pass
@pytest.mark.parametrize("Vc", [1, 32, 33, V])
def test_candidate_rows_and_mistakes(Vc):
    x = rr.cand_rows(Vc, 3)
    NT = (Vc + 31) // 32
    assert x.shape == (rr.CAND_ROWS, rr.ld_of(Vc)) and x.shape[1] >= 32 * NT and x.shape[1] % 4 == 0
    assert (x[:, Vc:] == rr.PAD_VALUE).all()
    val, idx = rr.candidates_reference(x, Vc)
    pos = idx - 32 * np.arange(NT)[None, :]
    valid = np.minimum(32, Vc - 32 * np.arange(NT))
    for r in range(32):
        assert (pos[r] == np.minimum(r, valid - 1)).all()        # the maximum at each of the 32 positions, the last valid column included
    if Vc == V:
        assert valid[-1] == 17 and idx[31, -1] == V - 1
        t = x[32, :32 * (NT - 1)].reshape(NT - 1, 32)
        assert ((t == t.max(1, keepdims=True)).sum(1) == 2).all()      # a tie inside every tile
        first, last = t.argmax(1), 31 - t[:, ::-1].argmax(1)
        assert ((last // 4) != (first // 4)).any() and ((last // 4) == (first // 4)).any()     # across and inside a lane's 16 bytes
    assert idx[33].tolist() == (32 * np.arange(NT)).tolist()
    assert val[34, 0] == -np.inf and idx[34, 0] == 0
    assert not rr.judge_candidates(rr.emulate_candidates(x, Vc), (val, idx))
    tok = rr.argmax_reference(val, idx)
    assert tok.tolist() == x[:, :Vc].argmax(1).tolist()           # the two kernels chained are np.argmax
    if Vc % 32:
        assert rr.judge_candidates(rr.emulate_candidates(x, Vc, mistake="no_mask"), (val, idx))
    if Vc >= 32:
        assert rr.judge_candidates(rr.emulate_candidates(x, Vc, mistake="last_max"), (val, idx))


# ------------------------------------------------------------------------------------------------ arg-max and bookkeeping
def _sentinel_ids(S, L):
    return (np.arange(S * L, dtype=np.int64).reshape(S, L) % 1000) + 100000


@pytest.mark.parametrize("NT", rr.ARGMAX_NT)
@pytest.mark.parametrize("S", rr.ARGMAX_S)
def test_argmax_inputs(S, NT):
    d = rr.argmax_inputs(S, NT, 0)
    cv, ci = d["cand_val"], d["cand_idx"]
    assert (np.diff(ci.astype(np.int64), axis=1) > 0).all()
    tok = rr.argmax_reference(cv, ci)
    kinds = [k for k, _ in d["plan"]]
    for s, (kind, pos) in enumerate(d["plan"]):
        if kind == "all_neg_inf":
            assert tok[s] == 0
        elif kind == "eos":
            assert tok[s] == rr.EOS
        else:
            p, q = pos
            assert cv[s, p] == cv[s, q] == cv[s].max() and tok[s] == ci[s, p]
            if kind == "trips" and NT > 256 * rr.ARGMAX_U:
                assert q >= 256 * rr.ARGMAX_U and q % 256 == p % 256        # the tail loop holds the later maximum
            if kind == "waves" and NT > 64:
                assert q == p + 64
    if S >= 5:
        assert {"threads", "waves", "trips", "all_neg_inf", "eos"} <= set(kinds)
        assert 0 < d["finished"].sum() < S
    allf = rr.argmax_inputs(S, NT, 0, all_finish=True)
    assert (rr.argmax_reference(allf["cand_val"], allf["cand_idx"]) == rr.EOS).all()


def test_step_reference_and_mistakes():
    S, L, t = 5, 9, 3
    d = rr.argmax_inputs(S, 257, 0)
    tok = rr.argmax_reference(d["cand_val"], d["cand_idx"])
    ids0 = _sentinel_ids(S, L)
    ref = rr.step_reference(tok, ids0, d["finished"], t, 0)
    ids, fin, step, done_len, sync = ref
    assert (ids[d["finished"] != 0, t + 1] == rr.PAD).all() and (np.delete(ids, t + 1, 1) == np.delete(ids0, t + 1, 1)).all()
    assert step == t + 1 and sync == 0 and done_len == 0 and fin[4] == 1 and fin[0] == 0
    assert rr.judge_step(rr.step_reference(tok, ids0, d["finished"], t, 0, mistake="no_pad"), ref)
    # a batch the step finishes: done_len = t + 2 when it was 0, untouched when already set
    a = rr.argmax_inputs(S, 257, 0, all_finish=True)
    tok = rr.argmax_reference(a["cand_val"], a["cand_idx"])
    assert rr.step_reference(tok, ids0, a["finished"], t, 0)[3] == t + 2
    keep = rr.step_reference(tok, ids0, a["finished"], t, 2)
    assert keep[3] == 2
    assert rr.judge_step(rr.step_reference(tok, ids0, a["finished"], t, 2, mistake="done_len_overwrite"), keep)


# ------------------------------------------------------------------------------------------------ symbols and refusals
EINVAL = -1
HOOKS = ("rgrg_debug_beam_row_topk", "rgrg_debug_beam_merge", "rgrg_debug_logits_candidates", "rgrg_debug_argmax_update")


def test_hooks_are_exported_with_their_signatures():
    lib = _hip.load()
    for name in HOOKS:
        assert name in _hip.SIGNATURES and getattr(lib, name).argtypes == _hip.SIGNATURES[name][1]


def test_null_pointers_are_refused_before_any_launch():
    """RGRG_EINVAL without touching the GPU: these run on a machine that has none."""
    lib = _hip.load()
    assert lib.rgrg_debug_beam_row_topk(None, 1024, 1000, 3, 8, None, None, None, None, None) == EINVAL
    assert lib.rgrg_debug_beam_merge(None, None, None, None, None, 3, 4, V, None, None, None, None, None) == EINVAL
    assert lib.rgrg_debug_logits_candidates(None, 1024, 1000, 3, None, None, None) == EINVAL
    assert lib.rgrg_debug_argmax_update(None, None, 32, None, 8, None, None, None, None, 3, None) == EINVAL
