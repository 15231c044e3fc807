"""The rank and arg-max kernels of greedy and plain beam search on the MI355X, each ALONE through its rgrg_debug_* hook against the
numpy references of tests/rank_reference.py: beam_row_topk_kernel<8,1024> / <16,1024> / <32,512> and beam_row_topk_wide_kernel
(tokens, value bits and row_max equal; row_logsum to the project's fp32 bound against float64), beam_merge_kernel and
beam_merge_wide_kernel (scores as bits, tokens, beams), logits_candidates_kernel (bits and columns per 32-column tile) and
argmax_update_kernel with record_step_token (everything the step writes, and nothing else).  The inputs are the builders of
rank_reference: exact ties, all winners in one thread's stride, ragged shapes, padding at 3e38, -inf logits.  What they plant, and that
the comparisons used here reject a wrong kernel, is shown without a GPU by tests/test_rank_reference.py.

-inf logits: before this test existed, beam_row_topk_kernel returned row_logsum = NaN for a row in which some thread met -inf as
its FIRST element and a finite one later (exp(-inf - -inf) in the one-pass sum; first seen in test_row_ranking[neg_inf-*] of the
register-list forms, the wide form was right).  The kernel now keeps -inf out of the running sum."""
import os

import numpy as np
import pytest
import torch

import group_beam_reference as gbr
import rank_reference as rr
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
V = rr.V_MODEL
EINVAL = -1
SENT_F, SENT_I = -7777.0, -7


def _p(t):
    return t.data_ptr()


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the shared inputs are read-only)


class _wide_form:
    """The wide kernels at K <= 32: the hooks' switch, set for one call."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["RGRG_DEBUG_BEAM_WIDE"] = "1"

    def __exit__(self, *a):
        os.environ.pop("RGRG_DEBUG_BEAM_WIDE", None)


def _report(kernel, case, fig):
    print(f"RANK kernel={kernel} case={case} err={fig['err']:.3e} noise={fig['noise']:.3e} bound={fig['bound']:.3e} used={fig['used']:.3f}")


def _kernel_name(K, wide=False):
    LIST, T = rr.instantiation(K)
    return "beam_row_topk_wide_kernel" if (wide or LIST is None) else f"beam_row_topk_kernel<{LIST},{T}>"


# ------------------------------------------------------------------------------------------------ 1. row ranking
def _row_topk(x_dev, Vc, K, wide=False):
    """One launch on R rows; outputs carry one sentinel row behind them.  -> dict of numpy arrays (R rows) after the sentinel checks."""
    lib = _hip.load()
    R, ld = x_dev.shape
    W = rr.row_width(K, wide)
    row_max = torch.full((R + 1,), SENT_F, dtype=torch.float32, device=DEV)
    row_logsum = torch.full((R + 1,), SENT_F, dtype=torch.float32, device=DEV)
    top_val = torch.full((R + 1, W), SENT_F, dtype=torch.float32, device=DEV)
    top_tok = torch.full((R + 1, W), SENT_I, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with _wide_form(wide):
        _hip.check(lib.rgrg_debug_beam_row_topk(_p(x_dev), ld, Vc, R, K, _p(row_max), _p(row_logsum), _p(top_val), _p(top_tok), None),
                   "rgrg_debug_beam_row_topk")
    torch.cuda.synchronize()
    got = dict(row_max=row_max.cpu().numpy(), row_logsum=row_logsum.cpu().numpy(), val=top_val.cpu().numpy(), tok=top_tok.cpu().numpy())
    assert got["row_max"][R] == SENT_F and got["row_logsum"][R] == SENT_F, "sentinel row of row_max / row_logsum written"
    assert (got["val"][R] == SENT_F).all() and (got["tok"][R] == SENT_I).all(), "sentinel row of the candidate lists written"
    assert (got["val"][:, K:] == SENT_F).all() and (got["tok"][:, K:] == SENT_I).all(), "entries beyond K written"
    return {k: v[:R] for k, v in got.items()}


_REF = {}


def _row_ref(builder, K, Vc, extra):
    key = (builder, K, Vc, extra)
    if key not in _REF:
        _REF[key] = rr.row_reference(rr.build_rows(builder, K, Vc, extra), Vc, K)
    return _REF[key]


@pytest.mark.parametrize("builder,K,Vc,extra", rr.row_cases(), ids=lambda v: str(v))
def test_row_ranking(builder, K, Vc, extra):
    """Tokens, value bits and row_max equal the stable argsort; row_logsum within MARGIN x the float32 reference's own error of the
    float64 one.  K = 32 runs the wide form on the same rows as well: same tokens and values, the same bound."""
    x = rr.build_rows(builder, K, Vc, extra)
    ref = _row_ref(builder, K, Vc, extra)
    x_dev = _dev(x)
    case = f"{builder},K={K},V={Vc},ld={x.shape[1]}"
    got = _row_topk(x_dev, Vc, K)
    fails, fig = rr.judge_rows(got, ref, K)
    _report(_kernel_name(K), case, fig)
    assert not fails, fails
    if K == 32:
        wide = _row_topk(x_dev, Vc, K, wide=True)
        fails, fig = rr.judge_rows(wide, ref, K)
        _report(_kernel_name(K, True), case, fig)
        assert not fails, fails
        assert np.array_equal(wide["tok"], got["tok"]) and np.array_equal(wide["val"].view(np.int32), got["val"].view(np.int32))


def test_row_ranking_refusals():
    """Return codes only: every call is refused before a launch."""
    lib = _hip.load()
    x = torch.zeros((3, 1024), dtype=torch.float32, device=DEV)
    f = torch.zeros((4 * 32,), dtype=torch.float32, device=DEV)
    i = torch.zeros((4 * 32,), dtype=torch.int32, device=DEV)
    ok = [_p(x), 1024, 1000, 3, 8, _p(f), _p(f), _p(f), _p(i), None]
    for pos in (0, 5, 6, 7, 8):
        bad = list(ok)
        bad[pos] = None
        assert lib.rgrg_debug_beam_row_topk(*bad) == EINVAL
    for pos, v in ((1, 999), (2, 0), (3, 0), (4, 0), (4, 1), (4, 7), (4, 1002), (4, -2)):      # ld < V, V, rows, K < 2, odd K, K > V
        bad = list(ok)
        bad[pos] = v
        assert lib.rgrg_debug_beam_row_topk(*bad) == EINVAL, (pos, v)
    assert lib.rgrg_debug_beam_row_topk(*ok) == 0


# ------------------------------------------------------------------------------------------------ 2. item merge
def _merge(d, S, nb, Vc, wide=False):
    lib = _hip.load()
    K = 2 * nb
    dev = {k: _dev(v) for k, v in d.items()}
    scratch = torch.full((S + 1, nb * K), SENT_F, dtype=torch.float32, device=DEV)
    out_s = torch.full((S + 1, K), SENT_F, dtype=torch.float32, device=DEV)
    out_t = torch.full((S + 1, K), SENT_I, dtype=torch.int32, device=DEV)
    out_b = torch.full((S + 1, K), SENT_I, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with _wide_form(wide):
        _hip.check(lib.rgrg_debug_beam_merge(_p(dev["row_max"]), _p(dev["row_logsum"]), _p(dev["top_val"]), _p(dev["top_tok"]),
                                             _p(dev["beam_scores"]), S, nb, Vc, _p(scratch), _p(out_s), _p(out_t), _p(out_b), None),
                   "rgrg_debug_beam_merge")
    torch.cuda.synchronize()
    s, t, b = out_s.cpu().numpy(), out_t.cpu().numpy(), out_b.cpu().numpy()
    assert (s[S] == SENT_F).all() and (t[S] == SENT_I).all() and (b[S] == SENT_I).all(), "sentinel row written"
    assert (scratch[S] == SENT_F).all(), "sentinel row of the score scratch written"
    return s[:S], t[:S], b[:S]


@pytest.mark.parametrize("kind", ["ties", "random", "group_inputs"])
@pytest.mark.parametrize("nb", rr.NARROW_NB + rr.WIDE_NB)
def test_item_merge(nb, kind):
    """S = 3, V = 50257: scores as bits, tokens and beams equal merge_reference with one group and no penalty.  group_inputs: what
    the group merge's test feeds it (rows 32 wide: up to 16 beams; wider beams take the random builder's second seed)."""
    S = rr.MERGE_S
    if kind == "ties":
        d = rr.merge_ties(nb, 0, wide=nb > 16)
    elif kind == "random":
        d = rr.merge_random(nb, 0, wide=nb > 16)
    else:
        d = gbr.merge_inputs(nb, 1) if nb <= 16 else rr.merge_random(nb, 1, wide=True)
    ref = rr.merge_reference(d, S, nb, V)
    fails = rr.judge_merge(_merge(d, S, nb, V), ref)
    assert not fails, fails
    if nb == 16:      # K = 32: the wide form on the same lists (rows 32 = K wide)
        fails = rr.judge_merge(_merge(d, S, nb, V, wide=True), ref)
        assert not fails, fails


@pytest.mark.parametrize("nb", [4, 17])
def test_row_ranking_chained_with_merge(nb):
    """The row hook's own outputs go into the merge hook and into the numpy merge: bit equal.  Rows: flat, row 1 of every item a copy
    of row 0 (the same token at the same score in two beams), a first step's beam scores in item 0."""
    S, K = rr.MERGE_S, 2 * nb
    R = S * nb
    x = rr.rows_flat(R, V, 900 + nb).copy()
    for s in range(S):
        x[s * nb + 1] = x[s * nb]
    x = rr.pad_rows(x, rr.LD_MODEL)
    rows = _row_topk(_dev(x), V, K)
    scores = (-np.random.default_rng(nb).integers(1, 8, R) / 8).astype(np.float32)
    scores[:nb] = rr.first_step_scores(1, nb)
    for s in range(1, S):
        scores[s * nb] = scores[s * nb + 1] = 0.0      # the two equal rows lead their item: the flat rows' values lie within 1e-4
    d = dict(row_max=rows["row_max"], row_logsum=rows["row_logsum"], top_val=rows["val"], top_tok=rows["tok"], beam_scores=scores)
    ref = rr.merge_reference(d, S, nb, V)
    assert rr.merge_tie_stats(d, S, nb, V)["same_token"] > 0
    fails = rr.judge_merge(_merge(d, S, nb, V), ref)
    assert not fails, fails


def test_item_merge_refusals():
    lib = _hip.load()
    f = torch.zeros((3 * 4 * 32,), dtype=torch.float32, device=DEV)
    i = torch.zeros((3 * 4 * 32,), dtype=torch.int32, device=DEV)
    ok = [_p(f), _p(f), _p(f), _p(i), _p(f), 3, 4, V, _p(f), _p(f), _p(i), _p(i), None]
    for pos in (0, 1, 2, 3, 4, 8, 9, 10, 11):
        bad = list(ok)
        bad[pos] = None
        assert lib.rgrg_debug_beam_merge(*bad) == EINVAL, pos
    for pos, v in ((5, 0), (5, 65536), (6, 0), (6, -1), (7, 7)):      # S outside 1 .. 65535, nb < 1, V < 2 nb
        bad = list(ok)
        bad[pos] = v
        assert lib.rgrg_debug_beam_merge(*bad) == EINVAL, (pos, v)


# ------------------------------------------------------------------------------------------------ 3. candidates pass
def _candidates(x_dev, Vc):
    lib = _hip.load()
    R, ld = x_dev.shape
    NT = (Vc + 31) // 32
    cv = torch.full((R + 1, NT), SENT_F, dtype=torch.float32, device=DEV)
    ci = torch.full((R + 1, NT), SENT_I, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    _hip.check(lib.rgrg_debug_logits_candidates(_p(x_dev), ld, Vc, R, _p(cv), _p(ci), None), "rgrg_debug_logits_candidates")
    torch.cuda.synchronize()
    assert (cv[R] == SENT_F).all() and (ci[R] == SENT_I).all(), "sentinel row written"
    return cv[:R], ci[:R]


def _argmax_update(cv, ci, ids, finished, step, done_len):
    """One launch on device candidates; host state in, host state out: (ids, finished, step, done_len, sync)."""
    lib = _hip.load()
    S, NT = cv.shape
    ids_d, fin_d = _dev(ids), _dev(finished)
    st = torch.tensor([step, done_len, 0, SENT_I], dtype=torch.int32, device=DEV)      # step, done_len, sync, a sentinel behind them
    torch.cuda.synchronize()
    _hip.check(lib.rgrg_debug_argmax_update(_p(cv), _p(ci), NT, _p(ids_d), ids.shape[1], _p(fin_d), _p(st), _p(st) + 4, _p(st) + 8, S, None),
               "rgrg_debug_argmax_update")
    torch.cuda.synchronize()
    w = st.cpu().numpy()
    assert w[3] == SENT_I
    return ids_d.cpu().numpy(), fin_d.cpu().numpy(), int(w[0]), int(w[1]), int(w[2])


def _sentinel_ids(S, L):
    return (np.arange(S * L, dtype=np.int64).reshape(S, L) % 1000) + 100000


@pytest.mark.parametrize("Vc,extra", [(1, 0), (32, 0), (33, 0), (33, 32), (V, 0)])
def test_candidates_pass(Vc, extra):
    """35 rows: the tile maximum at each of the 32 positions (the last valid column of the ragged tile included), ties inside a tile,
    a constant row, -inf, padding at 3e38.  cand_val bits and cand_idx equal the per-tile first maximum; chained with the arg-max
    kernel the token is np.argmax of the row."""
    x = rr.cand_rows(Vc, 3, extra)
    ref = rr.candidates_reference(x, Vc)
    cv, ci = _candidates(_dev(x), Vc)
    fails = rr.judge_candidates((cv.cpu().numpy(), ci.cpu().numpy()), ref)
    assert not fails, fails
    S, L, t = x.shape[0], 6, 2
    ids0, fin0 = _sentinel_ids(S, L), np.zeros(S, np.int32)
    got = _argmax_update(cv.contiguous(), ci.contiguous(), ids0, fin0, t, 0)
    tok = x[:, :Vc].argmax(1)
    assert got[0][:, t + 1].tolist() == tok.tolist()
    fails = rr.judge_step(got, rr.step_reference(tok, ids0, fin0, t, 0))
    assert not fails, fails


def test_candidates_pass_refusals():
    lib = _hip.load()
    x = torch.zeros((3, 1028), dtype=torch.float32, device=DEV)
    f = torch.zeros((3 * 33,), dtype=torch.float32, device=DEV)
    i = torch.zeros((3 * 33,), dtype=torch.int32, device=DEV)
    ok = [_p(x), 1024, 1000, 3, _p(f), _p(i), None]
    for pos in (0, 4, 5):
        bad = list(ok)
        bad[pos] = None
        assert lib.rgrg_debug_logits_candidates(*bad) == EINVAL, pos
    # ld < V; ld < 32 NT (V = 1000: 1024); ld % 4; a pointer 4 bytes off 16-byte alignment; V < 1; rows < 1
    for pos, v in ((1, 996), (1, 1000), (1, 1008), (1, 1026), (0, _p(x) + 4), (2, 0), (3, 0)):
        bad = list(ok)
        bad[pos] = v
        assert lib.rgrg_debug_logits_candidates(*bad) == EINVAL, (pos, v)
    assert lib.rgrg_debug_logits_candidates(*ok) == 0


# ------------------------------------------------------------------------------------------------ 4. arg-max and bookkeeping
@pytest.mark.parametrize("NT", rr.ARGMAX_NT)
@pytest.mark.parametrize("S", rr.ARGMAX_S)
def test_argmax_update(S, NT):
    """Two launches back to back on one state (the sync word of the first serves the second): a step with ties across threads, waves
    and trips (the tail loop beyond 3328 candidates included), a row of -inf, an EOS row and finished rows, then a step in which every
    row still open takes EOS - done_len = t + 2 when it was 0, untouched when already set.  Everything record_step_token writes
    equals the numpy step; every other column of ids comes back as it was."""
    L, t = 8, 3
    a, b = rr.argmax_inputs(S, NT, 0), rr.argmax_inputs(S, NT, 0, all_finish=True)
    cva, cia, cvb, cib = _dev(a["cand_val"]), _dev(a["cand_idx"]), _dev(b["cand_val"]), _dev(b["cand_idx"])
    toka, tokb = rr.argmax_reference(a["cand_val"], a["cand_idx"]), rr.argmax_reference(b["cand_val"], b["cand_idx"])
    for done0 in (0, 2):
        ids0 = _sentinel_ids(S, L)
        got1 = _argmax_update(cva, cia, ids0, a["finished"], t, done0)
        ref1 = rr.step_reference(toka, ids0, a["finished"], t, done0)
        fails = rr.judge_step(got1, ref1)
        assert not fails, (done0, fails)
        got2 = _argmax_update(cvb, cib, got1[0], got1[1], got1[2], got1[3])
        ref2 = rr.step_reference(tokb, ref1[0], ref1[1], ref1[2], ref1[3])
        fails = rr.judge_step(got2, ref2)
        assert not fails, (done0, fails)
        assert ref2[2] == t + 2 and (ref2[1] == 1).all() and ref2[3] == (2 if done0 else (t + 3 if ref1[3] == 0 else t + 2))


def test_argmax_update_refusals():
    lib = _hip.load()
    f = torch.zeros((3 * 32,), dtype=torch.float32, device=DEV)
    i = torch.zeros((3 * 32,), dtype=torch.int32, device=DEV)
    ids = torch.zeros((3, 8), dtype=torch.int64, device=DEV)
    w = torch.zeros((4,), dtype=torch.int32, device=DEV)
    ok = [_p(f), _p(i), 32, _p(ids), 8, _p(i), _p(w), _p(w) + 4, _p(w) + 8, 3, None]
    for pos in (0, 1, 3, 5, 6, 7, 8):
        bad = list(ok)
        bad[pos] = None
        assert lib.rgrg_debug_argmax_update(*bad) == EINVAL, pos
    for pos, v in ((2, 0), (9, 0), (9, 65536), (4, 1)):      # NT < 1, S outside 1 .. 65535, no column step + 1
        bad = list(ok)
        bad[pos] = v
        assert lib.rgrg_debug_argmax_update(*bad) == EINVAL, (pos, v)
    w[0] = 7                                                     # *step = 7 on ids 8 wide: column 8 does not exist
    torch.cuda.synchronize()
    assert lib.rgrg_debug_argmax_update(*ok) == EINVAL
    w[0] = -1
    torch.cuda.synchronize()
    assert lib.rgrg_debug_argmax_update(*ok) == EINVAL
