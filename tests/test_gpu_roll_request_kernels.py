"""The kernels behind the requests of a rolling session ALONE.

The retire pass with a request ring, through rgrg_debug_roll_session_step_req, against the numpy model of
tests/rolling_request_reference.py on its hook_cases(R) - own limits 2, L - 1 and L in one pass; a stop token beside another row's EOS;
four stop ids with the hit on the fourth; the cancel flag on a running row, on a sequence that takes its row in this pass and on one
that ended before - at R = 5 and at R = 260, where the rows under test straddle the start of the workgroup's second 256-row pass.
tests/test_rolling_request_reference.py shows that these cases reject the named mutations.  A null ring is rgrg_debug_roll_session_step
bit for bit.

The rolling sampler with a request ring, through rgrg_debug_roll_sample_req: V = 50257, R = 5 - an idle row and four rows that hold
sequences of three requests which differ in temperature, top-k (1 and 0 among them), top-p, seed and q0.  Every row is compared with
the numpy sampler of tests/sample_reference.py evaluated with that row's parameters under the counter (q - q0, len - 1)."""
import numpy as np
import pytest
import torch

import rolling_reference as M
import rolling_request_reference as Q
import rolling_session_reference as S
import sample_reference as sr
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H = 16
LEN_SENTINEL = -99       # (-1 is a length word here: a sequence cut to BOS alone)


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _ring(ring):
    return None if ring is None else torch.from_numpy(np.frombuffer(ring.tobytes(), dtype=np.uint8).copy()).to(DEV)


def _step(lib, entry, st, arg, ids0, lens0, C, n, S_before, submit, handout, retire, R_, L, ring):
    """One call of a session-step hook on copies of the host arrays -> (state, ids, lens) as numpy."""
    dev = {k: _i32(v) for k, v in st.items()}
    ids, lens, a, r = torch.from_numpy(ids0.copy()).to(DEV), _i32(lens0), _i32(arg), _ring(ring)
    args = [_p(dev["seq"]), _p(dev["len"]), _p(dev["tok"]), _p(dev["pos"]), _p(dev["step"]), _p(dev["shared"]), _p(a), _p(ids), None,
            ids0.shape[1], _p(lens), C, n, S_before, submit, handout, retire, R_, L, None, 0, None, 0, 0, H, 0, 0, 0, 0]
    if entry == "rgrg_debug_roll_session_step_req":
        args.append(_p(r))
    _hip.check(getattr(lib, entry)(*args, None), entry)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dev.items()}, ids.cpu().numpy(), lens.cpu().numpy()


def _buffers(C, L, ended):
    ids, lens = np.full((C, L + 1), -1, dtype=np.int64), np.full(C, LEN_SENTINEL, dtype=np.int32)
    for q, ln in ended.items():
        lens[q % C] = ln
    return ids, lens


@pytest.mark.parametrize("R", (5, 260))
@pytest.mark.parametrize("name", ("limits_mixed", "stop_beside_eos", "fourth_stop_id", "cancel_three_ways"))
def test_retire_pass_with_a_request_ring_equals_the_model(lib, name, R):
    case = [c for c in Q.hook_cases(R) if c[0] == name][0]
    _, C, n, S_before, submit, handout, retire, R_, L, st, arg, ring, ended = case
    ids0, lens0 = _buffers(C, L, ended)
    got_st, got_ids, got_lens = _step(lib, "rgrg_debug_roll_session_step_req", st, arg, ids0, lens0, C, n, S_before, submit, handout, retire, R_, L, ring)
    want_st = {k: v.copy() for k, v in st.items()}
    want_ids, want_lens = ids0.copy(), lens0.copy()
    Q.session_step_req(want_st, arg, want_ids, want_lens, None, C, n, S_before, submit, handout, retire, L, ring)
    for k in want_st:
        assert np.array_equal(got_st[k], want_st[k]), (name, R, k, got_st[k][-8:].tolist(), want_st[k][-8:].tolist())
    assert np.array_equal(got_ids, want_ids), (name, R, "ids")
    assert np.array_equal(got_lens, want_lens), (name, R, "lens", got_lens[-12:].tolist(), want_lens[-12:].tolist())
    F = R - 5
    if name == "cancel_three_ways":     # spelled out once: cut at 4 tokens, cut to BOS alone, ended before: intact, flagged and pending: seated
        assert got_lens[F:F + 4].tolist() == [5, -4, -1, 7] and (got_ids[F + 1] == -1).all() and (got_ids[F + 2] == -1).all()
        assert got_st["seq"][F:F + 2].tolist() == [F + 5, F + 6] and got_st["len"][F] == 1 and got_lens[F + 5] == LEN_SENTINEL
    if name == "limits_mixed":
        assert got_lens[F:F + 4].tolist() == [2, L - 1, LEN_SENTINEL, 4]


@pytest.mark.parametrize("name", ("ring_of_5_retire", "two_per_feature_row", "many_rows"))
def test_a_null_ring_is_the_plain_hook_bit_for_bit(lib, name):
    """The same state through rgrg_debug_roll_session_step and through the new hook with req = NULL: every output array equal."""
    case = [c for c in S.hook_cases() if c[0] == name][0]
    _, C, n, S_before, submit, handout, retire, R_, L, st, arg = case
    ids0, lens0 = M.sentinel_output(C, L + 1)
    a = _step(lib, "rgrg_debug_roll_session_step", st, arg, ids0, lens0, C, n, S_before, submit, handout, retire, R_, L, None)
    b = _step(lib, "rgrg_debug_roll_session_step_req", st, arg, ids0, lens0, C, n, S_before, submit, handout, retire, R_, L, None)
    assert all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert not np.array_equal(a[1], ids0)


def test_a_ring_of_session_values_changes_nothing(lib):
    """What rgrg_decoder_roll_submit writes - the session's limit, no stop token, no flag - gives the plain hook's result too."""
    case = [c for c in S.hook_cases() if c[0] == "ring_of_5_retire"][0]
    _, C, n, S_before, submit, handout, retire, R_, L, st, arg = case
    ids0, lens0 = M.sentinel_output(C, L + 1)
    a = _step(lib, "rgrg_debug_roll_session_step", st, arg, ids0, lens0, C, n, S_before, submit, handout, retire, R_, L, None)
    b = _step(lib, "rgrg_debug_roll_session_step_req", st, arg, ids0, lens0, C, n, S_before, submit, handout, retire, R_, L, Q.new_ring(C, L))
    assert all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------ the sampler
V, LD, LD_LP, C_RING = sr.V_MODEL, sr.LD_MODEL, 16, 8
BLOCK = (2.0, 7, 0.5, 999)      # the step's parameter block: must not be read when a ring is given
# three requests: sequences 9 .. 12 (q0 = 9), 13 .. 14 (q0 = 13), 15 .. 16 (q0 = 15) in a ring of 8
REQUESTS = {"a": dict(q0=9, temperature=0.7, top_k=50, top_p=0.9, seed=0x1234_5678_9ABC_DEF0),
            "b": dict(q0=13, temperature=1.0, top_k=1, top_p=1.0, seed=77),
            "c": dict(q0=15, temperature=1.3, top_k=0, top_p=0.8, seed=2 ** 63 + 5)}
ROWS = [(11, 3, "a"), (-1, 0, None), (13, 1, "b"), (16, 7, "c"), (12, 15, "a")]      # (sequence, len, request) of the 5 rows
LP_SENTINEL, ARG_SENTINEL = 12345.0, -7


@pytest.fixture(scope="module")
def sampler_run(lib):
    ring = Q.new_ring(C_RING, 16)
    for q in range(9, 17):
        kw = REQUESTS["a" if q < 13 else "b" if q < 15 else "c"]
        Q.set_request(ring, q, **kw)
    x = np.full((5, LD), np.inf, dtype=np.float32)       # the pitch padding must not be read
    refs = []
    for r, (q, ln, key) in enumerate(ROWS):
        kw = REQUESTS[key or "a"]
        xs, rows, _ = sr.make_rows("peaked" if key != "b" else "ties", 1, 8800 + r, kw["temperature"], kw["top_k"], kw["top_p"])
        x[r, :V] = xs[0]
        refs.append(rows[0])
    logits = torch.from_numpy(x).to(DEV)
    seq, ln = _i32([q for q, _, _ in ROWS]), _i32([n for _, n, _ in ROWS])
    arg = torch.full((5,), ARG_SENTINEL, dtype=torch.int32, device=DEV)
    lp = torch.full((C_RING, LD_LP), LP_SENTINEL, dtype=torch.float32, device=DEV)
    _hip.check(lib.rgrg_debug_roll_sample_req(_p(logits), LD, V, 5, _p(seq), _p(ln), *BLOCK, _p(_ring(ring)), C_RING, _p(arg), _p(lp), LD_LP,
                                              None), "rgrg_debug_roll_sample_req")
    torch.cuda.synchronize()
    return dict(logits=logits, refs=refs, arg=arg.cpu().numpy(), lp=lp.cpu().numpy(), ring=ring)


def _want(run):
    out = []
    for r, (q, ln, key) in enumerate(ROWS):
        if key is not None:
            kw = REQUESTS[key]
            tok, lp = run["refs"][r].draw(kw["seed"], q - kw["q0"], ln - 1)
            out.append((r, q, ln, kw, tok, lp))
    return out


def test_sampler_writes_one_cell_per_active_row(sampler_run):
    arg, lp = sampler_run["arg"], sampler_run["lp"]
    assert arg[1] == ARG_SENTINEL and (arg[[0, 2, 3, 4]] >= 0).all()
    cells = {(q % C_RING, ln) for q, ln, key in ROWS if key}
    assert {(int(i), int(j)) for i, j in zip(*np.nonzero(lp != LP_SENTINEL))} == cells


def test_sampler_rows_are_accepted_by_the_reference_under_their_own_counter(sampler_run):
    """The acceptance rule of tests/sample_reference.py per row - and NOT under the counter row q, the step's block or another
    request's seed, for the rows that draw (top_k != 1)."""
    arg, lp = sampler_run["arg"], sampler_run["lp"]
    for r, q, ln, kw, tok, _ in _want(sampler_run):
        ok, why = sampler_run["refs"][r].accept(kw["seed"], q - kw["q0"], ln - 1, arg[r], lp[q % C_RING, ln])
        assert ok, (r, why)
    assert arg[2] == int(np.argmax(sampler_run["logits"][2, :V].cpu().numpy()))     # top_k = 1: the first-occurrence arg-max, log-prob 0
    assert abs(float(lp[13 % C_RING, 1])) <= 1e-6                                     # one token is kept: q = 1


def test_sampler_tokens_equal_the_numpy_sampler_bit_for_bit(sampler_run):
    for r, q, ln, kw, tok, _ in _want(sampler_run):
        print(f"REQ SAMPLER row {r}: sequence {q} counter ({q - kw['q0']}, {ln - 1}) token {sampler_run['arg'][r]} reference {tok}")
    assert [int(sampler_run["arg"][r]) for r, *_ in _want(sampler_run)] == [tok for *_, tok, _ in _want(sampler_run)]


def test_sampler_logprobs_equal_the_numpy_sampler_bit_for_bit(sampler_run):
    """The fp32 log-prob of every row against the float64 log-prob of the numpy sampler rounded to fp32, as bit patterns."""
    got = np.array([sampler_run["lp"][q % C_RING, ln] for _, q, ln, *_ in _want(sampler_run)], dtype=np.float32)
    want = np.array([lp for *_, lp in _want(sampler_run)], dtype=np.float64).astype(np.float32)
    for (r, *_), g, w in zip(_want(sampler_run), got, want):
        print(f"REQ SAMPLER row {r}: log-prob {float(g)!r} reference {float(w)!r} ulps apart {int(abs(int(g.view(np.int32)) - int(w.view(np.int32))))}")
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_sampler_rows_equal_the_one_row_entry_with_their_parameters(lib, sampler_run):
    """rgrg_sample_logits_f32 for each row with its request's values, row0 = q - q0 and step = len - 1: token and log-prob bits."""
    tok = torch.empty((1,), dtype=torch.int32, device=DEV)
    one = torch.empty((1,), dtype=torch.float32, device=DEV)
    for r, q, ln, kw, _, _ in _want(sampler_run):
        _hip.check(lib.rgrg_sample_logits_f32(sampler_run["logits"][r:].data_ptr(), LD, 1, V, kw["temperature"], kw["top_k"], kw["top_p"],
                                              kw["seed"], ln - 1, q - kw["q0"], _p(tok), _p(one), None), "rgrg_sample_logits_f32")
        assert int(tok) == sampler_run["arg"][r]
        assert one.cpu().numpy().view(np.int32)[0] == sampler_run["lp"][q % C_RING, ln].view(np.int32)


def test_sampler_with_a_null_ring_is_the_plain_hook(lib, sampler_run):
    seq, ln = _i32([3, -1, 0, 6, 2]), _i32([3, 0, 1, 7, 15])
    outs = []
    for entry in ("rgrg_debug_roll_sample", "rgrg_debug_roll_sample_req"):
        arg = torch.full((5,), ARG_SENTINEL, dtype=torch.int32, device=DEV)
        lp = torch.full((7, LD_LP), LP_SENTINEL, dtype=torch.float32, device=DEV)
        extra = (None, 0) if entry.endswith("_req") else ()
        _hip.check(getattr(lib, entry)(_p(sampler_run["logits"]), LD, V, 5, _p(seq), _p(ln), 0.9, 40, 0.95, 20240607, *extra, _p(arg), _p(lp),
                                       LD_LP, None), entry)
        outs.append((arg.cpu(), lp.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    assert int((outs[0][1] != LP_SENTINEL).sum()) == 4 and outs[0][0][1] == ARG_SENTINEL


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_of_both_hooks(lib):
    st = M.new_state(4, 0)
    dev = {k: _i32(v) for k, v in st.items()}
    arg, lens = _i32(np.zeros(4)), _i32(np.zeros(4))
    ids = torch.zeros((4, 8), dtype=torch.int64, device=DEV)

    def step(ring, C=4, L=6):
        return lib.rgrg_debug_roll_session_step_req(_p(dev["seq"]), _p(dev["len"]), _p(dev["tok"]), _p(dev["pos"]), _p(dev["step"]),
                                                    _p(dev["shared"]), _p(arg), _p(ids), None, 8, _p(lens), C, 1, 0, 0, 1, 0, 4, L, None, 0, None,
                                                    0, 0, H, 0, 0, 0, 0, _p(_ring(ring)), None)

    def bad(**kw):
        ring = Q.new_ring(4, 6)
        for k, v in kw.items():
            ring[k][2] = v
        return ring
    assert step(Q.new_ring(4, 6)) == 0 and step(None) == 0
    assert step(bad(max_length=1)) != 0 and b"request ring entry 2" in lib.rgrg_last_error()
    assert step(bad(max_length=7)) != 0          # beyond the row's width
    assert step(Q.new_ring(4, 6), C=0) != 0 and step(Q.new_ring(4, 6), L=1) != 0

    logits = torch.zeros((1, 64), dtype=torch.float32, device=DEV)
    z, one = torch.zeros((4,), dtype=torch.int32, device=DEV), torch.ones((4,), dtype=torch.int32, device=DEV)

    def sample(ring, C=4, **kw):
        return lib.rgrg_debug_roll_sample_req(_p(logits), kw.get("ld", 64), kw.get("V", 64), kw.get("R", 1), _p(z), _p(one), kw.get("T", 1.0), 0,
                                              1.0, 1, _p(_ring(ring)), C, _p(z), None, 0, None)
    assert sample(Q.new_ring(4, 6)) == 0 and sample(None, C=0) == 0
    assert sample(Q.new_ring(4, 6), C=0) != 0
    assert sample(bad(top_p=0.0)) != 0 and sample(bad(top_p=1.5)) != 0 and sample(bad(inv_T=0.0)) != 0 and sample(bad(top_k=-1)) != 0
    assert sample(bad(q0=-1)) != 0
    assert sample(Q.new_ring(4, 6), R=0) != 0 and sample(Q.new_ring(4, 6), ld=63) != 0 and sample(None, T=0.0) != 0
    torch.cuda.synchronize()
