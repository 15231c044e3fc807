"""The rolling sampler (roll_sample_kernel, rgrg_amd/csrc/sample.hip) alone, through rgrg_debug_roll_sample: one launch over R
decoder rows whose identity - the sequence a row holds and its length - comes from the rolling state.  Every active row must draw
under the Philox counter (sequence, length - 1) - judged by the acceptance rule of tests/sample_reference.py on its seeded rows,
coin-flip rows already rejected - and write the token to arg[row] and the log-prob to lp[sequence][length]; idle rows and every other
cell must stay as they were."""
import numpy as np
import pytest
import torch

import sample_reference as sr
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED = 0x0F1E_2D3C_4B5A_6978
R_VALUES = (1, 5, 64, 65, 300)
# (temperature, top_k, top_p) and the kind of logits row each meets (flat rows meet top_p only behind a top-k: sample_reference.py)
FILTERS = [(1.0, 0, 1.0, "flat"), (0.7, 50, 0.9, "peaked"), (1.3, 40, 0.8, "ties"), (1.0, 1, 1.0, "neg_inf")]
SEQ_LIMIT, LD_LP = 2 ** 20, 301          # sequence numbers below 2^20, lengths 1 .. 300
LP_SENTINEL, ARG_SENTINEL = 12345.0, -7   # no log-prob is positive, no token negative


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


@pytest.fixture(scope="module")
def lp_buf():
    """[2^20][301] fp32, 1.26 GB: every cell a sequence number below 2^20 can address, so that a write to a wrong cell shows."""
    return torch.empty((SEQ_LIMIT, LD_LP), dtype=torch.float32, device=DEV)


def _state(R, rng):
    """Idle rows (every fourth, never row 0), sequence numbers out of order with the largest and the smallest among them, lengths
    1 .. 300 with both ends."""
    seq = (1 + rng.choice(SEQ_LIMIT - 2, R, replace=False)).astype(np.int32)
    ln = rng.integers(1, LD_LP, R).astype(np.int32)
    seq[0], ln[0] = SEQ_LIMIT - 1, LD_LP - 1
    if R > 2:
        seq[2], ln[2] = 0, 1
    idle = (np.arange(R) % 4) == 1
    seq[idle], ln[idle] = -1, 0
    return seq, ln


def _launch(lib, logits, ld, R, seq, ln, T, k, p, lp_buf):
    arg = torch.full((R,), ARG_SENTINEL, dtype=torch.int32, device=DEV)
    lp_buf.fill_(LP_SENTINEL)
    _hip.check(lib.rgrg_debug_roll_sample(logits.data_ptr(), ld, sr.V_MODEL, R, seq.data_ptr(), ln.data_ptr(), T, k, p, SEED,
                                          arg.data_ptr(), lp_buf.data_ptr(), LD_LP, None), "rgrg_debug_roll_sample")
    return arg, int((lp_buf != LP_SENTINEL).sum())


@pytest.mark.parametrize("T,k,p,kind", FILTERS)
def test_every_active_row_draws_under_its_sequence_counter_and_nothing_else_is_written(lib, lp_buf, T, k, p, kind):
    fi = FILTERS.index((T, k, p, kind))
    x, rows, _ = sr.make_rows(kind, sr.ROWS_PER_CASE, 4000 + fi, T, k, p)
    rng = np.random.default_rng(50 + fi)
    for R in R_VALUES:
        ld = sr.V_MODEL if R == 5 else sr.LD_MODEL          # the unaligned pitch once: scalar loads
        buf = torch.full((R, ld), float("inf"), dtype=torch.float32)   # the pitch padding must not be read
        buf[:, :sr.V_MODEL] = torch.from_numpy(x)[torch.arange(R) % len(rows)]
        logits = buf.to(DEV)
        seq_h, len_h = _state(R, rng)
        seq, ln = torch.from_numpy(seq_h).to(DEV), torch.from_numpy(len_h).to(DEV)
        active = np.flatnonzero(seq_h >= 0)
        cells = (torch.from_numpy(seq_h[active].astype(np.int64)).to(DEV), torch.from_numpy(len_h[active].astype(np.int64)).to(DEV))

        arg, written = _launch(lib, logits, ld, R, seq, ln, T, k, p, lp_buf)
        lp = lp_buf[cells].clone()
        arg2, written2 = _launch(lib, logits, ld, R, seq, ln, T, k, p, lp_buf)
        assert torch.equal(arg, arg2) and torch.equal(lp.view(torch.int32), lp_buf[cells].view(torch.int32)), "two equal launches differ"
        # one cell per active row, no other: every cell of the buffer that is not the sentinel is one of them
        assert written == written2 == len(active) and bool((lp != LP_SENTINEL).all()), (R, written, len(active))
        arg_h, lp_h = arg.cpu().numpy(), lp.cpu().numpy()
        assert (arg_h[seq_h < 0] == ARG_SENTINEL).all(), "an idle row wrote its token"
        assert torch.equal(seq.cpu(), torch.from_numpy(seq_h)) and torch.equal(ln.cpu(), torch.from_numpy(len_h))   # the state is read only
        for i, r in enumerate(active):
            ok, why = rows[r % len(rows)].accept(SEED, int(seq_h[r]), int(len_h[r]) - 1, arg_h[r], lp_h[i])
            assert ok, (kind, T, k, p, R, int(r), int(seq_h[r]), int(len_h[r]), why)
        if k == 1:
            assert np.array_equal(arg_h[active], np.argmax(x, 1)[active % len(rows)]), "top_k = 1 is not the arg-max"


def test_the_counter_is_the_sequence_and_its_length_not_the_row(lib, lp_buf):
    """The same logits in every row: rows that hold the same (sequence, length) draw the same token wherever they stand, and the
    draw is the one rgrg_sample_logits_f32 makes for row0 = sequence, step = length - 1."""
    T, k, p = 1.0, 0, 1.0
    x, rows, _ = sr.make_rows("peaked", 1, 4100, T, k, p)
    R, ld = 9, sr.LD_MODEL
    buf = torch.full((R, ld), float("inf"), dtype=torch.float32)
    buf[:, :sr.V_MODEL] = torch.from_numpy(x)[0]
    logits = buf.to(DEV)
    seq_h = np.array([70000, 3, -1, 70000, 3, 12, 70000, -1, 12], dtype=np.int32)
    len_h = np.array([5, 17, 0, 5, 17, 1, 6, 0, 1], dtype=np.int32)
    arg, written = _launch(lib, logits, ld, R, torch.from_numpy(seq_h).to(DEV), torch.from_numpy(len_h).to(DEV), T, k, p, lp_buf)
    a = arg.cpu().numpy()
    assert written == 4 and a[0] == a[3] and a[1] == a[4] and a[5] == a[8] and a[2] == a[7] == ARG_SENTINEL
    tok = torch.empty((1,), dtype=torch.int32, device=DEV)
    one = torch.empty((1,), dtype=torch.float32, device=DEV)
    for r in (0, 1, 5, 6):
        _hip.check(lib.rgrg_sample_logits_f32(logits.data_ptr(), ld, 1, sr.V_MODEL, T, k, p, SEED, int(len_h[r]) - 1, int(seq_h[r]),
                                              tok.data_ptr(), one.data_ptr(), None), "rgrg_sample_logits_f32")
        assert int(tok) == a[r]
        assert torch.equal(one.view(torch.int32), lp_buf[int(seq_h[r]), int(len_h[r])].reshape(1).view(torch.int32))
    assert len({a[0], a[1], a[5], a[6]}) > 1


def test_refusals(lib):
    z = torch.zeros((4,), dtype=torch.int32, device=DEV)
    one = torch.ones((4,), dtype=torch.int32, device=DEV)
    logits = torch.zeros((1, 64), dtype=torch.float32, device=DEV)
    call = lambda **kw: lib.rgrg_debug_roll_sample(logits.data_ptr(), kw.get("ld", 64), kw.get("V", 64), kw.get("R", 1), z.data_ptr(),   # noqa: E731
                                                   one.data_ptr(), kw.get("T", 1.0), 0, 1.0, 1, z.data_ptr(), None, 0, None)
    assert call() == 0
    assert call(R=0) != 0 and call(ld=63) != 0 and call(T=0.0) != 0 and call(V=0) != 0
