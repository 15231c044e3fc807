"""What a rolling session enqueues around a step - submit-init, the hand-out-only pass, retire, refill - ALONE through
rgrg_debug_roll_session_step, on buffers that show every write (rolling_reference.sentinel_output), against the numpy model of
tests/rolling_session_reference.py on its hook_cases(), which tests/test_rolling_session_reference.py shows to reject the named
mutations: a ring of 5 whose rows wrap inside one hand-out, two sequences per feature row on three ukv ring rows, the hand-out-only
pass over active and idle rows, the submit-init alone, and 600 rows (three passes of the workgroup) with sequence numbers beyond a
ring of 1024."""
import numpy as np
import pytest
import torch

import attn_reference as R
import rolling_reference as M
import rolling_session_reference as S
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = torch.float32
H = 16
D = H * 64
LP_SENTINEL = -7.0


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _run(lib, case, with_lp=False, kv=None, ukv=None, n_layer=0, T_slots=0, kv16=0, fp16=0):
    name, C, n, S_before, submit, handout, retire, R_, L, st, arg = case
    ids0, lens0 = M.sentinel_output(C, L + 1)
    lp0 = np.full((C, L + 1), LP_SENTINEL, dtype=np.float32) if with_lp else None
    dev = {k: _i32(v) for k, v in st.items()}
    ids, lens, a = torch.from_numpy(ids0).to(DEV), _i32(lens0), _i32(arg)
    lp = torch.from_numpy(lp0).to(DEV) if with_lp else None
    kv_stride = R_ * H * T_slots * 64
    _hip.check(lib.rgrg_debug_roll_session_step(
        _p(dev["seq"]), _p(dev["len"]), _p(dev["tok"]), _p(dev["pos"]), _p(dev["step"]), _p(dev["shared"]), _p(a), _p(ids), _p(lp), L + 1,
        _p(lens), C, n, S_before, submit, handout, retire, R_, L, _p(ukv), 0 if ukv is None else ukv.shape[1], _p(kv), 2 * kv_stride,
        kv_stride, H, T_slots, n_layer, kv16, fp16, None), "rgrg_debug_roll_session_step")
    torch.cuda.synchronize()
    want_st = {k: v.copy() for k, v in st.items()}
    want_ids, want_lens = M.sentinel_output(C, L + 1)
    want_lp = lp0.copy() if with_lp else None
    refills = S.session_step(want_st, arg, want_ids, want_lens, want_lp, C, n, S_before, submit, handout, retire, L)
    for k in want_st:
        assert np.array_equal(dev[k].cpu().numpy(), want_st[k]), (name, k, dev[k].cpu().tolist(), want_st[k].tolist())
    assert np.array_equal(ids.cpu().numpy(), want_ids), (name, "ids", ids.cpu().tolist(), want_ids.tolist())
    assert np.array_equal(lens.cpu().numpy(), want_lens), (name, "lens")
    if with_lp:
        assert np.array_equal(lp.cpu().numpy(), want_lp), (name, "lp")
    return refills, dev, ids, lens, want_st


@pytest.mark.parametrize("case", S.hook_cases(), ids=lambda c: c[0])
def test_session_step_equals_the_model(lib, case):
    _run(lib, case)


def test_slots_wrap_inside_one_handout(lib):
    case = [c for c in S.hook_cases() if c[0] == "slots_wrap_in_one_handout"][0]
    (a, b), _, ids, lens, _ = _run(lib, case)
    assert [(r, q) for r, q, _ in a] == [(1, 8), (3, 9), (4, 10)] and b == []
    rows = ids.cpu()
    assert rows[3, 0] == M.BOS and rows[4, 0] == M.BOS and rows[0, 0] == M.BOS       # 8, 9, 10 -> ring rows 3, 4, 0
    assert rows[1, 3] == M.EOS and lens.cpu()[1] == 4                                  # 6 (ring row 1) ended in the retire pass
    assert (rows[2, [0, 1]] == -1).all() and rows[2, 2] == 777                         # 7: its next token, nothing else


def test_handout_only_pass_touches_no_active_row(lib):
    case = [c for c in S.hook_cases() if c[0] == "handout_only_mixed"][0]
    name, C, n, S_before, submit, handout, retire, R_, L, st, arg = case
    (a, b), dev, ids, lens, _ = _run(lib, case)
    active = st["seq"] >= 0
    for k in S.ROW_KEYS:
        assert np.array_equal(dev[k].cpu().numpy()[active], st[k][active]), k
    assert (ids.cpu() == -1).all() and (lens.cpu() == -1).all()                        # no append, no retire, although arg is EOS
    assert [(r, q) for r, q, _ in a] == [(1, 7), (3, 8)] and dev["seq"].cpu().tolist() == [4, 7, 6, 8, 5, -1]
    assert dev["shared"].cpu().tolist() == [9, 5, 2, 3]                                 # no step counted


def test_submit_init_writes_exactly_the_new_rows(lib):
    case = [c for c in S.hook_cases() if c[0] == "submit_init_only"][0]
    name, C, n, S_before, submit, handout, retire, R_, L, st, arg = case
    _, dev, ids, lens, _ = _run(lib, case, with_lp=True)
    rows, ln = ids.cpu(), lens.cpu()
    new = sorted(q % C for q in range(S_before, S_before + submit))
    assert new == [0, 5, 6, 7]
    for r in range(C):
        if r in new:
            assert rows[r, 0] == M.BOS and (rows[r, 1:L] == M.PAD).all() and rows[r, L] == -1 and ln[r] == 0
        else:
            assert (rows[r] == -1).all() and ln[r] == -1
    for k in S.ROW_KEYS:
        assert np.array_equal(dev[k].cpu().numpy(), st[k]), k                           # no row state is reset
    assert dev["shared"].cpu().tolist() == [13, st["shared"][1] + 4, 0, 3]


@pytest.mark.parametrize("fmt", ("f32", "bf16", "f16"))
def test_refill_reads_the_ukv_ring_row_of_the_feature_row(lib, fmt):
    """C = 6, n = 2: sequences 6, 7 (feature row 3 -> ukv ring row 0), 8, 9 (feature row 4 -> ring row 1).  Slot 0 of a refilled row,
    every layer, K and V: that ukv row in kv_slot0_kernel's rounding - the value itself in the fp32 cache, its round-to-nearest-even
    in a 16-bit one - and not one other element of the cache changes."""
    case = [c for c in S.hook_cases() if c[0] == "two_per_feature_row"][0]
    name, C, n, S_before, submit, handout, retire, R_, L, st, arg = case
    n_layer, T = 3, 5
    g = torch.Generator().manual_seed(5)
    ukv = torch.randn((C // n, n_layer * 2 * D + 32), generator=g).to(DEV)
    kv16, fp16 = (0, 0) if fmt == "f32" else (1, int(fmt == "f16"))
    dt = F32 if fmt == "f32" else R.t16(fp16)
    kv = torch.randn((n_layer, 2, R_, H, T, 64), generator=g).to(dt).to(DEV)
    before = kv.clone()
    a, b = _run(lib, case, kv=kv, ukv=ukv, n_layer=n_layer, T_slots=T, kv16=kv16, fp16=fp16)[0]
    assert a == [(2, 6, 0), (3, 7, 0), (4, 8, 1)] and b == [(0, 9, 1)]
    want = before.clone()
    for r, _, row in a + b:
        want[:, :, r, :, 0, :] = ukv[row, :n_layer * 2 * D].reshape(n_layer, 2, H, 64).to(dt)
    view = torch.int32 if fmt == "f32" else torch.int16
    assert torch.equal(kv.view(view), want.view(view))
    assert not torch.equal(kv.view(view), before.view(view))


def test_einval(lib):
    st = M.new_state(4, 0)                 # every row idle: the one call that launches hands sequences 0, 1 out
    dev = {k: _i32(v) for k, v in st.items()}
    arg, lens = _i32(np.zeros(4)), _i32(np.zeros(4))
    ids = torch.zeros((4, 8), dtype=torch.int64, device=DEV)
    f = lib.rgrg_debug_roll_session_step

    def call(C, n, S_before, submit):
        return f(_p(dev["seq"]), _p(dev["len"]), _p(dev["tok"]), _p(dev["pos"]), _p(dev["step"]), _p(dev["shared"]), _p(arg), _p(ids), None,
                 8, _p(lens), C, n, S_before, submit, 1, 0, 4, 6, None, 0, None, 0, 0, H, 0, 0, 0, 0, None)
    assert call(4, 1, 0, 2) == 0
    assert call(0, 1, 0, 0) != 0           # no ring
    assert call(4, 3, 0, 0) != 0           # C is not a multiple of n
    assert call(4, 2, 0, 3) != 0           # a submit is whole feature rows
    assert call(4, 1, 0, 5) != 0           # more than the ring holds
    assert call(4, 1, 0x7fffffff // 1024, 1) != 0
    torch.cuda.synchronize()
