"""The device pieces rolling-batch beam search adds, each ALONE through its test hook.

Attention with an ancestor table AND a per-row step (rgrg_debug_attn_decode_rowstep_src; attn_decode_kernel<true, ni, false, true>
and attn_decode_kv16_wave_kernel<true, fp16, false, false, true>): ONE launch over 11 slots of 4 rows whose slots stand at steps 0,
1, 6, 7, 70, 71, 72, 73, 143, 144 and 150 - the tail and chunk boundaries of tests/test_gpu_rolling_kernels.py - with a table that
holds random rows of the row's own slot per cache slot, so keys really come from other rows.  Outputs and the written cache slot
t + 1 are compared BIT FOR BIT against the existing HAS_SRC instantiation (rgrg_debug_attn_decode with the same table), launched once
per distinct step at *step = t on a copy of the cache, and against the float64 reference of tests/attn_reference.py under that file's
bound.  Every cache element outside the one written slot per row must be unchanged.

The turn kernel (rgrg_debug_beam_roll_turn) against the numpy rule of tests/rolling_beam_reference.py."""
import math

import numpy as np
import pytest
import torch

import attn_reference as R
import rolling_beam_reference as M
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
RGRG_EINVAL = -1
H = 16
D = H * 64
NB = 4
STEPS = (0, 1, 6, 7, 70, 71, 72, 73, 143, 144, 150)
SLOTS = max(STEPS) + 3   # one slot behind the last one written: it must stay untouched


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


_CASES = {}


def _slots(kv16):
    """One 4-row case of attn_reference.decode_inputs per step, with an ancestor table inside the 4 rows (the designated key of head 0
    comes from ANOTHER row) and its float64 / float32 references; computed once per cache format and shared."""
    if kv16 not in _CASES:
        cases = []
        for i, t in enumerate(STEPS):
            d = R.decode_inputs(NB, H, t + 2, SLOTS, 47000 + 100 * t + (7 if kv16 is None else kv16), True, None, kv16, "half",
                                tile=144 if kv16 is None else (8 if t + 2 < 40 else 72), offset=i)
            Kc, Vc = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])
            d["r64"] = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, t, d["src"], None, F64, kv16=kv16)
            d["r32"] = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, t, d["src"], None, F32, kv16=kv16)
            assert bool((d["src"][:, :t + 1] != torch.arange(NB)[:, None]).any()) or t == 0
            cases.append(d)
        _CASES[kv16] = cases
    return _CASES[kv16]


def _inputs(cases, kv16):
    """The cases stacked into one batch of len(cases) * 4 rows: qkv rows, K / V planes, the table with every slot's rows offset to
    its place, the per-row steps."""
    S = NB * len(cases)
    ld = 3 * D + 64
    x = torch.zeros(S, ld)
    for g, d in enumerate(cases):
        r = slice(NB * g, NB * g + NB)
        x[r, :D], x[r, D:2 * D], x[r, 2 * D:3 * D] = d["q"].reshape(NB, D), d["kn"].reshape(NB, D), d["vn"].reshape(NB, D)
    K, V = torch.cat([d["K"] for d in cases]), torch.cat([d["V"] for d in cases])
    if kv16 is not None:
        K, V = R.to_bits(K, kv16), R.to_bits(V, kv16)
    src = torch.cat([d["src"] + NB * g for g, d in enumerate(cases)]).int()
    rs = torch.tensor([d["step"] for d in cases for _ in range(NB)], dtype=torch.int32)
    return x.to(DEV), ld, K.to(DEV).contiguous(), V.to(DEV).contiguous(), src.to(DEV).contiguous(), rs.to(DEV)


def _bits(t, kv16):
    return t.view(torch.int32 if kv16 is None else torch.int16)


def _launch_rolling(lib, cases, kv16, ni=0, max_wgs=0, out16=False):
    x, ld, K, V, src, rs = _inputs(cases, kv16)
    S = x.shape[0]
    K0, V0 = K.clone(), V.clone()
    out = torch.full((S * D,), math.nan, dtype=F32, device=DEV)
    o16 = torch.zeros(S * D, dtype=torch.int16, device=DEV) if out16 else None
    _hip.check(lib.rgrg_debug_attn_decode_rowstep_src(_p(x), ld, _p(K), _p(V), _p(rs), _p(src), _p(out), _p(o16), S, H, SLOTS,
                                                      0 if kv16 is None else 1, int(bool(kv16)), ni, max_wgs, None),
               "rgrg_debug_attn_decode_rowstep_src")
    torch.cuda.synchronize()
    # the row's own slot, and no other slot of any row (bitwise: the planes hold NaN patterns)
    steps = rs.cpu().tolist()
    for plane, before in ((K, K0), (V, V0)):
        a, b = _bits(plane, kv16).clone(), _bits(before, kv16).clone()
        for s, t in enumerate(steps):
            a[s, :, t + 1], b[s, :, t + 1] = 0, 0
        assert torch.equal(a, b), "a cache slot other than the row's step + 1 was written"
    res = R.from_bits(o16.cpu(), kv16).reshape(S, H, 64) if out16 else out.cpu().reshape(S, H, 64)
    return res, K.cpu(), V.cpu()


def _launch_lockstep(lib, cases, kv16, t, ni=0):
    """The existing HAS_SRC kernel over ALL rows of a copy of the cache at *step = t (only the rows of the slot at step t are
    meaningful; the others read slots their case never filled)."""
    x, ld, K, V, src, _ = _inputs(cases, kv16)
    S = x.shape[0]
    out = torch.full((S * D,), math.nan, dtype=F32, device=DEV)
    step = torch.tensor([t], dtype=torch.int32, device=DEV)
    _hip.check(lib.rgrg_debug_attn_decode(_p(x), ld, _p(K), _p(V), _p(step), _p(out), None, S, H, SLOTS, _p(src), None,
                                          0 if kv16 is None else 1, int(bool(kv16)), ni, 0, 0, None), "rgrg_debug_attn_decode")
    torch.cuda.synchronize()
    return out.cpu().reshape(S, H, 64), K.cpu(), V.cpu()


def _check(lib, name, cases, kv16, got, K, V, ni=0):
    for g, d in enumerate(cases):
        t, r = d["step"], slice(NB * g, NB * g + NB)
        c = R.compare(got[r], d["r64"][0], d["r32"][0], None)
        print(f"ATTNPARITY kernel={name} case=slot_step={t} err={c['err']:.3e} noise={c['noise']:.3e} floor={c['floor']:.3e} "
              f"bound={c['bound']:.3e} used={c['used']:.3f}")
        assert c["ok"], f"{name} slot at step {t}: max|got - ref64| = {c['err']:.3e} exceeds {c['bound']:.3e}"
        assert R.designated_weight_ok(d["r64"][3][:, :, None, :], d["desig"]), "the designated key does not hold 0.2 .. 0.8 of the softmax"
        one, K1, V1 = _launch_lockstep(lib, cases, kv16, t, ni=ni)
        assert torch.equal(_bits(got[r].contiguous(), None), _bits(one[r].contiguous(), None)), \
            f"slot at step {t} differs from the HAS_SRC kernel at *step = {t}"
        assert torch.equal(_bits(K[r, :, t + 1].contiguous(), kv16), _bits(K1[r, :, t + 1].contiguous(), kv16))
        assert torch.equal(_bits(V[r, :, t + 1].contiguous(), kv16), _bits(V1[r, :, t + 1].contiguous(), kv16))


@pytest.mark.parametrize("ni", (9, 2))
def test_attn_rowstep_src_f32(lib, ni):
    cases = _slots(None)
    got, K, V = _launch_rolling(lib, cases, None, ni=ni)
    _check(lib, f"attn_decode_f32_rowstep_src_ni{ni}", cases, None, got, K, V, ni=ni)
    for g, d in enumerate(cases):
        r, slot = slice(NB * g, NB * g + NB), d["step"] + 1
        assert torch.equal(K[r, :, slot], d["kn"]) and torch.equal(V[r, :, slot], d["vn"]), "the row's slot does not hold the new k / v"
    if ni == 9:   # ni = 0 is the product's rule: 9 keys per group at S * H <= 4096
        assert torch.equal(_launch_rolling(lib, cases, None, ni=0)[0], got)


@pytest.mark.parametrize("fp16", (0, 1))
def test_attn_rowstep_src_kv16(lib, fp16):
    cases = _slots(fp16)
    name = f"attn_decode_kv16_rowstep_src_{'f16' if fp16 else 'bf16'}"
    got, K, V = _launch_rolling(lib, cases, fp16)
    _check(lib, name, cases, fp16, got, K, V)
    for g, d in enumerate(cases):
        r, slot = slice(NB * g, NB * g + NB), d["step"] + 1
        assert torch.equal(R.from_bits(K[r, :, slot], fp16), d["r64"][1].float()) and \
            torch.equal(R.from_bits(V[r, :, slot], fp16), d["r64"][2].float()), "the row's slot is not the RNE rounding of the new k / v"
    # a capped grid (a wave walks several items, each at its own step) and the 16-bit output
    capped = _launch_rolling(lib, cases, fp16, max_wgs=5)
    assert torch.equal(capped[0], got) and torch.equal(capped[1], K) and torch.equal(capped[2], V), "grid capped at 5 workgroups differs"
    g16 = _launch_rolling(lib, cases, fp16, out16=True)[0]
    assert torch.equal(g16, R.rnd16(got, fp16)), "out16 is not the rounding of out"


def test_attn_rowstep_src_einval(lib):
    """Steps outside 0 .. T_slots - 2 and table entries outside the rows are refused before any launch: the outputs keep their NaN."""
    z16 = torch.zeros(2 * H * 4 * 64, dtype=torch.int16, device=DEV)
    q = torch.zeros(2, 3 * D, device=DEV)
    out = torch.full((2 * D,), math.nan, device=DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    ok, late, neg = i32([0, 2]), i32([0, 3]), i32([-1, 0])
    tab, bad_tab = i32([[0, 1, 0, 0], [1, 0, 1, 0]]), i32([[0, 1, 0, 0], [1, 0, 1, 2]])
    f = lib.rgrg_debug_attn_decode_rowstep_src
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(late), _p(tab), _p(out), None, 2, H, 4, 1, 0, 0, 0, None) == RGRG_EINVAL   # slot 4 of 4
    assert b"row_step[1] = 3" in lib.rgrg_last_error()
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(neg), _p(tab), _p(out), None, 2, H, 4, 1, 0, 0, 0, None) == RGRG_EINVAL
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(ok), _p(bad_tab), _p(out), None, 2, H, 4, 1, 0, 0, 0, None) == RGRG_EINVAL   # row 2 of 2
    assert b"src[1][3] = 2" in lib.rgrg_last_error()
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(ok), None, _p(out), None, 2, H, 4, 1, 0, 0, 0, None) == RGRG_EINVAL          # no table
    assert f(_p(q), 3 * D, _p(z16), _p(z16), None, _p(tab), _p(out), None, 2, H, 4, 1, 0, 0, 0, None) == RGRG_EINVAL         # no row_step
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(ok), _p(tab), _p(out), None, 2, H, 4, 0, 0, 5, 0, None) == RGRG_EINVAL      # ni = 5
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call launched"
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(ok), _p(tab), _p(out), None, 2, H, 4, 1, 0, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


# ------------------------------------------------------------------------------------------------ the turn kernel
def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


@pytest.mark.parametrize("T", (13, 160))
@pytest.mark.parametrize("nb", (2, 4, 5))
def test_turn_kernel_equals_the_rule(lib, nb, T):
    """9 slots: fresh, idle and continuing ones mixed; the continuing slots at steps 0, 1, T - 2 (the last one a table row holds) and
    random ones; parents permuted in one slot, all the same row in another, random (with duplicates) in the rest.  Cells behind
    t + 1 and all cells of idle rows keep the sentinel the new table was filled with; a fresh row writes cell 0 only."""
    rng = np.random.default_rng(100 * nb + T)
    kinds = ["cont", "fresh", "cont", "idle", "cont", "cont", "fresh", "cont", "idle"]
    steps = [0, 5, 1, 7, T - 2, int(rng.integers(0, T - 1)), 3, int(rng.integers(0, T - 1)), 0]
    G, R_ = len(kinds), len(kinds) * nb
    parent, step = np.zeros(R_, np.int32), np.zeros(R_, np.int32)
    for g, kind in enumerate(kinds):
        r = slice(g * nb, (g + 1) * nb)
        step[r] = steps[g]
        if kind == "fresh":
            parent[r] = M.FRESH
        elif kind == "idle":
            parent[r] = M.IDLE
        elif g == 0:
            parent[r] = g * nb + rng.permutation(nb)
        elif g == 2:
            parent[r] = g * nb + nb - 1
        else:
            parent[r] = g * nb + rng.integers(0, nb, nb)
    src_old = (np.arange(R_)[:, None] // nb * nb + rng.integers(0, nb, (R_, T))).astype(np.int32)
    src_new = np.full((R_, T), -7, np.int32)
    want_new, want_step = M.turn_rule(src_old, src_new, parent, step, nb)
    d_old, d_new, d_par, d_step = _i32(src_old), _i32(src_new), _i32(parent), _i32(step)
    _hip.check(lib.rgrg_debug_beam_roll_turn(_p(d_old), _p(d_new), _p(d_par), _p(d_step), T, nb, R_, None), "rgrg_debug_beam_roll_turn")
    torch.cuda.synchronize()
    assert np.array_equal(d_new.cpu().numpy(), want_new), (nb, T)
    assert np.array_equal(d_step.cpu().numpy(), want_step)
    assert np.array_equal(d_old.cpu().numpy(), src_old) and np.array_equal(d_par.cpu().numpy(), parent)
    # what the rule implies, spelled out on the result
    got = d_new.cpu().numpy()
    for g, kind in enumerate(kinds):
        for r in range(g * nb, (g + 1) * nb):
            written = {"idle": 0, "fresh": 1, "cont": steps[g] + 2}[kind]
            assert (got[r, written:] == -7).all() and (got[r, :written] != -7).all()


def test_turn_kernel_einval(lib):
    T, nb, R_ = 8, 2, 4
    old, new = _i32(np.zeros((R_, T))), _i32(np.full((R_, T), -7))
    f = lib.rgrg_debug_beam_roll_turn
    cases = [([0, 2, 2, 3], [1, 1, 2, 2]),     # row 1 names a parent of the other slot
             ([0, 1, 2, 3], [1, 2, 2, 2]),     # the rows of slot 0 stand at different steps
             ([0, 1, 2, 3], [1, 1, 7, 7]),     # step T - 1: no cell t + 1
             ([0, 1, -3, 3], [1, 1, 2, 2])]    # not a row, not a code
    for parent, step in cases:
        assert f(_p(old), _p(new), _p(_i32(parent)), _p(_i32(step)), T, nb, R_, None) == RGRG_EINVAL, (parent, step)
    assert f(_p(old), _p(old), _p(_i32([0, 1, 2, 3])), _p(_i32([1, 1, 2, 2])), T, nb, R_, None) == RGRG_EINVAL   # the tables alias
    assert f(_p(old), _p(new), _p(_i32([0, 1, 2])), _p(_i32([1, 1, 2])), T, nb, 3, None) == RGRG_EINVAL          # R not a multiple of nb
    torch.cuda.synchronize()
    assert bool((new == -7).all()), "a refused call launched"
