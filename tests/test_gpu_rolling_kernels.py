"""The two kernels rolling-batch decoding adds, each ALONE through its test hook.

Attention with a per-row step (rgrg_debug_attn_decode_rowstep; attn_decode_kernel<.., ROWSTEP> and
attn_decode_kv16_wave_kernel<.., ROWSTEP>): ONE launch whose rows stand at steps 0, 1, 6, 7, 70, 71, 72, 73, 143, 144 and 150 - the
tail-switch boundaries of the 8-key groups, the 72-key chunk of the 16-bit kernel, the 144-key chunk of the fp32 kernel - against the
float64 reference of tests/attn_reference.py with that file's bound, and BIT FOR BIT against the existing kernel launched alone on
the row at *step = row_step[s] (rgrg_debug_attn_decode).  The new key / value must land in the row's own slot and nowhere else.

Retire and refill (rgrg_debug_roll_step) against the numpy model of tests/rolling_reference.py on its hook_cases(), which
tests/test_rolling_reference.py shows to reject the named mutations."""
import math

import numpy as np
import pytest
import torch

import attn_reference as R
import rolling_reference as M
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
RGRG_EINVAL = -1
H = 16
D = H * 64
STEPS = (0, 1, 6, 7, 70, 71, 72, 73, 143, 144, 150)
SLOTS = max(STEPS) + 3   # one slot behind the last one written: it must stay untouched


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


_ROWS = {}


def _rows(kv16):
    """One single-row case of attn_reference.decode_inputs per step (edge-weighted: the designated key of every head holds half of
    the softmax and walks through the image key, the new token's slot and the chunk edges), with its float64 / float32 references;
    computed once per cache format and shared."""
    if kv16 not in _ROWS:
        rows = []
        for i, t in enumerate(STEPS):
            d = R.decode_inputs(1, H, t + 2, SLOTS, 31000 + 100 * t + (7 if kv16 is None else kv16), False, None, kv16, "half",
                                tile=144 if kv16 is None else (8 if t + 2 < 40 else 72), offset=i)
            Kc, Vc = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])
            d["r64"] = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, t, None, None, F64, kv16=kv16)
            d["r32"] = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, t, None, None, F32, kv16=kv16)
            rows.append(d)
        _ROWS[kv16] = rows
    return _ROWS[kv16]


def _qkv(rows):
    ld = 3 * D + 64
    x = torch.zeros(len(rows), ld)
    for s, d in enumerate(rows):
        x[s, :D], x[s, D:2 * D], x[s, 2 * D:3 * D] = d["q"].reshape(D), d["kn"].reshape(D), d["vn"].reshape(D)
    return x.to(DEV), ld


def _planes(rows, kv16):
    K, V = torch.cat([d["K"] for d in rows]), torch.cat([d["V"] for d in rows])
    if kv16 is not None:
        K, V = R.to_bits(K, kv16), R.to_bits(V, kv16)
    return K.to(DEV).contiguous(), V.to(DEV).contiguous()


def _bits(t, kv16):
    return t.view(torch.int32 if kv16 is None else torch.int16)


def _launch_rowstep(lib, rows, kv16, ni=0, max_wgs=0, out16=False):
    S = len(rows)
    x, ld = _qkv(rows)
    K, V = _planes(rows, kv16)
    K0, V0 = K.clone(), V.clone()
    out = torch.full((S * D,), math.nan, dtype=F32, device=DEV)
    o16 = torch.zeros(S * D, dtype=torch.int16, device=DEV) if out16 else None
    rs = torch.tensor([d["step"] for d in rows], dtype=torch.int32, device=DEV)
    _hip.check(lib.rgrg_debug_attn_decode_rowstep(_p(x), ld, _p(K), _p(V), _p(rs), _p(out), _p(o16), S, H, SLOTS, 0 if kv16 is None else 1,
                                                  int(bool(kv16)), ni, max_wgs, None), "rgrg_debug_attn_decode_rowstep")
    torch.cuda.synchronize()
    # the row's own slot, and no other slot of any row (bitwise: the planes hold NaN patterns)
    for plane, before in ((K, K0), (V, V0)):
        a, b = _bits(plane, kv16).clone(), _bits(before, kv16).clone()
        for s, d in enumerate(rows):
            a[s, :, d["step"] + 1], b[s, :, d["step"] + 1] = 0, 0
        assert torch.equal(a, b), "a cache slot other than the row's step + 1 was written"
    res = R.from_bits(o16.cpu(), kv16).reshape(S, H, 64) if out16 else out.cpu().reshape(S, H, 64)
    return res, K.cpu(), V.cpu()


def _launch_alone(lib, d, kv16, ni=0):
    """The existing kernel on ONE row at *step = the row's step."""
    x, ld = _qkv([d])
    K, V = _planes([d], kv16)
    out = torch.full((D,), math.nan, dtype=F32, device=DEV)
    step = torch.tensor([d["step"]], dtype=torch.int32, device=DEV)
    _hip.check(lib.rgrg_debug_attn_decode(_p(x), ld, _p(K), _p(V), _p(step), _p(out), None, 1, H, SLOTS, None, None, 0 if kv16 is None else 1,
                                          int(bool(kv16)), ni, 0, 0, None), "rgrg_debug_attn_decode")
    torch.cuda.synchronize()
    return out.cpu().reshape(1, H, 64), K.cpu(), V.cpu()


def _check_rows(kernel, rows, got, kv16, out16=None):
    for s, d in enumerate(rows):
        r = R.compare(got[s:s + 1], d["r64"][0], d["r32"][0], out16)
        print(f"ATTNPARITY kernel={kernel} case=row_step={d['step']} err={r['err']:.3e} noise={r['noise']:.3e} floor={r['floor']:.3e} "
              f"bound={r['bound']:.3e} used={r['used']:.3f}")
        assert r["ok"], f"{kernel} row_step={d['step']}: max|got - ref64| = {r['err']:.3e} exceeds {r['bound']:.3e}"
        assert R.designated_weight_ok(d["r64"][3][:, :, None, :], d["desig"]), "the designated key does not hold 0.2 .. 0.8 of the softmax"


@pytest.mark.parametrize("ni", (9, 2))
def test_attn_rowstep_f32(lib, ni):
    rows = _rows(None)
    got, K, V = _launch_rowstep(lib, rows, None, ni=ni)
    _check_rows(f"attn_decode_f32_rowstep_ni{ni}", rows, got, None)
    for s, d in enumerate(rows):
        slot = d["step"] + 1
        assert torch.equal(K[s, :, slot], d["kn"][0]) and torch.equal(V[s, :, slot], d["vn"][0]), "the row's slot does not hold the new k / v"
        one, K1, V1 = _launch_alone(lib, d, None, ni=ni)
        assert torch.equal(got[s:s + 1], one), f"row at step {d['step']} differs from the kernel alone at *step = {d['step']}"
        assert torch.equal(_bits(K[s:s + 1], None), _bits(K1, None)) and torch.equal(_bits(V[s:s + 1], None), _bits(V1, None))
    if ni == 9:   # ni = 0 is the product's rule: 9 keys per group at S * H <= 4096
        assert torch.equal(_launch_rowstep(lib, rows, None, ni=0)[0], got)


@pytest.mark.parametrize("fp16", (0, 1))
def test_attn_rowstep_kv16(lib, fp16):
    rows = _rows(fp16)
    name = f"attn_decode_kv16_rowstep_{'f16' if fp16 else 'bf16'}"
    got, K, V = _launch_rowstep(lib, rows, fp16)
    _check_rows(name, rows, got, fp16)
    for s, d in enumerate(rows):
        slot = d["step"] + 1
        assert torch.equal(R.from_bits(K[s, :, slot], fp16), d["r64"][1][0].float()) and \
            torch.equal(R.from_bits(V[s, :, slot], fp16), d["r64"][2][0].float()), "the row's slot is not the RNE rounding of the new k / v"
        one, K1, V1 = _launch_alone(lib, d, fp16)
        assert torch.equal(got[s:s + 1], one), f"row at step {d['step']} differs from the kernel alone at *step = {d['step']}"
        assert torch.equal(K[s:s + 1], K1) and torch.equal(V[s:s + 1], V1)
    # a capped grid (a wave walks several items, each at its own step) and the 16-bit output
    capped = _launch_rowstep(lib, rows, fp16, max_wgs=5)
    assert torch.equal(capped[0], got) and torch.equal(capped[1], K) and torch.equal(capped[2], V), "grid capped at 5 workgroups differs"
    g16 = _launch_rowstep(lib, rows, fp16, out16=True)[0]
    assert torch.equal(g16, R.rnd16(got, fp16)), "out16 is not the rounding of out"


def test_attn_rowstep_einval(lib):
    z16 = torch.zeros(2 * H * 4 * 64, dtype=torch.int16, device=DEV)
    q = torch.zeros(2, 3 * D, device=DEV)
    ok, late, neg = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in ([0, 2], [0, 3], [-1, 0]))
    f = lib.rgrg_debug_attn_decode_rowstep
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(ok), _p(q), None, 2, H, 4, 1, 0, 0, 0, None) == 0
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(late), _p(q), None, 2, H, 4, 1, 0, 0, 0, None) == RGRG_EINVAL   # slot 4 of 4
    assert b"row_step[1] = 3" in lib.rgrg_last_error()
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(neg), _p(q), None, 2, H, 4, 1, 0, 0, 0, None) == RGRG_EINVAL
    assert f(_p(q), 3 * D, _p(z16), _p(z16), None, _p(q), None, 2, H, 4, 1, 0, 0, 0, None) == RGRG_EINVAL         # no row_step
    assert f(_p(q), 3 * D, _p(z16), _p(z16), _p(ok), _p(q), None, 2, H, 4, 0, 0, 5, 0, None) == RGRG_EINVAL      # ni = 5
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ retire and refill
def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _roll(lib, case, kv=None, ukv=None, n_layer=0, T_slots=0, kv16=0, fp16=0):
    name, S, R_, L, st, arg = case
    ids0, lens0 = M.sentinel_output(S, L + 1)
    dev = {k: _i32(v) for k, v in st.items()}
    ids, lens, a = torch.from_numpy(ids0).to(DEV), _i32(lens0), _i32(arg)
    kv_stride = R_ * H * T_slots * 64
    _hip.check(lib.rgrg_debug_roll_step(_p(dev["seq"]), _p(dev["len"]), _p(dev["tok"]), _p(dev["pos"]), _p(dev["step"]), _p(dev["shared"]),
                                        _p(a), _p(ids), L + 1, _p(lens), S, R_, L, _p(ukv), 0 if ukv is None else ukv.shape[1], _p(kv),
                                        2 * kv_stride, kv_stride, H, T_slots, n_layer, kv16, fp16, None), "rgrg_debug_roll_step")
    torch.cuda.synchronize()
    want_st = {k: v.copy() for k, v in st.items()}
    want_ids, want_lens = M.sentinel_output(S, L + 1)
    refills = M.roll_step(want_st, arg, want_ids, want_lens, L)
    for k in want_st:
        assert np.array_equal(dev[k].cpu().numpy(), want_st[k]), (name, k, dev[k].cpu().tolist(), want_st[k].tolist())
    assert np.array_equal(ids.cpu().numpy(), want_ids), (name, "ids")
    assert np.array_equal(lens.cpu().numpy(), want_lens), (name, "lens")
    return refills


@pytest.mark.parametrize("case", M.hook_cases(), ids=lambda c: c[0])
def test_retire_refill_step_equals_the_model(lib, case):
    _roll(lib, case)


@pytest.mark.parametrize("fmt", ("f32", "bf16", "f16"))
def test_refill_copies_the_image_key_value_into_slot_0(lib, fmt):
    """Slot 0 of a refilled row, every layer, K and V: the sequence's ukv row in kv_slot0_kernel's rounding - the value itself in the
    fp32 cache, its round-to-nearest-even in a 16-bit one - and not one other element of the cache changes."""
    case = [c for c in M.hook_cases() if c[0] == "all_end_fewer_pending"][0]
    _, S, R_, L, _, _ = case
    n_layer, T = 3, 5
    g = torch.Generator().manual_seed(5)
    ukv = torch.randn((S, n_layer * 2 * D + 32), generator=g).to(DEV)
    kv16, fp16 = (0, 0) if fmt == "f32" else (1, int(fmt == "f16"))
    dt = F32 if fmt == "f32" else R.t16(fp16)
    kv = torch.randn((n_layer, 2, R_, H, T, 64), generator=g).to(dt).to(DEV)
    before = kv.clone()
    refills = _roll(lib, case, kv=kv, ukv=ukv, n_layer=n_layer, T_slots=T, kv16=kv16, fp16=fp16)
    assert refills == [(0, 5), (1, 6)]
    want = before.clone()
    for r, seq in refills:
        want[:, :, r, :, 0, :] = ukv[seq, :n_layer * 2 * D].reshape(n_layer, 2, H, 64).to(dt)
    view = torch.int32 if fmt == "f32" else torch.int16
    assert torch.equal(kv.view(view), want.view(view))
    assert not torch.equal(kv.view(view), before.view(view))
