"""Every attention kernel ALONE against the float64 reference of tests/attn_reference.py, through the rgrg_debug_attn_* hooks
(the product's own launchers on caller-provided buffers).  One launch per case, every output element compared:
max |got - ref64| <= MARGIN * max |ref32 - ref64| + one ulp of the output type at max |ref| - the bound comes from the reference
alone (attn_reference.bound).  Each figure is printed before it is asserted (lines starting with ATTNPARITY); the worst ratios
observed on the MI355X are kept in profiles/attn_kernel_parity.md.

Inputs are edge-weighted unless a case says otherwise: one designated key per (row, head) holds half of the softmax, and it
walks through the image key, the current token's slot and the first / last key of every chunk or tile the kernel forms.
"""
import math

import pytest
import torch

import attn_reference as R
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
RGRG_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(t, dtype=None):
    return None if t is None else t.to(device=DEV, dtype=dtype or t.dtype).contiguous()


def _check(kernel, case, name, got, ref64, ref32, out16=None, margin=R.MARGIN, extra_floor=0.0):
    r = R.compare(got, ref64, ref32, out16, margin, extra_floor)
    print(f"ATTNPARITY kernel={kernel} case={case} out={name} err={r['err']:.3e} noise={r['noise']:.3e} floor={r['floor']:.3e} "
          f"bound={r['bound']:.3e} ratio={r['ratio']:.2f} used={r['used']:.3f}")
    assert r["ok"], f"{kernel} {case} {name}: max|got - ref64| = {r['err']:.3e} exceeds {r['bound']:.3e} (noise {r['noise']:.3e}, floor {r['floor']:.3e})"


def _mask(lib, seed, stream_id, p, shape, row_len):
    out = torch.empty(shape, dtype=F32, device=DEV)
    _hip.check(lib.rgrg_dropout_mask_f32(seed, stream_id, p, out.numel(), row_len, _p(out), None), "rgrg_dropout_mask_f32")
    return out.cpu()


def test_host_dropout_mask_equals_the_exported_one(lib):
    """attn_reference.philox_mask (used by the GPU-less sensitivity tests) is rgrg_dropout_mask_f32 bit for bit."""
    for shape, row_len in (((2, 16, 5, 6), 6), ((3, 16, 33, 34), 34), ((1000,), 0)):
        assert torch.equal(_mask(lib, 0x1234567890ABCDEF, 13, 0.25, shape, row_len), R.philox_mask(0x1234567890ABCDEF, 13, 0.25, shape, row_len))


# ------------------------------------------------------------------------------------------------ decode kernels
def _run_decode(lib, d, *, kv16=None, out16=False, ni=0, frag_out=0, max_wgs=0, expect=0):
    """One rgrg_debug_attn_decode launch on the inputs of attn_reference.decode_inputs.  Returns (out, K plane, V plane) as
    fp32 CPU tensors after checking that the launch left every cache byte outside slot step + 1 untouched."""
    S, H, slots = d["S"], d["H"], d["slots"]
    D = H * 64
    ld = 3 * D + 64   # a row pitch larger than the row: the kernels take it as an argument
    qkv = torch.zeros(S, ld)
    qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D] = d["q"].reshape(S, D), d["kn"].reshape(S, D), d["vn"].reshape(S, D)
    if kv16 is None:
        K, V = _dev(d["K"]), _dev(d["V"])
    else:
        K, V = _dev(R.to_bits(d["K"], kv16)), _dev(R.to_bits(d["V"], kv16))
    K0, V0 = K.clone(), V.clone()
    rows_pad = (S + 31) // 32 * 32
    out = torch.full((rows_pad * D,), math.nan, dtype=F32, device=DEV)
    o16 = torch.zeros(S * D, dtype=torch.int16, device=DEV) if out16 else None
    step = torch.tensor([d["step"]], dtype=torch.int32, device=DEV)
    dq, src, km = _dev(qkv), _dev(d["src"]), _dev(d["kmask"])
    rc = lib.rgrg_debug_attn_decode(_p(dq), ld, _p(K), _p(V), _p(step), _p(out), _p(o16), S, H, slots, _p(src), _p(km),
                                    0 if kv16 is None else 1, int(bool(kv16)), ni, frag_out, max_wgs, None)
    assert rc == expect, (rc, lib.rgrg_last_error())
    if expect:
        return None
    torch.cuda.synchronize()
    slot = d["step"] + 1
    for plane, before in ((K, K0), (V, V0)):   # bitwise: the planes hold NaN patterns
        a, b = plane.view(torch.int32 if kv16 is None else torch.int16).clone(), before.view(torch.int32 if kv16 is None else torch.int16).clone()
        a[:, :, slot], b[:, :, slot] = 0, 0
        assert torch.equal(a, b), "a cache slot other than step + 1 was written"
    if out16:
        res = R.from_bits(o16.cpu(), kv16).reshape(S, H, 64)
    elif frag_out:
        idx = torch.tensor([R.frag_off(s, k, D) for s in range(S) for k in range(D)])
        res = out.cpu()[idx].reshape(S, H, 64)
    else:
        res = out.cpu()[:S * D].reshape(S, H, 64)
    wid = (lambda t: t.cpu()) if kv16 is None else (lambda t: R.from_bits(t.cpu(), kv16))
    return res, wid(K)[:, :, slot], wid(V)[:, :, slot]


def _decode_refs(d, kv16=None, out16=False):
    Kc, Vc = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])   # the reference gathers slots < nkeys - 1 only; NaN * 0 otherwise
    r64 = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, d["step"], d["src"], d["kmask"], F64, kv16=kv16, out16=out16)
    r32 = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, d["step"], d["src"], d["kmask"], F32, kv16=kv16, out16=out16)
    return r64, r32


F32_NKEYS = (2, 3, 15, 16, 17, 32, 33, 64, 65, 143, 144, 145, 146, 160, 288, 289)
# (S, ancestor table, key mask, weighting)
F32_CONFIGS = ((33, False, None, "half"), (33, True, None, "half"), (3, False, "random", "half"), (1, False, "all_tokens", "half"),
               (3, False, "current", "half"), (1, True, None, None))


@pytest.mark.parametrize("nkeys", F32_NKEYS)
def test_attn_decode_f32(lib, nkeys):
    """attn_decode_kernel<HAS_SRC, 9 | 2, HAS_MASK>: chunks of 144 (9 per group) / 32 (2 per group) keys, tail in steps of 16."""
    for ci, (S, with_src, kmk, wt) in enumerate(F32_CONFIGS):
        d = R.decode_inputs(S, 16, nkeys, nkeys + 1 + ci % 3, 100 * nkeys + ci, with_src, kmk, None, wt, tile=16 if nkeys < 40 else 144, offset=ci)
        r64, r32 = _decode_refs(d)
        if wt:   # (rows whose token keys are all masked have only the image key to weigh: exempt, as in the teacher-forced forms)
            unmasked = None if d["kmask"] is None else (d["kmask"][:, 1:nkeys] >= 0).float()
            assert R.designated_weight_ok(r64[3][:, :, None, :], d["desig"], unmasked), "the designated key does not hold 0.2 .. 0.8 of the softmax"
        case = f"nkeys={nkeys},S={S},src={int(with_src)},mask={kmk},w={wt}"
        got9 = _run_decode(lib, d, ni=9)
        got2 = _run_decode(lib, d, ni=2)
        got0 = _run_decode(lib, d, ni=0)
        _check("attn_decode_f32", case, "out", got9[0], r64[0], r32[0])
        _check("attn_decode_f32", case + ",ni=2", "out", got2[0], r64[0], r32[0])
        assert torch.equal(got9[0], got0[0]), "ni = 0 did not select the 9-key instantiation for S * H <= 4096"
        for got in (got9, got2):
            assert torch.equal(got[1], d["kn"]) and torch.equal(got[2], d["vn"]), "slot step + 1 does not hold the new k / v exactly"
        if ci < 2:
            gotf = _run_decode(lib, d, ni=0, frag_out=1)
            assert torch.equal(gotf[0], got9[0]), "frag_out = 1 is not frag_out = 0 re-laid out"


@pytest.mark.parametrize("nkeys", F32_NKEYS)
def test_attn_decode_f32_9_and_2_keys_per_group_bit_identical(lib, nkeys):
    """The 9- and the 2-key instantiation give the same bits at the same S: the running softmax of attn_chunk advances key by
    key, so a group's result does not depend on how its keys are cut into chunks (it did before: up to 1.07e-6 apart, 1 - 4 fp32
    ulps, at every key count but 17 and 32 - profiles/attn_kernel_parity.md)."""
    d = R.decode_inputs(33, 16, nkeys, nkeys + 1, 100 * nkeys, False, None, None, "half", tile=16 if nkeys < 40 else 144)
    got9, got2 = _run_decode(lib, d, ni=9)[0], _run_decode(lib, d, ni=2)[0]
    diff = (got9.double() - got2.double()).abs()
    print(f"ATTNPARITY kernel=attn_decode_f32 case=nkeys={nkeys},S=33,ni9_vs_ni2 out=out maxdiff={float(diff.max()):.3e} "
          f"differing={int((diff > 0).sum())}/{diff.numel()} max={float(got9.abs().max()):.3e}")
    assert torch.equal(got9, got2), "9 and 2 keys per group differ"


@pytest.mark.parametrize("weighted,nkeys", [("big_first", 146), ("big_last", 146), ("big_first", 289), ("big_last", 289), ("big_last", 33)])
def test_attn_decode_f32_large_scores(lib, weighted, nkeys):
    """A score of 60 holds the maximum in the first / in the last chunk: the running-softmax rescale and the m == -inf guards."""
    for with_src in (False, True):
        d = R.decode_inputs(5, 16, nkeys, nkeys + 2, 7 * nkeys, with_src, None, None, weighted, tile=144)
        r64, r32 = _decode_refs(d)
        for ni in (9, 2):
            _check("attn_decode_f32", f"{weighted},nkeys={nkeys},src={int(with_src)},ni={ni}", "out", _run_decode(lib, d, ni=ni)[0], r64[0], r32[0])


def test_attn_decode_einval(lib):
    d = R.decode_inputs(4, 16, 9, 12, 5, True, "random", None, None)
    _run_decode(lib, d, expect=RGRG_EINVAL)                       # kmask with src
    d["src"] = None
    _run_decode(lib, d, kv16=0, expect=RGRG_EINVAL)               # kmask with a 16-bit cache
    d3 = R.decode_inputs(4, 6, 9, 12, 5, False, None, 0, None)
    _run_decode(lib, d3, kv16=0, expect=RGRG_EINVAL)              # H % 4 with a 16-bit cache
    _run_decode(lib, R.decode_inputs(2, 16, 9, 12, 5), ni=5, expect=RGRG_EINVAL)


KV16_NKEYS = (2, 7, 8, 9, 47, 48, 49, 71, 72, 73, 80, 81, 120, 121, 144, 145, 146, 216, 217, 300)


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("nkeys", KV16_NKEYS)
def test_attn_decode_kv16(lib, nkeys, fp16):
    """attn_decode_kv16_wave_kernel<HAS_SRC, F16>: chunks of 72 keys, tail in steps of 8; one wave per (sequence, head) or, with a
    capped grid, 2 - 3 items per wave (528 items over 280 / 200 waves)."""
    configs = [(33, False, False, "half"), (33, True, True, "half"), (3, True, False, "half"), (1, False, True, None)]
    if nkeys in (9, 145):
        configs.append((130, True, True, "half"))
    for ci, (S, with_src, out16, wt) in enumerate(configs):
        d = R.decode_inputs(S, 16, nkeys, nkeys + ci % 3, 1000 * nkeys + 10 * fp16 + ci, with_src, None, fp16, wt, tile=8 if nkeys < 40 else 72, offset=ci)
        r64, r32 = _decode_refs(d, fp16, out16)
        if wt:
            assert R.designated_weight_ok(r64[3][:, :, None, :], d["desig"]), "the designated key does not hold 0.2 .. 0.8 of the softmax"
        case = f"nkeys={nkeys},S={S},src={int(with_src)},out16={int(out16)},w={wt}"
        got = _run_decode(lib, d, kv16=fp16, out16=out16)
        _check(f"attn_decode_kv16_{'f16' if fp16 else 'bf16'}", case, "out16" if out16 else "out", got[0], r64[0], r32[0], fp16 if out16 else None)
        assert torch.equal(got[1], r64[1].float()) and torch.equal(got[2], r64[2].float()), "slot step + 1 is not the RNE rounding of the new k / v"
        if S == 33:
            for cap in (70, 50):
                gc = _run_decode(lib, d, kv16=fp16, out16=out16, max_wgs=cap)
                assert torch.equal(gc[0], got[0]) and torch.equal(gc[1], got[1]) and torch.equal(gc[2], got[2]), f"grid capped at {cap} workgroups differs"


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("weighted,nkeys", [("big_first", 146), ("big_last", 146), ("big_last", 217), ("big_last", 73)])
def test_attn_decode_kv16_large_scores(lib, weighted, nkeys, fp16):
    for with_src in (False, True):
        d = R.decode_inputs(5, 16, nkeys, nkeys + 2, 9 * nkeys + fp16, with_src, None, fp16, weighted, tile=72)
        r64, r32 = _decode_refs(d, fp16)
        _check(f"attn_decode_kv16_{'f16' if fp16 else 'bf16'}", f"{weighted},nkeys={nkeys},src={int(with_src)}", "out",
               _run_decode(lib, d, kv16=fp16, max_wgs=7)[0], r64[0], r32[0])


# ------------------------------------------------------------------------------------------------ teacher-forced kernels
KCOL, LD_PAD = 128, 64   # the image key / value sit at a column offset inside a wider row, as in the product (layer l: l * 2 * D)


def _ukv_rows(t, D, dtype=F32):
    S = t["S"]
    u = torch.zeros(S, KCOL + 2 * D + LD_PAD, dtype=dtype)
    u[:, KCOL:KCOL + 2 * D] = t["ukv"].reshape(S, 2 * D).to(dtype)
    return u


TF_T = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 255, 256, 300, 1023)
TF_VARIANTS = ((None, 0.0), ("right", 0.25), ("left", 0.0), ("all", 0.25))
SEED, STREAM = 0x5EEDC0FFEE123, 9


def _fits(variant, T):
    return variant == 3 or (variant == 1 and T + 1 <= 96) or (variant == 2 and T + 1 <= 256)


@pytest.mark.parametrize("T", TF_T)
def test_attn_prefill(lib, T):
    """attn_prefill_kernel<3>, <8> and attn_prefill_stream_kernel, each forced wherever T + 1 keys fit it: out, lse, out16.
    H = 3 makes S * H * ceil(T / 32) odd (waves of the last workgroup return early); H = 16 is the model's."""
    for vi, (amk, p) in enumerate(TF_VARIANTS):
        S, H = (1, 3) if T > 256 else ((3, 3) if vi % 2 == 0 else (2, 16))
        if amk == "all":
            S = max(S, 2)
        fp16 = vi % 2
        wt = None if (vi == 2 and T > 2) else "half"
        t = R.tf_inputs(S, T, H, 31 * T + vi, amk, None, wt, offset=vi)
        D = H * 64
        drop = _mask(lib, SEED, STREAM, p, (S, H, T, T + 1), T + 1) if p > 0 else None
        o64, l64, P64 = R.tf_forward(t["qkv"], t["ukv"], t["am"], drop, F64)
        o32, l32, _ = R.tf_forward(t["qkv"], t["ukv"], t["am"], drop, F32)
        if wt:
            assert R.designated_weight_ok(P64, t["desig"], t["am"]), "the designated key does not hold 0.2 .. 0.8 of the softmax"
        qkv, ukv, am = _dev(t["qkv"].reshape(S * T, 3 * D)), _dev(_ukv_rows(t, D)), _dev(t["am"])
        results = {}
        for variant in (0, 1, 2, 3):
            out = torch.full((S * T, D), math.nan, dtype=F32, device=DEV)
            o16 = torch.zeros(S * T, D, dtype=torch.int16, device=DEV)
            lse = torch.full((S * T, H), math.nan, dtype=F32, device=DEV)
            rc = lib.rgrg_debug_attn_prefill(_p(qkv), _p(ukv), ukv.shape[1], KCOL, _p(am), _p(out), _p(o16), _p(lse), S, H, T, variant,
                                             SEED, STREAM, p, fp16, None)
            if variant and not _fits(variant, T):
                assert rc == RGRG_EINVAL, f"variant {variant} accepted {T + 1} keys"
                continue
            assert rc == 0, lib.rgrg_last_error()
            torch.cuda.synchronize()
            results[variant] = (out.cpu().reshape(S, T, H, 64), lse.cpu().reshape(S, T, H), R.from_bits(o16.cpu(), fp16).reshape(S, T, H, 64))
            case = f"T={T},S={S},H={H},am={amk},p={p},variant={variant},w={wt}"
            _check("attn_prefill", case, "out", results[variant][0], o64, o32)
            _check("attn_prefill", case, "lse", results[variant][1], l64, l32)
            _check("attn_prefill", case, f"out16_{'f16' if fp16 else 'bf16'}", results[variant][2], R.rnd16(o64, fp16), R.rnd16(o32, fp16), fp16)
            assert torch.equal(results[variant][2], R.rnd16(results[variant][0], fp16)), "out16 is not the rounding of out"
        first = results[3]
        for variant, r in results.items():   # register and streaming kernels: the same tile and register order
            assert all(torch.equal(a, b) for a, b in zip(r, first)), f"variant {variant} and the streaming kernel differ"


@pytest.mark.parametrize("weighted", ("big_first", "big_last"))
def test_attn_prefill_large_scores(lib, weighted):
    for T in (70, 300):
        S, H = 2, 16
        D = H * 64
        t = R.tf_inputs(S, T, H, 77 + T, None, None, weighted)
        o64, l64, _ = R.tf_forward(t["qkv"], t["ukv"], None, None, F64)
        o32, l32, _ = R.tf_forward(t["qkv"], t["ukv"], None, None, F32)
        qkv, ukv = _dev(t["qkv"].reshape(S * T, 3 * D)), _dev(_ukv_rows(t, D))
        out = torch.full((S * T, D), math.nan, dtype=F32, device=DEV)
        lse = torch.full((S * T, H), math.nan, dtype=F32, device=DEV)
        _hip.check(lib.rgrg_debug_attn_prefill(_p(qkv), _p(ukv), ukv.shape[1], KCOL, None, _p(out), None, _p(lse), S, H, T, 0, 0, 0, 0.0, 0, None))
        torch.cuda.synchronize()
        _check("attn_prefill", f"{weighted},T={T}", "out", out.cpu().reshape(S, T, H, 64), o64, o32)
        _check("attn_prefill", f"{weighted},T={T}", "lse", lse.cpu().reshape(S, T, H), l64, l32)


BWD_T = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 255, 256, 300, 1023)


@pytest.mark.parametrize("T", BWD_T)
def test_attn_backward_f32(lib, T):
    """attn_delta_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel against torch autograd through the float64 forward: d_qkv, the
    image key / value gradient d_ukv, delta; and the 16-bit d_qkv16 form with ukv_scale = 2^15 against the scaled reference.
    att / lse handed to the kernels are the float64 forward's, rounded to fp32."""
    H, D = 16, 1024
    variants = TF_VARIANTS if T < 1023 else TF_VARIANTS[1:2]
    for vi, (amk, p) in enumerate(variants):
        S = 2 if (T <= 128 or amk == "all") else 1
        t = R.tf_inputs(S, T, H, 57 * T + vi, amk, None, "half", offset=vi)
        drop = _mask(lib, SEED, STREAM, p, (S, H, T, T + 1), T + 1) if p > 0 else None
        o64, l64, P64 = R.tf_forward(t["qkv"], t["ukv"], t["am"], drop, F64)
        assert R.designated_weight_ok(P64, t["desig"], t["am"])
        att, lse = o64.float(), l64.float()
        g64 = R.tf_grads(t["qkv"], t["ukv"], t["am"], drop, t["d_att"], F64)
        g32 = R.tf_grads(t["qkv"], t["ukv"], t["am"], drop, t["d_att"], F32)
        dl64 = (t["d_att"].double() * att.double()).sum(-1)
        dl32 = (t["d_att"] * att).sum(-1)
        qkv, ukv, am = _dev(t["qkv"].reshape(S * T, 3 * D)), _dev(_ukv_rows(t, D)), _dev(t["am"])
        dO, datt, dlse = _dev(t["d_att"].reshape(S * T, D)), _dev(att.reshape(S * T, D)), _dev(lse.reshape(S * T, H))
        for mode16 in ((None,) if vi != 2 else (None, 0, 1)):
            delta = torch.full((S * T, H), math.nan, dtype=F32, device=DEV)
            d_qkv = torch.full((S * T, 3 * D), math.nan, dtype=F32, device=DEV)
            d_ukv = torch.zeros(S, ukv.shape[1], dtype=F32, device=DEV)
            d16 = torch.zeros(S * T, 3 * D, dtype=torch.int16, device=DEV) if mode16 is not None else None
            scale = 1.0 if mode16 is None else 32768.0
            _hip.check(lib.rgrg_debug_attn_backward_f32(_p(qkv), _p(ukv), ukv.shape[1], KCOL, _p(am), _p(dO), _p(datt), _p(dlse), _p(delta),
                                                        _p(d_qkv), _p(d_ukv), _p(d16), S, H, T, SEED, STREAM, p, int(bool(mode16)), scale, None),
                       "rgrg_debug_attn_backward_f32")
            torch.cuda.synchronize()
            case = f"T={T},S={S},am={amk},p={p},out16={mode16}"
            got_ukv = d_ukv.cpu()
            _check("attn_backward_f32", case, "d_ukv", got_ukv[:, KCOL:KCOL + 2 * D].reshape(S, 2, H, 64), g64[1] * scale, g32[1] * scale)
            assert not got_ukv[:, :KCOL].any() and not got_ukv[:, KCOL + 2 * D:].any(), "d_ukv was written outside its columns"
            _check("attn_backward_f32", case, "delta", delta.cpu().reshape(S, T, H), dl64, dl32)
            if mode16 is None:
                _check("attn_backward_f32", case, "d_qkv", d_qkv.cpu().reshape(S, T, 3, H, 64), g64[0], g32[0])
            else:
                _check("attn_backward_f32", case, f"d_qkv16_{'f16' if mode16 else 'bf16'}", R.from_bits(d16.cpu(), mode16).reshape(S, T, 3, H, 64),
                       R.rnd16(g64[0], mode16), R.rnd16(g32[0], mode16), mode16)


A16_T = (1, 2, 31, 32, 33, 63, 64, 95, 96, 97, 126, 127)


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("T", A16_T)
def test_attn_train16(lib, T, fp16):
    """attn16_fwd_kernel<F16> (att16, lse) and attn16_bwd_kernel<F16> (d_qkv16, d_ukv) on 16-bit operands; the reference rounds
    P x mask / dS where the kernels feed them to the matrix core (attn_reference docstring).  The backward reads the float64
    forward's output (rounded to the 16-bit type) and lse (rounded to fp32), like the reference backward."""
    H, D, S = 16, 1024, 2
    name = f"attn16_{'f16' if fp16 else 'bf16'}"
    for vi, (amk, p) in enumerate(TF_VARIANTS):
        t = R.tf_inputs(S, T, H, 91 * T + 4 * fp16 + vi, amk, fp16, "half" if vi != 2 else None, offset=vi)
        drop = _mask(lib, SEED, STREAM, p, (S, H, T, T + 1), T + 1) if p > 0 else None
        o64, l64, P64 = R.tf_forward(t["qkv"], t["ukv"], t["am"], drop, F64, p16=fp16)
        o32, l32, _ = R.tf_forward(t["qkv"], t["ukv"], t["am"], drop, F32, p16=fp16)
        if vi != 2:
            assert R.designated_weight_ok(P64, t["desig"], t["am"])
        qkv, am = _dev(R.to_bits(t["qkv"].reshape(S * T, 3 * D), fp16)), _dev(t["am"])
        ukv = _dev(R.to_bits(_ukv_rows(t, D), fp16))
        o16 = torch.zeros(S * T, D, dtype=torch.int16, device=DEV)
        lse = torch.full((S * T, H), math.nan, dtype=F32, device=DEV)
        _hip.check(lib.rgrg_debug_attn_train16(0, _p(qkv), _p(ukv), ukv.shape[1], KCOL, _p(am), _p(o16), _p(lse), None, None, None, S, H, T,
                                               SEED, STREAM, p, 1.0, fp16, None), "rgrg_debug_attn_train16 forward")
        torch.cuda.synchronize()
        case = f"T={T},am={amk},p={p}"
        _check(name + "_fwd", case, "att16", R.from_bits(o16.cpu(), fp16).reshape(S, T, H, 64), R.rnd16(o64, fp16), R.rnd16(o32, fp16), fp16)
        _check(name + "_fwd", case, "lse", lse.cpu().reshape(S, T, H), l64, l32)
        att, lsef = R.rnd16(o64, fp16).float(), l64.float()
        scale = 2.0 ** -7 if vi == 3 else 1.0
        b64 = R.tf_backward_manual(t["qkv"], t["ukv"], t["am"], drop, t["d_att"], att, lsef, F64, p16=fp16)
        b32 = R.tf_backward_manual(t["qkv"], t["ukv"], t["am"], drop, t["d_att"], att, lsef, F32, p16=fp16)
        dO, a16, dlse = _dev(R.to_bits(t["d_att"].reshape(S * T, D), fp16)), _dev(R.to_bits(att.reshape(S * T, D), fp16)), _dev(lsef.reshape(S * T, H))
        d16 = torch.zeros(S * T, 3 * D, dtype=torch.int16, device=DEV)
        d_ukv = torch.zeros(S, ukv.shape[1], dtype=F32, device=DEV)
        _hip.check(lib.rgrg_debug_attn_train16(1, _p(qkv), _p(ukv), ukv.shape[1], KCOL, _p(am), _p(a16), _p(dlse), _p(dO), _p(d16), _p(d_ukv), S, H, T,
                                               SEED, STREAM, p, scale, fp16, None), "rgrg_debug_attn_train16 backward")
        torch.cuda.synchronize()
        _check(name + "_bwd", case, "d_qkv16", R.from_bits(d16.cpu(), fp16).reshape(S, T, 3, H, 64), R.rnd16(b64[0], fp16), R.rnd16(b32[0], fp16), fp16)
        # d_ukv is fp32 but sums products of 16-bit-rounded P / dS: operands on a rounding boundary may fall either way (flip_floor)
        dOh, qh = t["d_att"].permute(0, 2, 1, 3), t["qkv"][:, :, 0].permute(0, 2, 1, 3)
        flips = max(R.flip_floor(b64[3][0], b32[3][0], dOh, fp16), R.flip_floor(b64[3][1], b32[3][1], qh, fp16)) * scale
        _check(name + "_bwd", case, "d_ukv", d_ukv.cpu()[:, KCOL:KCOL + 2 * D].reshape(S, 2, H, 64), b64[1] * scale, b32[1] * scale,
               extra_floor=flips)


def test_attn_train16_refuses_128_tokens(lib):
    """T + 1 = 129 keys do not fit the one-workgroup kernels: attn16_supported(128) is false and both directions fail with EINVAL."""
    S, H, T, D = 1, 16, 128, 1024
    z = torch.zeros(S * T, 3 * D, dtype=torch.int16, device=DEV)
    u = torch.zeros(S, 2 * D, dtype=torch.int16, device=DEV)
    o = torch.zeros(S * T, D, dtype=torch.int16, device=DEV)
    lse = torch.zeros(S * T, H, dtype=F32, device=DEV)
    du = torch.zeros(S, 2 * D, dtype=F32, device=DEV)
    for backward in (0, 1):
        rc = lib.rgrg_debug_attn_train16(backward, _p(z), _p(u), 2 * D, 0, None, _p(o), _p(lse), _p(o), _p(z.clone()), _p(du), S, H, T, 0, 0, 0.0, 1.0, 0, None)
        assert rc == RGRG_EINVAL


@pytest.mark.parametrize("nkeys", (17, 65))
def test_attn_decode_f32_masked_above_256_sequences(lib, nkeys):
    """S * H > 4096: the product's rule (ni = 0) picks attn_decode_kernel<false, 2, true> - float64-checked like the small-S form,
    and bit-identical with the forced 2- and 9-key instantiations."""
    d = R.decode_inputs(260, 16, nkeys, nkeys + 1, 5 * nkeys, False, "random", None, "half", tile=16)
    r64, r32 = _decode_refs(d)
    got0 = _run_decode(lib, d, ni=0)
    _check("attn_decode_f32", f"nkeys={nkeys},S=260,mask=random,rule", "out", got0[0], r64[0], r32[0])
    assert torch.equal(_run_decode(lib, d, ni=2)[0], got0[0]), "ni = 0 did not select the 2-key instantiation for S * H > 4096"
    _check("attn_decode_f32", f"nkeys={nkeys},S=260,mask=random,ni=9", "out", _run_decode(lib, d, ni=9)[0], r64[0], r32[0])


# ------------------------------------------------------------------------------------------------ the masked incremental forward
def _cached_inputs(S, T):
    g = torch.Generator().manual_seed(2024)
    feats = torch.randn(S, 1024, generator=g)
    ids = torch.randint(0, 50257, (S, T), generator=g)
    am = torch.ones(S, T)
    am[::2, 1:3] = 0.0   # padding INSIDE the prompt of every other row
    am[1::4, 0] = 0.0
    return feats, ids, am


def test_forward_cached_refuses_a_mask_in_16_bit_mode_above_the_row_limit(lib):
    """rgrg_decoder_forward_cached called directly (no Python mirror, which forces precision 0): in precision modes 1 and 2 above
    the row limit the step would read the 16-bit cache, whose kernel has no mask - the call fails with RGRG_EINVAL and says why;
    it never returns RGRG_OK with unmasked logits.  The same call without a mask, and the masked call in mode 0, succeed."""
    from conftest import gpu_model
    eng = gpu_model("bench").engine()
    S, T = 72, 3
    feats, ids, am = (_dev(t) for t in _cached_inputs(S, T))
    dec = eng._get_decoder(S, 8)
    eng._cached = None
    logits = torch.empty(S, T, eng.vocab, dtype=F32, device=DEV)
    try:
        for mode in (1, 2):
            _hip.check(lib.rgrg_decoder_set_precision(dec, mode), "rgrg_decoder_set_precision")
            assert S > lib.rgrg_decoder_row_limit(dec)
            rc = lib.rgrg_decoder_forward_cached(dec, _p(feats), _p(ids), None, _p(am), S, T, 0, _p(logits), None)
            assert rc == RGRG_EINVAL and b"attention_mask" in lib.rgrg_last_error()
            _hip.check(lib.rgrg_decoder_forward_cached(dec, _p(feats), _p(ids), None, None, S, T, 0, _p(logits), None), "unmasked, 16-bit mode")
            torch.cuda.synchronize()
            assert bool(torch.isfinite(logits).all())
    finally:
        _hip.check(lib.rgrg_decoder_set_precision(dec, 0), "rgrg_decoder_set_precision")
    _hip.check(lib.rgrg_decoder_forward_cached(dec, _p(feats), _p(ids), None, _p(am), S, T, 0, _p(logits), None), "masked, fp32 mode")
    torch.cuda.synchronize()


def test_forward_cached_masked_above_256_sequences_equals_small_batches():
    """fp32, padded attention_mask, 260 sequences (S * 16 heads > 4096: attn_decode_kernel<false, 2, true>) against the same rows
    fed 4 at a time (<false, 9, true>, the form the float64 test above pins).  Bound: the 2e-3 on logits that every fp32
    end-to-end pin of this suite uses (the GEMMs of the two paths differ, the attention kernels are bit-identical); dropping
    the mask must move the same logits by far more than that."""
    from conftest import gpu_model
    eng = gpu_model("bench").engine()
    S, T = 260, 4
    feats, ids, am = _cached_inputs(S, T)
    big, _ = eng.forward_cached(feats.to(DEV), ids.to(DEV), 0, cache_len=8, attention_mask=am.to(DEV))
    big = big.cpu()
    nomask, _ = eng.forward_cached(feats.to(DEV), ids.to(DEV), 0, cache_len=8)
    rows = [0, 1, 2, 3, 128, 129, 130, 131, 256, 257, 258, 259]
    for r0 in (0, 4, 8):
        rr = rows[r0:r0 + 4]
        small, _ = eng.forward_cached(feats[rr].to(DEV), ids[rr].to(DEV), 0, cache_len=8, attention_mask=am[rr].to(DEV))
        err = float((big[rr] - small.cpu()).abs().max())
        moved = float((nomask.cpu()[rr] - small.cpu()).abs().max())
        print(f"ATTNPARITY kernel=forward_cached_masked case=rows={rr} out=logits err={err:.3e} bound=2e-3 unmasked_moves={moved:.3e}")
        assert err <= 2e-3 and moved > 2e-2
