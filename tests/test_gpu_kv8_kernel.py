"""attn_decode_kv8_wave_kernel ALONE against the float64 reference (tests/kv8_reference.py over tests/attn_reference.py), through
rgrg_debug_attn_decode_kv8 - the product's launcher on caller-provided buffers.  One launch per case, every output element
compared: max |got - ref64| <= MARGIN * max |ref32 - ref64| + one ulp of the output type at max |ref| (attn_reference.compare; the
power of that bound on these shapes is shown on the CPU in tests/test_kv8_reference.py).  Each figure is printed before it is
asserted (lines starting with ATTNPARITY).  The kernel forms chunks of 144 keys and a tail in steps of 16."""
import math

import pytest
import torch

import attn_reference as R
import kv8_reference as K8
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


def _check(case, name, got, ref64, ref32, out16):
    r = R.compare(got, ref64, ref32, out16)
    print(f"ATTNPARITY kernel=attn_decode_kv8 case={case} out={name} err={r['err']:.3e} noise={r['noise']:.3e} floor={r['floor']:.3e} "
          f"bound={r['bound']:.3e} ratio={r['ratio']:.2f} used={r['used']:.3f}")
    assert r["ok"], f"attn_decode_kv8 {case} {name}: max|got - ref64| = {r['err']:.3e} exceeds {r['bound']:.3e} (noise {r['noise']:.3e}, floor {r['floor']:.3e})"


def _run(lib, d, *, out16=None, max_wgs=0, expect=0, kmask=None):
    """One launch on the inputs of kv8_reference.decode_inputs_kv8 -> (out fp32 [S,H,64], stored K bytes, stored V bytes [S,H,64]) on
    the CPU, after checking that every cache byte outside slot step + 1 is unchanged (canaries included)."""
    S, H, slots = d["S"], d["H"], d["slots"]
    D = H * 64
    ld = 3 * D + 64
    qkv = torch.zeros(S, ld)
    qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D] = d["q"].reshape(S, D), d["kn"].reshape(S, D), d["vn"].reshape(S, D)
    K, V = _dev(K8.to_bytes(d["K"])), _dev(K8.to_bytes(d["V"]))   # NaN (slots >= nkeys - 1) -> 0x7F
    slot = d["step"] + 1
    assert bool((K[:, :, slot:] == 0x7F).all()) and bool((V[:, :, slot:] == 0x7F).all())
    K0, V0 = K.clone(), V.clone()
    out = torch.full((S * D,), math.nan, dtype=F32, device=DEV)
    o16 = torch.zeros(S * D, dtype=torch.int16, device=DEV) if out16 is not None else None
    step = torch.tensor([d["step"]], dtype=torch.int32, device=DEV)
    dq, src, km = _dev(qkv), _dev(d["src"]), _dev(kmask)
    rc = lib.rgrg_debug_attn_decode_kv8(_p(dq), ld, _p(K), _p(V), _p(step), None if out16 is not None else _p(out), _p(o16), S, H, slots,
                                        _p(src), _p(km), int(bool(out16)), max_wgs, None)
    assert rc == expect, (rc, lib.rgrg_last_error())
    if expect:
        return None
    torch.cuda.synchronize()
    for plane, before in ((K, K0), (V, V0)):
        a, b = plane.clone(), before.clone()
        a[:, :, slot], b[:, :, slot] = 0, 0
        assert torch.equal(a, b), "a cache slot other than step + 1 was written"
    res = (R.from_bits(o16.cpu(), out16) if out16 is not None else out.cpu()).reshape(S, H, 64)
    return res, K.cpu()[:, :, slot], V.cpu()[:, :, slot]


def _refs(d, out16):
    Kc, Vc = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])
    f = lambda dt: K8.decode_forward_kv8(d["q"], d["kn"], d["vn"], Kc, Vc, d["step"], d["src"], dt, out16=out16)  # noqa: E731
    return f(F64), f(F32)


def _stored_ok(got, d):
    assert torch.equal(got[1], K8.to_bytes(d["kn"])) and torch.equal(got[2], K8.to_bytes(d["vn"])), \
        "slot step + 1 does not hold clamp + one rounding to nearest even of the new k / v"


@pytest.mark.parametrize("nkeys", K8.KV8_NKEYS)
def test_attn_decode_kv8(lib, nkeys):
    """Every (ancestor table, output type) variant at every key count; the designated key (half of the softmax) cycles through the
    image key, the new token's slot and both sides of every 16-key load step (the 144-key chunk boundaries are among them); one
    variant has plain N(0,1) scores.  Slots >= nkeys - 1 hold 0x7F (NaN); the grid capped at 70 / 50 workgroups (528 items over 280 / 200 waves) gives the same bits."""
    for ci, (S, with_src, out16, wt) in enumerate(K8.KV8_VARIANTS):
        d = K8.kv8_case(nkeys, ci)
        r64, r32 = _refs(d, out16)
        if wt:
            assert R.designated_weight_ok(r64[3][:, :, None, :], d["desig"]), "the designated key does not hold 0.2 .. 0.8 of the softmax"
        case = f"nkeys={nkeys},S={S},src={int(with_src)},out16={out16},w={wt}"
        got = _run(lib, d, out16=out16)
        _check(case, "out" if out16 is None else "out16", got[0], r64[0], r32[0], out16)
        _stored_ok(got, d)
        if S == 33:
            for cap in (70, 50):
                gc = _run(lib, d, out16=out16, max_wgs=cap)
                assert all(torch.equal(a, b) for a, b in zip(gc, got)), f"grid capped at {cap} workgroups differs"


@pytest.mark.parametrize("nkeys", (2, 17, 145, 289))
def test_attn_decode_kv8_stores_the_reference_bytes(lib, nkeys):
    """The new k / v beyond +-448 (saturation, never NaN), on ties, subnormal, below half the smallest subnormal and -0: the bytes
    stored to slot step + 1 are torch's (clamp, one rounding to nearest even), and the large values take part as 448."""
    for with_src in (False, True):
        d = K8.decode_inputs_kv8(5, 16, nkeys, nkeys + 1, 77 * nkeys, with_src, "half", K8.KV8_STEP, edge_values="large")
        g = torch.Generator().manual_seed(nkeys)
        d["kn"][:, 1] = torch.randn(5, 64, generator=g) * 2.0 ** torch.randint(-12, 3, (5, 64), generator=g).float()
        d["vn"][:, 1] = torch.randn(5, 64, generator=g) * 2.0 ** torch.randint(-12, 10, (5, 64), generator=g).float()
        r64, r32 = _refs(d, None)
        got = _run(lib, d)
        _stored_ok(got, d)
        assert bool((got[2][:, 0, 16:21] == torch.tensor([0x7E, 0xFE, 0x7E, 0x7E, 0xFE], dtype=torch.uint8)).all())
        _check(f"edge_bytes,nkeys={nkeys},src={int(with_src)}", "out", got[0], r64[0], r32[0], None)


@pytest.mark.parametrize("weighted,nkeys", K8.KV8_BIG)
def test_attn_decode_kv8_large_scores(lib, weighted, nkeys):
    """A score of 60 holds the maximum in the first / in the last chunk: the running-softmax rescale and the m == -inf guards."""
    for ci, (S, with_src, out16, _) in enumerate(K8.KV8_VARIANTS[:K8.KV8_PLAIN]):
        d = K8.decode_inputs_kv8(min(S, 5), 16, nkeys, nkeys + 2, 9 * nkeys + ci, with_src, weighted, K8.KV8_CHUNK)
        r64, r32 = _refs(d, out16)
        got = _run(lib, d, out16=out16, max_wgs=7 if ci % 2 else 0)
        _check(f"{weighted},nkeys={nkeys},src={int(with_src)},out16={out16}", "out" if out16 is None else "out16", got[0], r64[0], r32[0], out16)
        _stored_ok(got, d)


def test_attn_decode_kv8_product_shape(lib):
    """S = 928, H = 16: the shape of the batch-32 decode step (3712 workgroups), at 65 keys, out16 as the step uses it."""
    d = K8.decode_inputs_kv8(928, 16, 65, 66, 5, False, None, edge_values=None)
    r64, r32 = _refs(d, 0)
    got = _run(lib, d, out16=0)
    _check("nkeys=65,S=928,src=0,out16=0,w=None", "out16", got[0], r64[0], r32[0], 0)
    _stored_ok(got, d)


def test_attn_decode_kv8_einval(lib):
    d = K8.decode_inputs_kv8(4, 16, 9, 12, 5)
    _run(lib, d, kmask=torch.zeros(4, 12), expect=RGRG_EINVAL)                       # no mask operand in this kernel
    _run(lib, K8.decode_inputs_kv8(4, 6, 9, 12, 5, weighted=None), expect=RGRG_EINVAL)   # H % 4
    # a plane of 2 GiB: refused before anything is launched (the buffers are never touched - one byte each is enough)
    one = torch.zeros(64, dtype=torch.uint8, device=DEV)
    qkv = torch.zeros(3 * 1024, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    S, T = 16384, 128   # 16384 * 16 * 128 * 64 B = 2 GiB
    rc = lib.rgrg_debug_attn_decode_kv8(_p(qkv), 3 * 1024, _p(one), _p(one), _p(step), _p(qkv), None, S, 16, T, None, None, 0, 0, None)
    assert rc == RGRG_EINVAL, rc
    assert b"2 GiB" in lib.rgrg_last_error()
