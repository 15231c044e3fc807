"""The kernels behind prompts in a rolling session ALONE, through rgrg_debug_roll_prompt_step: the submit-init that
writes the prompt into the id ring, the retire pass that seats a sequence behind its prompt (len = P, tok = prompt[P - 1], pos = step =
P - 1) and roll_prompt_refill_kernel, which copies the prompt's keys / values from the ring to the row's cache.

Shapes: R = 5 and R = 300 (more than one 256-row pass of the retire workgroup; the rows under test straddle row 256), 2 layers, H = 2,
12 cache slots, max_prompt_length 6, n = 2, Cf = 3, C = 6, sequences 8 .. 13 (both rings wrap), prompt lengths 1, 2 and 6, an fp32, a
bf16 and an fp16 cache.  The state arrays, the id ring, the length words and the log-probs are those of the numpy model
(tests/rolling_prompt_reference.py, whose cases tests/test_rolling_prompt_reference.py shows to reject the named mutations); the cache
is compared BYTE for byte with: the pre-filled pattern everywhere, but slot 0 of a seated row = its feature row's image key / value in
the cache's rounding, and slots 1 .. P - 1 = the ring's bytes."""
import numpy as np
import pytest
import torch

import rolling_prompt_reference as P
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LAYERS, H, SLOTS, LD_UKV = 2, 2, 12, 2 * 2 * 2 * 64 + 8
C, N, CF, MP, L = 6, P.HOOK_N, P.HOOK_CF, P.HOOK_MP, P.HOOK_L
KV = {"fp32": (torch.float32, torch.int32, 0, 0), "bf16": (torch.bfloat16, torch.int16, 1, 0), "fp16": (torch.float16, torch.int16, 1, 1)}


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _bits(shape, bits, seed):
    """Uniform random BIT patterns of the element's width - NaNs, infinities, denormals and both zeros among them: ring and cache hold
    bytes as far as the copy is concerned, and they are compared as integers."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = (-2 ** 31, 2 ** 31) if bits == torch.int32 else (-2 ** 15, 2 ** 15)
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int64).to(bits)


def _run(lib, R, kv, case, ptok, plen, with_cache=True):
    name, S_before, submit, handout, retire, st0, arg, req = case
    dt, bits, kv16, fp16 = KV[kv]
    st = {k: _i32(v) for k, v in st0.items()}
    ids0, lens0 = np.full((C, L + 1), -1, dtype=np.int64), np.full(C, -99, dtype=np.int32)
    lp0 = np.full((C, L + 1), 7.5, dtype=np.float32)
    ids, lens, lp = torch.from_numpy(ids0.copy()).to(DEV), _i32(lens0), torch.from_numpy(lp0.copy()).to(DEV)
    cache0 = _bits((LAYERS, 2, R, H, SLOTS, 64), bits, 11)
    ring = _bits((LAYERS, 2, CF, H, MP, 64), bits, 13)
    ukv = torch.randn((CF, LD_UKV), generator=torch.Generator().manual_seed(17)) * 3.0
    cache, ring_d, ukv_d = cache0.clone().to(DEV), ring.to(DEV), ukv.to(DEV)
    a, r_, pt, pl = _i32(arg), torch.from_numpy(np.frombuffer(req.tobytes(), dtype=np.uint8).copy()).to(DEV), _i32(ptok), _i32(plen)
    kv_stride = R * H * SLOTS * 64
    rc = lib.rgrg_debug_roll_prompt_step(_p(st["seq"]), _p(st["len"]), _p(st["tok"]), _p(st["pos"]), _p(st["step"]), _p(st["shared"]), _p(a),
                                         _p(ids), _p(lp), L + 1, _p(lens), C, N, S_before, submit, handout, retire, R, L,
                                         _p(ukv_d) if with_cache else None, LD_UKV, _p(cache) if with_cache else None, 2 * kv_stride, kv_stride,
                                         H, SLOTS, LAYERS, kv16, fp16, _p(r_), _p(pt), _p(pl), _p(ring_d) if with_cache else None, MP, None)
    _hip.check(rc, "rgrg_debug_roll_prompt_step")
    torch.cuda.synchronize()
    got = dict(st={k: v.cpu().numpy() for k, v in st.items()}, ids=ids.cpu().numpy(), lens=lens.cpu().numpy(), lp=lp.cpu().numpy(),
               cache=cache.cpu())
    # the model on the same arrays
    wst = {k: v.copy() for k, v in st0.items()}
    hand, ret = P.prompt_step(wst, arg, ids0, lens0, lp0, C, N, S_before, submit, handout, retire, L, ptok.astype(np.int64), plen, req)
    want_cache = cache0.clone()
    for r, q, f, p in hand + ret:
        slot0 = ukv[f, :LAYERS * 2 * H * 64].reshape(LAYERS, 2, H, 64).to(dt)      # slot 0 as today (round to nearest even)
        want_cache[:, :, r, :, 0] = slot0.view(bits)
        want_cache[:, :, r, :, 1:p] = ring[:, :, f, :, 1:p]
    want = dict(st=wst, ids=ids0, lens=lens0, lp=lp0, cache=want_cache)
    return got, want, hand + ret, bits


@pytest.mark.parametrize("kv", sorted(KV))
@pytest.mark.parametrize("R", (5, 300))
@pytest.mark.parametrize("case", range(4), ids=[c[0] for c in P.hook_cases(5)])
def test_prompt_step_equals_the_model_and_touches_nothing_else(lib, case, R, kv):
    ptok, plen = P.hook_rings()
    c = P.hook_cases(R)[case]
    got, want, seated, bits = _run(lib, R, kv, c, ptok, plen)
    for k in want["st"]:
        assert np.array_equal(got["st"][k], want["st"][k]), (c[0], R, k, got["st"][k][-50:].tolist(), want["st"][k][-50:].tolist())
    assert np.array_equal(got["ids"], want["ids"]), (c[0], got["ids"].tolist(), want["ids"].tolist())
    assert np.array_equal(got["lens"], want["lens"]) and np.array_equal(got["lp"], want["lp"])
    g, w = got["cache"], want["cache"]      # (integers: the element's bits)
    F = 0 if R == 5 else 253
    for r, q, f, p in seated:                                   # the message names the first place that differs
        assert torch.equal(g[:, :, r, :, 0], w[:, :, r, :, 0]), (c[0], "slot 0", r, q)
        assert torch.equal(g[:, :, r, :, 1:p], w[:, :, r, :, 1:p]), (c[0], "prompt slots", r, q, p)
        assert torch.equal(g[:, :, r, :, p:], w[:, :, r, :, p:]), (c[0], "slots behind the prompt", r, q, p)
    assert torch.equal(g, w), (c[0], "a byte outside the seated rows' slots 0 .. P - 1 changed")
    if c[0] == "submit_handout":
        assert [(r - F, q, p) for r, q, f, p in seated] == [(1, 10, 6), (3, 11, 6), (4, 12, 1)]
    if c[0] == "retire_and_seat":
        assert [(r - F, q, p) for r, q, f, p in seated] == [(0, 13, 1)] and got["lens"].tolist() == [2, -99, 4, -4, -99, 7]
    if c[0] == "cancel_before_first_step":
        assert got["lens"][11 % C] == -6 and seated == []
    if c[0] == "no_refills":
        assert seated == [] and got["st"]["shared"][P.REFILLS] == 0


def test_state_alone_without_a_cache(lib):
    """kv = ukv = pkv = NULL: the retire pass alone, the same state."""
    ptok, plen = P.hook_rings()
    c = P.hook_cases(300)[0]
    got, want, _, _ = _run(lib, 300, "fp32", c, ptok, plen, with_cache=False)
    assert all(np.array_equal(got["st"][k], want["st"][k]) for k in want["st"]) and np.array_equal(got["ids"], want["ids"])


def test_hook_refusals(lib):
    ptok, plen = P.hook_rings()
    c = P.hook_cases(5)[0]
    bad = plen.copy()
    bad[1] = MP + 1
    with pytest.raises(_hip.RgrgHipError, match="prompt ring row 1"):
        _run(lib, 5, "fp32", c, ptok, bad)
    bad[1] = 0
    with pytest.raises(_hip.RgrgHipError, match="prompt ring row 1"):
        _run(lib, 5, "fp32", c, ptok, bad)
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(64, dtype=torch.int64, device=DEV)
    def args(mp, L_):
        return [_p(z)] * 7 + [_p(i64), None, L_, _p(z), C, N, 0, 0, 0, 1, 5, L_, None, 0, None, 0, 0, H, 0, 0, 0, 0, None, _p(z), _p(z), None, mp, None]

    assert lib.rgrg_debug_roll_prompt_step(*args(9, 9)) != 0          # max_prompt_length >= max_length
    assert lib.rgrg_debug_roll_prompt_step(*args(0, 9)) != 0          # no ring at all: the hook without prompts is the other one
