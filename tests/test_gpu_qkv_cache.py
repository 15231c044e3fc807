"""c_attn writes the new token's k / v straight into the 16-bit K/V cache, the decode attention reads q only.

Three levels, each against the path it replaces (RGRG_QKV_CACHE=0 keeps that path alive):
  1. the folded-LayerNorm consumer GEMM with the K/V-cache epilogue (rgrg_debug_linear_bf16_ln_kv) against the same GEMM with its
     fp32 [M, 3072] output (rgrg_debug_linear_bf16_ln): q columns bit-equal, cache slot step + 1 = the RNE rounding of the old k / v
     columns, everything else untouched;
  2. the q-only attention (rgrg_debug_attn_decode_qonly) against the 16-bit kernel that patches and stores the new k / v itself
     (rgrg_debug_attn_decode): output bit-equal, within the float64 reference's bound, cache not written;
  3. the whole greedy step, default against RGRG_QKV_CACHE=0, in fresh processes: token ids, last logits and the cache bit-equal.

Test 2 runs H = 4 heads where the issue that introduced it asked for 2: the 16-bit kernels take four heads per workgroup and their
launcher refuses any other multiple (tests/test_gpu_attention_kernels.py::test_attn_decode_einval), so 4 is the smallest head count
on which the reference variant runs at all.
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import attn_reference as R
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
SENT16 = 0x5A5B          # int16 sentinel of the cache planes (a finite 16-bit value in both types)
SENT32 = 0x7FC12345      # int32 sentinel of the q buffer (a NaN: reading it as data would show)


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ 1. the GEMM epilogue
H, D, KDIM, T_SLOTS = 16, 1024, 1024, 5
M_ROWS = 70              # one full 64-row tile + a ragged 6-row tile


def _gemm_inputs(fp16, rows):
    """Raw 16-bit residual rows, their (sum, sum of squares) slots, gain-scaled 16-bit weights, their column sums, a shift."""
    g = torch.Generator().manual_seed(77 + fp16)
    x = R.rnd16(torch.randn(rows, KDIM, generator=g) * 1.5 + 0.25, fp16)
    w = R.rnd16(torch.randn(3 * D, KDIM, generator=g) * 0.03, fp16)
    shift = torch.randn(3 * D, generator=g) * 0.1
    blocks = x.reshape(rows, 16, 64)
    stats = torch.stack((blocks.sum(dim=2), (blocks * blocks).sum(dim=2)), dim=2).contiguous()   # [rows][16][2]
    return (R.to_bits(x, fp16).to(DEV), R.to_bits(w, fp16).to(DEV), shift.to(DEV), stats.to(DEV), w.sum(dim=1).to(DEV))


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("step", (0, T_SLOTS - 2))   # the first writable slot and the last slot
@pytest.mark.parametrize("r0,cache_rows", ((0, 96), (64, 134)))   # whole buffers / a row range that starts at sequence 64 of 134
def test_c_attn_cache_epilogue_equals_the_fp32_row(lib, fp16, step, r0, cache_rows):
    M = M_ROWS
    a16, wb, shift, stats, colsum = _gemm_inputs(fp16, cache_rows)
    step_dev = torch.tensor([step], dtype=torch.int32, device=DEV)
    old = torch.zeros(cache_rows, 3 * D, dtype=F32, device=DEV)
    _hip.check(lib.rgrg_debug_linear_bf16_ln(a16[r0:].data_ptr(), _p(wb), _p(shift), None, old[r0:].data_ptr(), None, None, stats[r0:].data_ptr(),
                                             _p(colsum), M, 3 * D, KDIM, 3 * D, 0, fp16, None), "rgrg_debug_linear_bf16_ln")
    q = torch.full((cache_rows, 3 * D), SENT32, dtype=torch.int32, device=DEV)
    kc = torch.full((cache_rows, H, T_SLOTS, 64), SENT16, dtype=torch.int16, device=DEV)
    vc = kc.clone()
    _hip.check(lib.rgrg_debug_linear_bf16_ln_kv(a16[r0:].data_ptr(), _p(wb), _p(shift), q[r0:].data_ptr(), stats[r0:].data_ptr(), _p(colsum),
                                                kc[r0:].data_ptr(), vc[r0:].data_ptr(), _p(step_dev), M, H, T_SLOTS, KDIM, 3 * D, fp16, None),
               "rgrg_debug_linear_bf16_ln_kv")
    torch.cuda.synchronize()
    old, q, kc, vc = old.cpu(), q.cpu(), kc.cpu(), vc.cpu()
    rows = slice(r0, r0 + M)
    assert torch.equal(q[rows, :D], old[rows, :D].view(torch.int32)), "q columns differ from the fp32 GEMM"
    slot = step + 1
    for name, plane, cols in (("K", kc, slice(D, 2 * D)), ("V", vc, slice(2 * D, 3 * D))):
        want = R.to_bits(old[rows, cols].to(R.t16(fp16)).float(), fp16).reshape(M, H, 64)   # torch's round-to-nearest-even
        assert torch.equal(plane[rows, :, slot], want), f"{name} slot {slot} is not the 16-bit rounding of the old columns"
        rest = plane.clone()
        rest[rows, :, slot] = SENT16
        assert bool((rest == SENT16).all()), f"{name}: a slot other than {slot}, or a row outside [{r0}, {r0 + M}), was written"
    outside = q.clone()
    outside[rows, :D] = SENT32
    assert bool((outside == SENT32).all()), "the q buffer was written outside the q columns of the launch's rows"


def test_c_attn_cache_epilogue_needs_the_layernorm_slots(lib):
    """Only the folded-LayerNorm consumer has the epilogue: without the slots the hook refuses instead of leaving the cache unwritten."""
    a16, wb, shift, stats, colsum = _gemm_inputs(0, 64)
    z16 = torch.zeros(64 * H * T_SLOTS * 64, dtype=torch.int16, device=DEV)
    y = torch.zeros(64, 3 * D, device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = lib.rgrg_debug_linear_bf16_ln_kv(_p(a16), _p(wb), _p(shift), _p(y), None, _p(colsum), _p(z16), _p(z16), _p(step_dev), 64, H, T_SLOTS,
                                          KDIM, 3 * D, 0, None)
    assert rc != 0


# ------------------------------------------------------------------------------------------------ 2. the q-only attention
QO_S, QO_H = 3, 4


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("nkeys", (2, 9, 72, 73, 129))   # one group; one full group; one 72-key chunk; two chunks; a 128-token decode's last step
def test_q_only_attention_equals_the_patching_kernel(lib, nkeys, fp16):
    S, Hh = QO_S, QO_H
    Dh = Hh * 64
    slots = nkeys + 1
    d = R.decode_inputs(S, Hh, nkeys, slots, 4000 * nkeys + fp16, False, None, fp16, "half", tile=8 if nkeys < 40 else 72)
    slot = d["step"] + 1
    Kc, Vc = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])
    r64 = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, d["step"], None, None, F64, kv16=fp16)
    r32 = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, d["step"], None, None, F32, kv16=fp16)
    step_dev = torch.tensor([d["step"]], dtype=torch.int32, device=DEV)
    # the reference variant: fp32 q | k | v row, NaN in slot step + 1 (it patches the new k / v in and stores them)
    ld = 3 * Dh + 64
    qkv = torch.zeros(S, ld)
    qkv[:, :Dh], qkv[:, Dh:2 * Dh], qkv[:, 2 * Dh:3 * Dh] = d["q"].reshape(S, Dh), d["kn"].reshape(S, Dh), d["vn"].reshape(S, Dh)
    K_old, V_old = R.to_bits(d["K"], fp16).to(DEV), R.to_bits(d["V"], fp16).to(DEV)
    outs = {}
    qkv = qkv.to(DEV)
    for out16 in (False, True):
        out = torch.full((S * Dh,), float("nan"), dtype=F32, device=DEV)
        o16 = torch.zeros(S * Dh, dtype=torch.int16, device=DEV) if out16 else None
        Kp, Vp = K_old.clone(), V_old.clone()
        _hip.check(lib.rgrg_debug_attn_decode(_p(qkv), ld, _p(Kp), _p(Vp), _p(step_dev), _p(out), _p(o16), S, Hh,
                                              slots, None, None, 1, fp16, 0, 0, 0, None), "rgrg_debug_attn_decode")
        torch.cuda.synchronize()
        outs[out16] = (o16 if out16 else out).cpu()
    # the q-only variant: a compact q buffer, slot step + 1 pre-filled with the rounded new k / v
    Kq, Vq = d["K"].clone(), d["V"].clone()
    Kq[:, :, slot], Vq[:, :, slot] = R.rnd16(d["kn"], fp16), R.rnd16(d["vn"], fp16)
    Kq, Vq = R.to_bits(Kq, fp16).to(DEV), R.to_bits(Vq, fp16).to(DEV)
    K0, V0 = Kq.clone(), Vq.clone()
    qd = d["q"].reshape(S, Dh).contiguous().to(DEV)
    for out16 in (False, True):
        out = torch.full((S * Dh,), float("nan"), dtype=F32, device=DEV)
        o16 = torch.zeros(S * Dh, dtype=torch.int16, device=DEV) if out16 else None
        _hip.check(lib.rgrg_debug_attn_decode_qonly(_p(qd), Dh, _p(Kq), _p(Vq), _p(step_dev), _p(out), _p(o16), S, Hh, slots, fp16, 0, None),
                   "rgrg_debug_attn_decode_qonly")
        torch.cuda.synchronize()
        got = (o16 if out16 else out).cpu()
        if out16:
            assert torch.equal(got, outs[True]), "out16 differs from the patching kernel"
        else:
            assert torch.equal(got.view(torch.int32), outs[False].view(torch.int32)), "out differs from the patching kernel"
            r = R.compare(got.reshape(S, Hh, 64), r64[0], r32[0])   # the bound of test_gpu_attention_kernels.py::test_attn_decode_kv16
            print(f"ATTNPARITY kernel=attn_decode_kv16_qonly_{'f16' if fp16 else 'bf16'} case=nkeys={nkeys} err={r['err']:.3e} "
                  f"noise={r['noise']:.3e} bound={r['bound']:.3e} used={r['used']:.3f}")
            assert r["ok"], f"max|got - ref64| = {r['err']:.3e} exceeds {r['bound']:.3e}"
        assert torch.equal(Kq, K0) and torch.equal(Vq, V0), "the q-only kernel wrote to the cache"


def test_q_only_attention_einval(lib):
    z = torch.zeros(4 * 6 * 4 * 64, dtype=torch.int16, device=DEV)
    q = torch.zeros(4, 6 * 64, device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.rgrg_debug_attn_decode_qonly(_p(q), 6 * 64, _p(z), _p(z), _p(step_dev), _p(q), None, 4, 6, 4, 0, 0, None) != 0   # H % 4
    assert lib.rgrg_debug_attn_decode_qonly(_p(q), 64, _p(z), _p(z), _p(step_dev), _p(q), None, 4, 4, 4, 0, 0, None) != 0        # ld_q < H * 64


# ------------------------------------------------------------------------------------------------ 3. the whole step
_STEP_CODE = (
    "import sys, hashlib, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "from conftest import gpu_model\n"
    "m = gpu_model('bench'); eng = m.engine(); out = {}\n"
    "for S in (130, 520):\n"
    "    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(S)).cuda()\n"
    "    ids = eng.greedy_decode(feats, 6, bf16=1)\n"
    "    lg = eng.last_logits(S).cpu()\n"
    "    assert eng.kv_format_in_use(S) == 1\n"
    "    kv = eng._kv\n"
    "    L, _, rows, Hh, T, _ = kv.shape\n"
    "    c16 = kv.view(torch.int16).reshape(-1)[:kv.numel()].reshape(L, 2, rows, Hh, T, 64)\n"   # 16-bit cache: same element strides
    "    dig = [hashlib.sha256(c16[l, p, :S, :, :ids.shape[1]].contiguous().cpu().numpy().tobytes()).hexdigest() for l in range(L) for p in range(2)]\n"
    "    out[S] = (ids.cpu(), lg, dig)\n"
    "torch.save(out, sys.argv[1])\n")


def test_greedy_step_equals_the_fp32_row_path():
    """bf16 autocast, `bench` weights, 6 tokens; 130 sequences (one range, ragged tile) and 520 (forked row ranges, ragged last tile).
    Default against RGRG_QKV_CACHE=0 (read once per decoder -> child processes): ids, last logits and every written cache slot
    of every layer (SHA-256 of the 16-bit planes over [S][H][tokens][64]) equal."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _STEP_CODE % (repo, os.path.join(repo, "tests"))
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, env_add in (("new", {}), ("old", {"RGRG_QKV_CACHE": "0"})):
            path = os.path.join(tmp, name + ".pt")
            env = {k: v for k, v in os.environ.items() if k != "RGRG_QKV_CACHE"}
            r = subprocess.run([sys.executable, "-c", code, path], env=dict(env, **env_add), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res[name] = torch.load(path)
    for S in (130, 520):
        (ids1, lg1, dig1), (ids0, lg0, dig0) = res["new"][S], res["old"][S]
        assert ids1.shape[1] >= 2
        assert torch.equal(ids1, ids0), S
        assert torch.equal(lg1, lg0), S
        assert dig1 == dig0, (S, [i for i, (a, b) in enumerate(zip(dig1, dig0)) if a != b])
        assert len(set(dig1)) == len(dig1)   # the planes hold data (no two layers alike), not the zero fill
