"""The consumer instantiations with a compile-time activation (rgrg_amd/csrc/gemm_bf16.hip, gemm_bf16_glds_kernel CACT: c_fc and
c_attn of the many-sequence 16-bit decode step - GPT2Block's ln_1 + attn c_attn and ln_2 + mlp c_fc + NewGELU,
src/language_model/language_model.py:338-366) against the instantiation with the run-time switch, which RGRG_CONS_EPI=0 keeps
alive.  The switch is read per launch, so both run in one process on the same buffers; rgrg_debug_cons_epilogue_launches
tells which one a launch took.  Every comparison is on raw bits.

  1. the c_fc form through rgrg_debug_linear_bf16_ln_kp(kp = 0): 16-bit Y16 or fp32 Y, act NONE / GELU_NEW, row pitch N and N + 8;
  2. the c_attn form through rgrg_debug_linear_bf16_ln_kv: fp32 q and both 16-bit cache planes, one slot per launch or none;
  3. launches the new epilogue must leave to the old one (pitch, alignment, activation, ragged column tile);
  4. the whole greedy step in fresh child processes: token ids, last logits and every written cache slot of every layer equal.

The new epilogue exists for the 64 x 64 tile only.  The launcher's heuristic gives a GEMM with N <= 64 the 128 x 64 tile, so the
N = 64 launches of part 1 run the old epilogue whatever the switch says (their counter difference is 0); N = 192 takes 64 x 64.
"""
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T16 = {0: torch.bfloat16, 1: torch.float16}
K = 1024                 # the consumer form requires the normalised width
GUARD = 2                # rows behind the launch's last row that nobody may touch
ROWS = 134 + GUARD
SENT16 = 0x5A5B          # int16 sentinel of 16-bit outputs (a finite value in both types)
SENT32 = 0x7FC12345      # int32 sentinel of fp32 outputs (a NaN)
SWITCH = "RGRG_CONS_EPI"
ACT_NONE, ACT_RELU, ACT_GELU_NEW = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


@pytest.fixture(autouse=True)
def _switch_restored():
    old = os.environ.get(SWITCH)
    yield
    if old is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = old


@functools.lru_cache(maxsize=None)
def _operands(N, fp16):
    """136 rows of the residual stream as 16 bit with their 16 (sum, sum of squares) slots, a 16-bit [N, 1024] weight, its column
    sums and a shift, made once per (N, type)."""
    g = torch.Generator().manual_seed(7000 * fp16 + N)
    x = torch.randn(ROWS, K, generator=g) * 1.5 + 0.25
    blocks = x.view(ROWS, 16, 64)
    stats = torch.stack((blocks.sum(-1), (blocks * blocks).sum(-1)), dim=-1).contiguous()      # [ROWS][16][2]
    a = x.to(T16[fp16]).view(torch.int16).to(DEV)
    w16 = (torch.randn(N, K, generator=g) / K ** 0.5).to(T16[fp16])
    colsum = w16.float().sum(-1)
    shift = torch.randn(N, generator=g) * 0.1
    return a, w16.view(torch.int16).to(DEV), shift.to(DEV), stats.to(DEV), colsum.to(DEV)


def _launched(lib, before, on, takes_new):
    assert lib.rgrg_debug_cons_epilogue_launches() - before == (1 if on and takes_new else 0), "the launch did not take the epilogue the switch names"


# ------------------------------------------------------------------------------------------------ 1. the c_fc form
def _c_fc(lib, N, fp16, M, r0, act, ldy, out16, on, takes_new=True, byte_off=0):
    a, w, shift, stats, colsum = _operands(N, fp16)
    rows = r0 + M + GUARD
    if out16:
        y = torch.full((rows * ldy + 8,), SENT16, dtype=torch.int16, device=DEV)
    else:
        y = torch.full((rows * ldy + 8,), SENT32, dtype=torch.int32, device=DEV)
    ptr = y.data_ptr() + byte_off + r0 * ldy * y.element_size()
    os.environ[SWITCH] = "1" if on else "0"
    before = lib.rgrg_debug_cons_epilogue_launches()
    _hip.check(lib.rgrg_debug_linear_bf16_ln_kp(a[r0:].data_ptr(), w.data_ptr(), shift.data_ptr(), None, None if out16 else ptr, ptr if out16 else None,
                                                None, None, stats[r0:].data_ptr(), colsum.data_ptr(), M, N, K, ldy, act, fp16, 0, None),
               "rgrg_debug_linear_bf16_ln_kp")
    torch.cuda.synchronize()
    _launched(lib, before, on, takes_new)
    off = byte_off // y.element_size()
    return y.cpu()[off:off + rows * ldy].view(rows, ldy), y.cpu()


def _check_rows(new, old, N, M, r0, sent):
    rows = slice(r0, r0 + M)
    assert torch.equal(new[rows, :N], old[rows, :N]), "the result differs"
    assert bool((new[rows, :N] != sent).any(dim=1).all()), "a row was not written"
    rest = new.clone()
    rest[rows, :N] = sent
    assert bool((rest == sent).all()), f"an element outside rows [{r0}, {r0 + M}) x columns [0, {N}) was written"


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("act", (ACT_NONE, ACT_GELU_NEW))
@pytest.mark.parametrize("M,r0", ((1, 0), (64, 0), (70, 0), (70, 64)))   # one row; a full tile; + a ragged 6-row tile; rows 64 .. 133 of 134
@pytest.mark.parametrize("N", (64, 192))
def test_c_fc_compile_time_epilogue_equals_the_run_time_one(lib, N, M, r0, act, fp16):
    takes_new = N > 64   # N = 64 runs on the 128 x 64 tile (module docstring)
    for out16 in (True, False):
        for ldy in (N, N + 8):
            old, old_all = _c_fc(lib, N, fp16, M, r0, act, ldy, out16, on=False)
            new, new_all = _c_fc(lib, N, fp16, M, r0, act, ldy, out16, on=True, takes_new=takes_new)
            sent = SENT16 if out16 else SENT32
            _check_rows(new, old, N, M, r0, sent)
            _check_rows(old, old, N, M, r0, sent)
            assert bool((new_all[-8:] == sent).all())


# ------------------------------------------------------------------------------------------------ 2. the c_attn form
T_SLOTS = 4


def _c_attn(lib, H, fp16, M, step, on):
    N, D = 3 * H * 64, H * 64
    a, w, shift, stats, colsum = _operands(N, fp16)
    rows = M + GUARD
    y = torch.full((rows, N), SENT32, dtype=torch.int32, device=DEV)
    kc = torch.full((rows, H, T_SLOTS, 64), SENT16, dtype=torch.int16, device=DEV)
    vc = torch.full((rows, H, T_SLOTS, 64), SENT16, dtype=torch.int16, device=DEV)
    step_dev = torch.tensor([step], dtype=torch.int32, device=DEV)
    os.environ[SWITCH] = "1" if on else "0"
    before = lib.rgrg_debug_cons_epilogue_launches()
    _hip.check(lib.rgrg_debug_linear_bf16_ln_kv(a.data_ptr(), w.data_ptr(), shift.data_ptr(), y.data_ptr(), stats.data_ptr(), colsum.data_ptr(),
                                                kc.data_ptr(), vc.data_ptr(), step_dev.data_ptr(), M, H, T_SLOTS, K, N, fp16, None),
               "rgrg_debug_linear_bf16_ln_kv")
    torch.cuda.synchronize()
    _launched(lib, before, on, True)
    return y.cpu(), kc.cpu(), vc.cpu(), D


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("step", (0, 2, 3))      # slots 1 and 3; slot 4 == T_slots: nothing may be written
@pytest.mark.parametrize("M", (1, 64, 70))
@pytest.mark.parametrize("H", (1, 2))            # N = 192 / 384
def test_c_attn_compile_time_epilogue_equals_the_run_time_one(lib, H, M, step, fp16):
    y0, k0, v0, D = _c_attn(lib, H, fp16, M, step, on=False)
    y1, k1, v1, _ = _c_attn(lib, H, fp16, M, step, on=True)
    slot = step + 1
    for y in (y0, y1):
        assert bool((y[:M, :D] != SENT32).any(dim=1).all()), "a q row was not written"
        rest = y.clone()
        rest[:M, :D] = SENT32
        assert bool((rest == SENT32).all()), "fp32 Y was written outside the q columns of the launch's rows"
    assert torch.equal(y1, y0), "q differs"
    for name, c0, c1 in (("k", k0, k1), ("v", v0, v1)):
        assert torch.equal(c1, c0), f"the {name} plane differs"
        for c in (c0, c1):
            rest = c.clone()
            if slot < T_SLOTS:
                assert bool((c[:M, :, slot] != SENT16).any(dim=-1).all()), f"a {name} cache row was not written"
                rest[:M, :, slot] = SENT16
            assert bool((rest == SENT16).all()), f"the {name} plane was written outside slot {slot} of the launch's rows"
    if slot < T_SLOTS:
        assert not torch.equal(k1[:M, :, slot], v1[:M, :, slot])


# ------------------------------------------------------------------------------------------------ 3. launches that must fall back
@pytest.mark.parametrize("case", ("ldy % 8 != 0", "Y16 base + 2 bytes", "act RELU", "N = 96"))
def test_launches_outside_the_eligibility_keep_the_run_time_epilogue(lib, case):
    N, ldy, act, byte_off = 192, 192, ACT_NONE, 0
    if case == "ldy % 8 != 0":
        ldy = N + 4
    elif case == "Y16 base + 2 bytes":
        byte_off = 2
    elif case == "act RELU":
        act = ACT_RELU
    else:
        N = ldy = 96
    M = 70
    old, old_all = _c_fc(lib, N, 0, M, 0, act, ldy, True, on=False, byte_off=byte_off)
    new, new_all = _c_fc(lib, N, 0, M, 0, act, ldy, True, on=True, takes_new=False, byte_off=byte_off)
    _check_rows(new, old, N, M, 0, SENT16)
    assert torch.equal(new_all, old_all)


# ------------------------------------------------------------------------------------------------ 4. the whole step
_STEP_CODE = (
    "import sys, hashlib, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "from conftest import gpu_model\n"
    "from rgrg_amd import _hip\n"
    "m = gpu_model('bench'); eng = m.engine(); out = {}\n"
    "for S in (130, 520):\n"
    "    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(S)).cuda()\n"
    "    ids = eng.greedy_decode(feats, 6, bf16=1)\n"
    "    lg = eng.last_logits(S).cpu()\n"
    "    kv = eng._kv\n"
    "    L, _, rows, Hh, T, _ = kv.shape\n"
    "    c16 = kv.view(torch.int16).reshape(-1)[:kv.numel()].reshape(L, 2, rows, Hh, T, 64)\n"   # 16-bit cache: same element strides
    "    dig = [hashlib.sha256(c16[l, p, :S, :, :ids.shape[1]].contiguous().cpu().numpy().tobytes()).hexdigest() for l in range(L) for p in range(2)]\n"
    "    out[S] = (ids.cpu(), lg, dig)\n"
    "out['cons'] = _hip.load().rgrg_debug_cons_epilogue_launches()\n"
    "torch.save(out, sys.argv[1])\n")


def test_greedy_step_equals_the_run_time_epilogue():
    """bf16 autocast, `bench` weights, 6 tokens; 130 sequences (one range, ragged tile) and 520 (forked row ranges, ragged last tile).
    Default against RGRG_CONS_EPI=0 in fresh child processes: ids, last logits and every written cache slot of every layer (SHA-256
    of the 16-bit planes over [S][H][tokens][64]) equal; the default took the new epilogue, the other never."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _STEP_CODE % (repo, os.path.join(repo, "tests"))
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, env_add in (("new", {}), ("old", {SWITCH: "0"})):
            path = os.path.join(tmp, name + ".pt")
            env = {k: v for k, v in os.environ.items() if k != SWITCH}
            r = subprocess.run([sys.executable, "-c", code, path], env=dict(env, **env_add), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res[name] = torch.load(path)
    assert res["new"]["cons"] > 0 and res["old"]["cons"] == 0
    for S in (130, 520):
        (ids1, lg1, dig1), (ids0, lg0, dig0) = res["new"][S], res["old"][S]
        assert ids1.shape[1] >= 2
        assert torch.equal(ids1, ids0), S
        assert torch.equal(lg1, lg0), S
        assert dig1 == dig0, (S, [i for i, (a, b) in enumerate(zip(dig1, dig0)) if a != b])
        assert len(set(dig1)) == len(dig1)   # the planes hold data (no two layers alike), not the zero fill
