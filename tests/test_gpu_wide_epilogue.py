"""The staged epilogue of the 64 x 64 K-parity producer (rgrg_amd/csrc/gemm_kp.inc, WIDE: attn_proj / mlp_proj of the many-sequence
16-bit decode step - GPT2Block's attn c_proj / mlp c_proj plus the residual add, src/language_model/language_model.py:338-366)
against the epilogue it replaces, which RGRG_WIDE_EPI=0 keeps alive.  The switch is read per launch, so both run in one process on
the same buffers; rgrg_debug_wide_epilogue_launches tells which one a launch took.  Every comparison is on raw bits.

  1. the producer GEMM through rgrg_debug_linear_bf16_ln_kp: fp32 x written in place of the residual, its 16-bit copy and the 16
     LayerNorm statistics slots of every row equal; nothing outside the launch's rows is written (sentinels);
  2. the whole greedy step in fresh child processes: token ids, last logits and every written cache slot of every layer equal.

The consumer forms of the issue that introduced this file (c_fc, c_attn with the K/V-cache epilogue) have no staged epilogue in this
tree, so there is nothing of theirs to compare here.
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
N = 1024                 # the producer form requires the normalised width
GUARD = 2                # rows behind the launch's last row that nobody may touch
SENT16 = 0x5A5B          # int16 sentinel of the 16-bit copy (a finite value in both types)
SENT32 = 0x7FC12345      # int32 sentinel of the statistics slots (a NaN)
SWITCH = "RGRG_WIDE_EPI"


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
def _operands(K, fp16):
    """136 rows of 16-bit activations, a 16-bit [1024, K] weight, a shift and the fp32 residual stream, made once per (K, type)."""
    g = torch.Generator().manual_seed(1000 * fp16 + K)
    rows = 134 + GUARD
    a = (torch.randn(rows, K, generator=g)).to(T16[fp16]).view(torch.int16).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(T16[fp16]).view(torch.int16).to(DEV)
    shift = (torch.randn(N, generator=g) * 0.1).to(DEV)
    x = (torch.randn(rows, N, generator=g) * 1.5 + 0.25).to(DEV)
    return a, w, shift, x


def _producer(lib, K, fp16, M, r0, wide):
    a, w, shift, x0 = _operands(K, fp16)
    rows = r0 + M + GUARD
    x = x0[:rows].clone()                                                   # R == Y: in place, as the step runs it
    yb = torch.full((rows, N), SENT16, dtype=torch.int16, device=DEV)
    so = torch.full((rows, 16, 2), SENT32, dtype=torch.int32, device=DEV)
    os.environ[SWITCH] = "1" if wide else "0"
    before = lib.rgrg_debug_wide_epilogue_launches()
    _hip.check(lib.rgrg_debug_linear_bf16_ln_kp(a[r0:].data_ptr(), w.data_ptr(), shift.data_ptr(), x[r0:].data_ptr(), x[r0:].data_ptr(), None,
                                                yb[r0:].data_ptr(), so[r0:].data_ptr(), None, None, M, N, K, N, 0, fp16, 1, None),
               "rgrg_debug_linear_bf16_ln_kp")
    torch.cuda.synchronize()
    assert lib.rgrg_debug_wide_epilogue_launches() - before == (1 if wide else 0), "the launch did not take the epilogue the switch names"
    return x.cpu().view(torch.int32), yb.cpu(), so.cpu()


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("M,r0", ((1, 0), (64, 0), (70, 0), (70, 64)))   # one row; a full tile; + a ragged 6-row tile; rows 64 .. 133 of 134
@pytest.mark.parametrize("K", (1024, 4096))                               # attn_proj / mlp_proj
def test_producer_staged_epilogue_equals_the_c_layout_epilogue(lib, K, M, r0, fp16):
    x_old, yb_old, so_old = _producer(lib, K, fp16, M, r0, wide=False)
    x_new, yb_new, so_new = _producer(lib, K, fp16, M, r0, wide=True)
    rows = slice(r0, r0 + M)
    x0 = _operands(K, fp16)[3][:r0 + M + GUARD].cpu().view(torch.int32)
    assert not torch.equal(x_new[rows], x0[rows]), "the launch left its rows as they were"
    assert torch.equal(x_new[rows], x_old[rows]), "fp32 x differs"
    assert torch.equal(yb_new[rows], yb_old[rows]), "the 16-bit copy differs"
    assert torch.equal(so_new[rows], so_old[rows]), "a statistics slot differs"
    assert bool((yb_new[rows] != SENT16).any(dim=1).all()) and bool((so_new[rows] != SENT32).all()), "a row or a slot was not written"
    for name, got, fill in (("x", x_new, x0), ("the 16-bit copy", yb_new, torch.full_like(yb_new, SENT16)),
                            ("the statistics", so_new, torch.full_like(so_new, SENT32))):
        rest, want = got.clone(), fill.clone()
        rest[rows], want[rows] = 0, 0
        assert torch.equal(rest, want), f"{name}: a row outside [{r0}, {r0 + M}) was written"


def test_producer_keeps_the_c_layout_epilogue_where_rows_are_not_16_byte_pieces(lib):
    """ldy = 1028 keeps fp32 rows 16-byte aligned but not the 16-bit ones: the launcher must fall back, and the result must be the
    one of the switched-off launch."""
    a, w, shift, x0 = _operands(1024, 0)
    M, ldy = 70, 1028
    outs = []
    for wide in ("0", "1"):
        x = torch.zeros(M, ldy, device=DEV)
        x[:, :N] = x0[:M]
        yb = torch.full((M, ldy), SENT16, dtype=torch.int16, device=DEV)
        so = torch.full((M, 16, 2), SENT32, dtype=torch.int32, device=DEV)
        os.environ[SWITCH] = wide
        before = lib.rgrg_debug_wide_epilogue_launches()
        _hip.check(lib.rgrg_debug_linear_bf16_ln_kp(a.data_ptr(), w.data_ptr(), shift.data_ptr(), x.data_ptr(), x.data_ptr(), None, yb.data_ptr(),
                                                    so.data_ptr(), None, None, M, N, 1024, ldy, 0, 0, 1, None), "rgrg_debug_linear_bf16_ln_kp")
        torch.cuda.synchronize()
        assert lib.rgrg_debug_wide_epilogue_launches() == before
        outs.append((x.cpu().view(torch.int32), yb.cpu(), so.cpu()))
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    assert bool((outs[1][1][:, N:] == SENT16).all()) and bool((outs[1][0][:, N:] == 0).all())


# ------------------------------------------------------------------------------------------------ 2. the whole step
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
    "out['wide'] = _hip.load().rgrg_debug_wide_epilogue_launches()\n"
    "torch.save(out, sys.argv[1])\n")


def test_greedy_step_equals_the_c_layout_epilogue():
    """bf16 autocast, `bench` weights, 6 tokens; 130 sequences (one range, ragged tile) and 520 (forked row ranges, ragged last tile).
    Default against RGRG_WIDE_EPI=0 in fresh child processes: ids, last logits and every written cache slot of every layer (SHA-256
    of the 16-bit planes over [S][H][tokens][64]) equal; the default took the staged epilogue, the other never."""
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
    assert res["new"]["wide"] > 0 and res["old"]["wide"] == 0
    for S in (130, 520):
        (ids1, lg1, dig1), (ids0, lg0, dig0) = res["new"][S], res["old"][S]
        assert ids1.shape[1] >= 2
        assert torch.equal(ids1, ids0), S
        assert torch.equal(lg1, lg0), S
        assert dig1 == dig0, (S, [i for i, (a, b) in enumerate(zip(dig1, dig0)) if a != b])
        assert len(set(dig1)) == len(dig1)   # the planes hold data (no two layers alike), not the zero fill
