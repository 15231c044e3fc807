"""The weight-streaming GEMMs of <= 128 token rows ALONE against the float64 reference of tests/skinny_reference.py, through the
rgrg_debug_direct_pack / rgrg_debug_direct_linear / rgrg_debug_skinny_linear hooks (the shape rules, packing steps and kernel dispatch
of the product path on the test's own buffers):
  fused decode plan   rgrg_skinny_direct_f32<MT, MODE, LNF, W16>, rgrg_skinny_direct_half_f32, rgrg_lm_head_wave_f32<DX_COMBINE4> and
                      pack_weights16_scaled_kernel / ln_fold_vectors_kernel / packed16_colsum_kernel (rgrg_amd/csrc/skinny_direct.inc)
  prefill GEMMs       rgrg_skinny_gemm_f32<PW, MT>, rgrg_skinny_gemm_f32_wide, skinny_reduce_kernel, pack_weights_kernel (decoder.hip)
One launch per case (and a second one on the same inputs, whose every output must carry identical bits - the split-K atomics
included), every output element compared.  fp32 outputs: attn_reference.compare, MARGIN * max|ref32 - ref64| + 2^-23 max|ref|, the
constant activation row of a folded form apart from the other rows (skinny_reference).  Exact (torch.equal): the packed weights
against the host packing; xout against the fp32 host combine / embedding sum; Yf rows >= M zero; zero_acc zero over both accumulators,
both halves and every row tile; cand_val = the maximum of the Y values THE KERNEL wrote for the tile and cand_idx the lowest such
column, < N; the sentinel row of a row-major Y, its columns N .. ldy - 1, and the row tile behind the last one of every
fragment-major buffer untouched.  The cases whose row count is in skinny_reference.NAN_PAD_ROWS hold NaN in the pad rows of the
activations, the residual and the accumulators: every stored row < M must still meet its bound.  Each figure is printed before it
is asserted (lines starting with SKINNY); the worst ones observed on the MI355X are kept in profiles/skinny_parity.md.  For the
16-bit-weight forms behind a LayerNorm the distance from the true LayerNorm-then-linear is printed too (dist_true), not asserted
(vocabulary-sized cases: at 33 rows only).
"""
import ctypes as C
import math

import pytest
import torch

import skinny_reference as R
from attn_reference import compare, to_bits
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
RGRG_EINVAL = -1
SENT, SENT_I = -777.25, -7
GARBAGE = 123.5
KERNEL_NAMES = {R.RAN_GENERIC: "generic", R.RAN_HALF: "row_half", R.RAN_LM_WAVE: "lm_head_wave"}


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(t, dtype=None):
    return None if t is None else t.to(device=DEV, dtype=dtype or t.dtype).contiguous()


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.rgrg_last_error())


def _report(family, case, kernel, res):
    for name, r in res.items():
        print(f"SKINNY family={family} case={case} kernel={kernel} out={name} err={r['err']:.3e} noise={r['noise']:.3e} "
              f"bound={r['bound']:.3e} used={r['used']:.3f}")
    for name, r in res.items():
        assert r["ok"], f"{family} {case} {name}: err {r['err']:.3e} exceeds {r['bound']:.3e} (noise {r['noise']:.3e})"


def _with_sentinel(flat, extra):
    """A flat device buffer: `flat` followed by `extra` sentinel elements."""
    return torch.cat((flat.to(F32), torch.full((extra,), SENT, dtype=F32))).to(DEV)


# ------------------------------------------------------------------------------------------------ one-time packing
_PACKED = {}


def _pack(lib, form, N, w16):
    """rgrg_debug_direct_pack on the weights of a form, checked (once) against the host packing and the host folded vectors; the
    device buffers are what every launch of that form then reads."""
    key = (form, N, w16)
    if key in _PACKED:
        return _PACKED[key]
    f = R.FORMS[form]
    K, lnf = f["K"], bool(f["lnf"])
    w = R.weights(form, N, K)
    NT = (N + 15) // 16
    W, g, beta, bias = _dev(w["W"]), _dev(w["g"]), _dev(w["beta"]), _dev(w["bias"])
    packed = torch.full((NT * 16 * K + 64,), SENT, dtype=F32, device=DEV)
    packed16 = torch.full((NT * 16 * K + 64,), 0x7B7B, dtype=torch.int16, device=DEV) if w16 else None
    c1 = torch.full((N + 1,), SENT, dtype=F32, device=DEV) if lnf else None
    c2 = torch.full((N + 1,), SENT, dtype=F32, device=DEV) if lnf else None
    c1_16 = torch.full((NT * 16 + 1,), SENT, dtype=F32, device=DEV) if (lnf and w16) else None
    _ok(lib, lib.rgrg_debug_direct_pack(_p(W), _p(g), _p(beta), _p(bias), N, K, w16, _p(packed), _p(packed16), _p(c1), _p(c2), _p(c1_16),
                                        None), f"pack {key}")
    torch.cuda.synchronize()
    Wg = w["W"] * w["g"] if lnf else w["W"]
    want = R.pack_direct(Wg)
    assert torch.equal(packed[:-64].cpu(), want), f"packed fp32 weights of {key} differ from the host packing"
    assert bool((packed[-64:] == SENT).all())
    res = {}
    if lnf:
        r64, r32 = R.fold_vectors(w["W"], w["g"], w["beta"], w["bias"], F64), R.fold_vectors(w["W"], w["g"], w["beta"], w["bias"], F32)
        res["c1"], res["c2"] = compare(c1[:N].cpu(), r64[0], r32[0]), compare(c2[:N].cpu(), r64[1], r32[1])
        assert float(c1[N]) == SENT and float(c2[N]) == SENT
    if w16:
        fp16 = w16 == 2
        assert torch.equal(packed16[:-64].cpu(), to_bits(R.rnd16(want, fp16), fp16)), f"16-bit fragments of {key} differ from round16(packed)"
        assert bool((packed16[-64:] == 0x7B7B).all())
        if lnf:
            Wr = R.rnd16(Wg, fp16)
            res["c1_16"] = compare(c1_16[:N].cpu(), Wr.double().sum(dim=1), Wr.sum(dim=1))
            assert float(c1_16[N:NT * 16].abs().max() if NT * 16 > N else 0.0) == 0.0 and float(c1_16[NT * 16]) == SENT
    _report("pack", f"{form},N={N},w16={w16}", "pack", res)
    _PACKED[key] = {"P": packed16 if w16 else packed, "c1": c1_16 if (lnf and w16) else c1, "c2": c2, "bias": bias, "keep": (packed, c1)}
    return _PACKED[key]


# ------------------------------------------------------------------------------------------------ the fused plan
def _launch_fused(lib, c, pk):
    """One launch on fresh buffers.  Returns (got for judge_fused, kernel code, raw output buffers, structural checks name -> bool)."""
    M, N, K, NT, mode = c["M"], c["N"], c["K"], c["NT"], c["mode"]
    MT = R.tiles_of(M)
    rows = MT * 32
    fill = math.nan if c["nan_pad"] else 0.0
    a = _hip.DirectArgs()
    keep, raw, checks, got = [], {}, {}, {}

    def put(name, t):
        keep.append(t)
        setattr(a, name, _p(t))
        return t

    if mode in (R.DX_PLAIN, R.DX_COMBINE4):
        put("Xf", _dev(R.to_frag(c["X"], MT, fill)))
    if mode == R.DX_COMBINE4:
        put("part", _dev(R.acc_to_flat(c["A0"], c["A1"], MT, fill)))
    if mode >= R.DX_EMBED:
        put("wte", _dev(c["wte"]))
        put("step", torch.tensor([c["step"]], dtype=torch.int32, device=DEV))
        if mode == R.DX_EMBED:
            put("ids", _dev(c["ids"]))
            a.ld_ids = c["ids"].shape[1]
        else:
            put("tok_override", _dev(c["tok"]))
        if mode == R.DX_EMBED_TOKPOS:
            put("pos_override", _dev(c["pos"]))
    put("P", pk["P"])
    a.bias = _p(pk["c2"] if c["lnf"] else pk["bias"])
    a.c1 = _p(pk["c1"]) if c["lnf"] else None
    a.K, a.N, a.act = K, N, c["act"]
    xout = Y = Yf = acc = zacc = cv = ci = None
    if mode != R.DX_PLAIN and not c.get("cand"):
        xout = put("xout", torch.full(((MT + 1) * 32 * K,), SENT, dtype=F32, device=DEV))
    ldy = N + (7 if c.get("cand") else 8)
    if c["out"] == "Y":
        Y = put("Y", torch.full((M + 1, ldy), SENT, dtype=F32, device=DEV))
        a.ldy = ldy
    elif c["out"] == "Yf":
        if c.get("R") is not None:     # in place, as the model does: the residual is the output buffer
            Yf = put("Yf", _with_sentinel(R.to_frag(c["R"], MT, fill), 32 * N))
            a.Rf = _p(Yf)
            zacc = put("zero_acc", _with_sentinel(torch.full((MT * 2 * 32 * N,), GARBAGE), 2 * 32 * N))
        else:
            Yf = put("Yf", _with_sentinel(torch.full((rows * N,), math.nan), 32 * N))
    else:
        acc = put("part_out", _with_sentinel(torch.zeros(MT * 2 * 32 * N), 2 * 32 * N))
    if c.get("cand"):
        cv = put("cand_val", torch.full((M + 1, NT), SENT, dtype=F32, device=DEV))
        ci = put("cand_idx", torch.full((M + 1, NT), SENT_I, dtype=torch.int32, device=DEV))
    ran = C.c_int(-1)
    _ok(lib, lib.rgrg_debug_direct_linear(C.byref(a), mode, int(c["lnf"]), c["w16"], M, C.byref(ran), None), c["name"])
    torch.cuda.synchronize()
    if Y is not None:
        raw["Y"] = Y.cpu()
        got["Y"] = raw["Y"][:M, :N].contiguous()
        checks["Y sentinel row and columns N .. ldy - 1 untouched"] = bool((raw["Y"][M] == SENT).all()) and bool((raw["Y"][:, N:] == SENT).all())
    if Yf is not None:
        raw["Yf"] = Yf.cpu()
        full = R.from_frag(raw["Yf"][:rows * N], rows, N)
        got["Y"] = full[:M].contiguous()
        checks["Yf rows >= M are zero"] = bool((full[M:] == 0).all())
        checks["Yf tile behind the last one untouched"] = bool((raw["Yf"][rows * N:] == SENT).all())
    if zacc is not None:
        raw["zero_acc"] = zacc.cpu()
        checks["zero_acc zero over every accumulator, half and row tile"] = bool((raw["zero_acc"][:MT * 2 * 32 * N] == 0).all())
        checks["zero_acc tile behind the last one untouched"] = bool((raw["zero_acc"][MT * 2 * 32 * N:] == SENT).all())
    if acc is not None:
        raw["part_out"] = acc.cpu()
        a0, a1 = R.acc_from_flat(raw["part_out"][:MT * 2 * 32 * N], MT, N)
        got["acc0"], got["acc1"] = a0[:M].contiguous(), a1[:M].contiguous()
        checks["part_out tile behind the last one untouched"] = bool((raw["part_out"][MT * 2 * 32 * N:] == SENT).all())
    if xout is not None:
        raw["xout"] = xout.cpu()
        got["xout"] = R.from_frag(raw["xout"][:rows * K], rows, K)[:M].contiguous()
        checks["xout tile behind the last one untouched"] = bool((raw["xout"][rows * K:] == SENT).all())
    if cv is not None:
        raw["cand_val"], raw["cand_idx"] = cv.cpu(), ci.cpu()
        got["cand_val"], got["cand_idx"] = raw["cand_val"][:M].contiguous(), raw["cand_idx"][:M].contiguous()
        checks["candidate sentinel row untouched"] = bool((raw["cand_val"][M] == SENT).all()) and bool((raw["cand_idx"][M] == SENT_I).all())
    return got, ran.value, raw, checks


def _run_fused(lib, form, M, w16, N):
    c = R.fused_case(form, M, w16, N)
    pk = _pack(lib, form, c["N"], w16)
    got, ran, raw, checks = _launch_fused(lib, c, pk)
    r64, r32 = R.fused_eval(c, F64), R.fused_eval(c, F32)
    res = R.judge_fused(got, c, r64, r32)
    if w16 and c["lnf"] and (c["N"] <= 8192 or M == 33):
        print(f"SKINNY family=fused case={c['name']} dist_true={float((got['Y'].double() - R.true_ln_linear(c)).abs().max()):.3e} "
              f"max_true={float(r64['Y'].abs().max()):.3e}")
    _report("fused", c["name"], KERNEL_NAMES.get(ran, ran), res)
    for what, ok in checks.items():
        assert ok, f"{c['name']}: {what}"
    assert ran == R.expected_kernel(c), f"{c['name']}: kernel {KERNEL_NAMES.get(ran, ran)} ran, expected {KERNEL_NAMES[R.expected_kernel(c)]}"
    _, ran2, raw2, _ = _launch_fused(lib, c, pk)
    assert ran2 == ran
    for k in raw:
        assert R.same_bits(raw[k], raw2[k]), f"{c['name']}: two launches on the same inputs differ in {k}"


FUSED = list(R.fused_cases())
FUSED_ID = [f"{f}-N{N or R.FORMS[f]['N']}-M{M}-w{w}" for f, M, w, N in FUSED]


@pytest.mark.parametrize("form,M,w16,N", [x for x in FUSED if x[2] == 0], ids=[i for x, i in zip(FUSED, FUSED_ID) if x[2] == 0])
def test_fused_plan_fp32(lib, form, M, w16, N):
    """Every form of the fused plan at every MT instance; 16 / 17 rows straddle the row-half dispatch of attn_proj; lm_head: the wave
    kernel (3142 tiles and 514 tiles, one valid column in the last one), the generic kernel from 33 rows on, planted ties."""
    _run_fused(lib, form, M, w16, N)


@pytest.mark.parametrize("form,M,w16,N", [x for x in FUSED if x[2] != 0], ids=[i for x, i in zip(FUSED, FUSED_ID) if x[2] != 0])
def test_fused_plan_16bit_weights(lib, form, M, w16, N):
    """The forms the model runs on 16-bit weights (more than one row tile), against the rounding-point reference; the pack hook's
    16-bit fragments and c1_16 are checked first (_pack)."""
    _run_fused(lib, form, M, w16, N)


# ------------------------------------------------------------------------------------------------ the prefill family
_PREFILL_W = {}


def _launch_prefill(lib, c, W, b):
    M, N, K, ldy = c["M"], c["N"], c["K"], c["ldy"]
    rows = R.tiles_of(M) * 32
    X = torch.full((rows, K), math.nan if c["nan_pad"] else 0.0, dtype=F32)
    X[:M] = c["X"]
    X = X.to(DEV)
    Y = torch.full((M + 1, ldy), SENT, dtype=F32, device=DEV)
    _ok(lib, lib.rgrg_debug_skinny_linear(_p(X), _p(W), _p(b), None, _p(Y), M, N, K, ldy, c["act"], None), c["name"])
    torch.cuda.synchronize()
    return Y.cpu()


@pytest.mark.parametrize("N,K,M,combo", list(R.prefill_cases()), ids=lambda v: str(v))
def test_prefill_gemms(lib, N, K, M, combo):
    """(1024, 1024): KS = 4, 4 chunks per wave, + skinny_reduce_kernel, as fst0 (bias, ReLU) and fst2 (bias) run it; N = 16400 and
    49152: the persistent wide kernel up to 31 rows, <16, MT> from 32 rows on."""
    c = R.prefill_case(N, K, M, combo)
    if (N, K) not in _PREFILL_W:
        _PREFILL_W[(N, K)] = (_dev(c["W"]), _dev(c["bias"]))
    W, b = _PREFILL_W[(N, K)]
    Y = _launch_prefill(lib, c, W, b)
    r64, r32 = R.prefill_eval(c, F64), R.prefill_eval(c, F32)
    kernel = "wide" if (c["KS"] == 1 and (N + 31) // 32 > 512 and M <= 31) else f"pw{K // (8 * c['KS'] * 8)}_mt{R.tiles_of(M)}"
    _report("prefill", c["name"], kernel, {"Y": compare(Y[:M, :N], r64, r32)})
    assert bool((Y[M] == SENT).all()) and bool((Y[:, N:] == SENT).all()), "the sentinel row or the columns N .. ldy - 1 were written"
    assert R.same_bits(Y, _launch_prefill(lib, c, W, b)), "two launches on the same inputs differ"


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(lib):
    """Every rejection of the hooks returns RGRG_EINVAL with a message and launches nothing (the pointers are 64-float dummies)."""
    d = torch.zeros(64, device=DEV)
    di = torch.zeros(64, dtype=torch.int32, device=DEV)
    dl = torch.zeros(64, dtype=torch.int64, device=DEV)
    p, pi_, pl = d.data_ptr(), di.data_ptr(), dl.data_ptr()

    def args(**kw):
        a = _hip.DirectArgs()
        base = dict(Xf=p, P=p, bias=p, Yf=p, K=1024, N=1024, act=0)
        base.update(kw)
        for k, v in base.items():
            setattr(a, k, v)
        return a

    def rejected(a, mode=0, lnf=0, w16=0, M=29):
        rc = lib.rgrg_debug_direct_linear(C.byref(a), mode, lnf, w16, M, None, None)
        return rc == RGRG_EINVAL and bool(lib.rgrg_last_error())

    assert rejected(args(), M=0) and rejected(args(), M=129)
    assert rejected(args(K=512)) and rejected(args(K=2048)) and rejected(args(K=4096, N=2048, part_out=p, Yf=None))
    assert rejected(args(K=4096, c1=p, part_out=p, Yf=None), lnf=1)                      # no LayerNorm fold on the split-K shape
    assert rejected(args(N=1000)) and rejected(args(N=1000, Yf=None, Y=p, ldy=1000, Rf=p)) and rejected(args(N=1000, Yf=None, Y=p, ldy=1000, zero_acc=p))
    assert rejected(args(Yf=None, Y=p, ldy=1023))                                        # ldy < N
    assert rejected(args(part=p), mode=1, lnf=0) and rejected(args(c1=p), mode=5, lnf=1) and rejected(args(), mode=-1) and rejected(args(), lnf=2)
    assert rejected(args(P=None)) and rejected(args(Xf=None)) and rejected(args(Yf=None))
    assert rejected(args(c1=None), lnf=1) and rejected(args(c1=p, bias=None), lnf=1)
    assert rejected(args(c1=p), mode=1, lnf=1)                                           # combine without the accumulators
    assert rejected(args(c1=p, Xf=None, step=pi_, ids=pl, ld_ids=4), mode=2, lnf=1)      # embedding without wte
    assert rejected(args(c1=p, Xf=None, wte=p, step=pi_), mode=2, lnf=1)                 # ... without ids
    assert rejected(args(c1=p, Xf=None, wte=p, step=pi_), mode=3, lnf=1)                 # ... without tokens
    assert rejected(args(c1=p, Xf=None, wte=p, tok_override=pi_), mode=4, lnf=1)         # ... without positions
    assert rejected(args(K=4096, Yf=None)) and rejected(args(K=4096, part_out=p))        # split-K: part_out, and nothing else
    assert rejected(args(cand_val=p)) and rejected(args(act=3)) and rejected(args(xout=p))
    assert rejected(args(), w16=1, M=32) and rejected(args(), w16=3, M=64)
    assert lib.rgrg_debug_direct_linear(None, 0, 0, 0, 29, None, None) == RGRG_EINVAL

    def pack_rejected(W=p, g=None, b=None, N=1024, K=1024, w16=0, packed=p, packed16=None, c1=None, c2=None, c1_16=None):
        rc = lib.rgrg_debug_direct_pack(W, g, b, None, N, K, w16, packed, packed16, c1, c2, c1_16, None)
        return rc == RGRG_EINVAL and bool(lib.rgrg_last_error())

    assert pack_rejected(W=None) and pack_rejected(packed=None) and pack_rejected(N=0) and pack_rejected(K=512)
    assert pack_rejected(g=p) and pack_rejected(g=p, b=p) and pack_rejected(g=p, b=p, c1=p)       # gain without beta; without c1 / c2
    assert pack_rejected(g=p, b=p, c1=p, c2=p, K=4096) and pack_rejected(K=4096, N=2048)
    assert pack_rejected(w16=3, packed16=p) and pack_rejected(w16=1) and pack_rejected(g=p, b=p, c1=p, c2=p, w16=2, packed16=p)

    def skinny_rejected(X=p, W=p, Y=p, M=29, N=1024, K=1024, ldy=1024, act=0):
        rc = lib.rgrg_debug_skinny_linear(X, W, p, None, Y, M, N, K, ldy, act, None)
        return rc == RGRG_EINVAL and bool(lib.rgrg_last_error())

    assert skinny_rejected(M=0) and skinny_rejected(M=129) and skinny_rejected(X=None) and skinny_rejected(W=None) and skinny_rejected(Y=None)
    assert skinny_rejected(K=1000) and skinny_rejected(K=0) and skinny_rejected(K=32) and skinny_rejected(N=0)
    assert skinny_rejected(ldy=1023) and skinny_rejected(act=7)
    torch.cuda.synchronize()
