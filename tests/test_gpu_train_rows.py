"""The row kernels of the teacher-forced training pass ALONE (rgrg_amd/csrc/train_ops.hip, the cross-entropy kernels of
decoder_lm.hip) against the float64 reference of tests/train_rows_reference.py, through the rgrg_debug_* hooks and the four
exported entries of the classifier gradients.  One launch per case, every output element compared; the bounds come from the
reference alone (train_rows_reference: fp32 outputs MARGIN * noise + 2^-23 max|ref|, 16-bit outputs half an ulp at the element's own
magnitude on top of MARGIN * noise, exact operations torch.equal).  Each figure is printed before it is asserted (lines starting
with TRAINROWS); the worst ones observed on the MI355X are kept in profiles/train_rows_parity.md.  Every output buffer carries one
row of sentinel behind the rows the launch covers, which must stay untouched.
"""
import math

import pytest
import torch

import train_rows_reference as R
from attn_reference import compare, from_bits, philox_mask, to_bits
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
RGRG_EINVAL = -1
SENT, SENT16 = -777.25, 0x7B7B
D = R.D


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(t, dtype=None):
    return None if t is None else t.to(device=DEV, dtype=dtype or t.dtype).contiguous()


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.rgrg_last_error())


def _report(kernel, case, res):
    for name, r in res.items():
        print(f"TRAINROWS kernel={kernel} case={case} out={name} err={r['err']:.3e} noise={r['noise']:.3e} bound={r['bound']:.3e} "
              f"used={r['used']:.3f}")
    for name, r in res.items():
        assert r["ok"], f"{kernel} {case} {name}: err {r['err']:.3e} exceeds {r['bound']:.3e} (noise {r['noise']:.3e})"


def _buf(rows, cols, fill, like=None):
    """[rows + 1, cols] fp32 on the device: `like` (or `fill`) in the first rows, the sentinel in the last one."""
    b = torch.full((rows + 1, cols), fill, dtype=F32)
    if like is not None:
        b[:rows] = like
    b[rows] = SENT
    return b.to(DEV)


def _buf16(rows, cols):
    return torch.full((rows + 1, cols), SENT16, dtype=torch.int16, device=DEV)


def _untouched(b, rows):
    return bool((b[rows:] == (SENT16 if b.dtype == torch.int16 else SENT)).all())


# ------------------------------------------------------------------------------------------------ residual + dropout + LayerNorm
@pytest.mark.parametrize("rows", R.ROWS)
def test_resid_dropout_ln16(lib, rows):
    """resid_dropout_ln16_kernel: one wave per row, four rows per workgroup."""
    for c in R.resid_cases(rows):
        fp16 = c["fp16"]
        x = _buf(rows, D, math.nan, c["y"] if c["alias"] else None)
        y = None if c["y16"] else (x if c["alias"] else _dev(c["y"]))
        y16 = _dev(to_bits(c["y"], fp16)) if c["y16"] else None
        resid, g, b = _dev(c["resid"]), _dev(c["g"]), _dev(c["b"])
        xn = _buf16(rows, D)
        _ok(lib, lib.rgrg_debug_resid_dropout_ln16(_p(y), _p(y16), _p(resid), _p(x), _p(g), _p(b), _p(xn), rows, R.SEED, R.SITE, c["p"],
                                                   fp16, None), c["name"])
        torch.cuda.synchronize()
        got = {"x": x[:rows].cpu(), "xn16": from_bits(xn[:rows].cpu(), fp16)}
        _report("resid_dropout_ln16", c["name"], R.judge(got, R.resid_dropout_ln16(c, F64), R.resid_dropout_ln16(c, F32), R.RESID_KINDS, fp16))
        assert _untouched(x, rows) and _untouched(xn, rows), "a row behind the last one was written"
        if c["p"] == 0.0:
            assert torch.equal(got["x"], c["y"] if c["resid"] is None else c["resid"] + c["y"]), "the fp32 store of x at p = 0 is not exact"
    bad = torch.zeros(4, D, device=DEV)
    b16 = torch.zeros(4, D, dtype=torch.int16, device=DEV)
    assert lib.rgrg_debug_resid_dropout_ln16(_p(bad), _p(b16), None, _p(bad), _p(bad), _p(bad), _p(b16), 4, 0, 0, 0.0, 0, None) == RGRG_EINVAL
    assert lib.rgrg_debug_resid_dropout_ln16(None, None, None, _p(bad), _p(bad), _p(bad), _p(b16), 4, 0, 0, 0.0, 0, None) == RGRG_EINVAL
    assert lib.rgrg_debug_resid_dropout_ln16(_p(bad), None, None, _p(bad), _p(bad), _p(bad), _p(b16), 0, 0, 0, 0.0, 0, None) == RGRG_EINVAL


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _run_ln_backward(lib, c, wave_kernel):
    rows, fp16 = c["rows"], c["fp16"]
    dy = None if c["dy16"] else _dev(c["dy"])
    dy16 = _dev(to_bits(c["dy"], fp16)) if c["dy16"] else None
    out = _buf(rows, D, math.nan, c["out_in"] if c["accumulate"] else None)   # accumulate = 0: NaN must not be read
    out16 = _buf16(rows, D) if c["with_out16"] else None
    x, g = _dev(c["x"]), _dev(c["g"])
    _ok(lib, lib.rgrg_debug_ln_backward(_p(dy), _p(dy16), _p(x), _p(g), _p(out), _p(out16), rows, c["accumulate"], R.SEED, R.SITE, c["p"], fp16,
                                        wave_kernel, None), c["name"])
    torch.cuda.synchronize()
    assert _untouched(out, rows) and (out16 is None or _untouched(out16, rows)), "a row behind the last one was written"
    got = {"out": out[:rows].cpu()}
    if out16 is not None:
        got["out16"] = from_bits(out16[:rows].cpu(), fp16)
    return got


@pytest.mark.parametrize("rows", R.ROWS)
def test_ln_backward16(lib, rows):
    """ln_backward16_kernel: one wave per row, with the masked 16-bit copy of the accumulated gradient."""
    for c in R.ln_backward_cases(rows):
        got = _run_ln_backward(lib, c, 1)
        _report("ln_backward16", c["name"], R.judge(got, R.ln_backward(c, F64), R.ln_backward(c, F32), R.ln_backward_kinds(c), c["fp16"]))


@pytest.mark.parametrize("rows", R.ROWS)
def test_ln_backward_f32_and_the_wave_kernel_on_equal_inputs(lib, rows):
    """ln_backward_kernel (one workgroup per row) and, on the same inputs, ln_backward16_kernel: both within the float64 bound."""
    for c in R.ln_backward_cases(rows, 0):
        r64, r32 = R.ln_backward(c, F64), R.ln_backward(c, F32)
        _report("ln_backward", c["name"], R.judge(_run_ln_backward(lib, c, 0), r64, r32, R.ln_backward_kinds(c)))
        _report("ln_backward16", c["name"] + ",as_f32", R.judge(_run_ln_backward(lib, c, 1), r64, r32, R.ln_backward_kinds(c)))
    z = torch.zeros(4, D, device=DEV)
    z16 = torch.zeros(4, D, dtype=torch.int16, device=DEV)
    call = lib.rgrg_debug_ln_backward
    assert call(None, _p(z16), _p(z), _p(z), _p(z), None, 4, 0, 0, 0, 0.0, 0, 0, None) == RGRG_EINVAL      # dy16 with the fp32 kernel
    assert call(_p(z), None, _p(z), _p(z), _p(z), _p(z16), 4, 0, 0, 0, 0.0, 0, 0, None) == RGRG_EINVAL     # out16
    assert call(_p(z), None, _p(z), _p(z), _p(z), None, 4, 0, 0, 0, 0.25, 0, 0, None) == RGRG_EINVAL       # a mask
    assert call(_p(z), _p(z16), _p(z), _p(z), _p(z), None, 4, 0, 0, 0, 0.0, 0, 1, None) == RGRG_EINVAL     # both dy and dy16
    assert call(_p(z), None, _p(z), _p(z), _p(z), None, 0, 0, 0, 0, 0.0, 0, 1, None) == RGRG_EINVAL        # no rows


# ------------------------------------------------------------------------------------------------ cross entropy
def _ce_rows(lib, c, ids=None, am="case"):
    M, rows = c["M"], c["rows"]
    lg, tok = _dev(c["logits"]), _dev(c["ids"] if ids is None else ids)
    amd = _dev((c["am"] if isinstance(am, str) else am).reshape(-1))
    row_loss = torch.full((M + 1,), SENT, device=DEV)
    row_valid = torch.full((M + 1,), 12345, dtype=torch.int32, device=DEV)
    row_lse = torch.full((M + 1,), math.nan, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _ok(lib, lib.rgrg_debug_ce_rows(_p(lg), c["ld"], c["V"], c["row0"], rows, _p(tok), _p(amd), c["T"], M, _p(row_loss), _p(row_valid), _p(row_lse),
                                    _p(err), None), c["name"])
    torch.cuda.synchronize()
    assert float(row_loss[M]) == SENT and int(row_valid[M]) == 12345 and math.isnan(float(row_lse[M])), "entry M was written"
    assert torch.equal(lg.cpu(), c["logits"]), "ce_rows changed the logits"
    return row_loss, row_valid, row_lse, err


def _finalize(lib, row_loss, row_valid, n, id_error=None):
    loss = torch.full((2,), SENT, device=DEV)
    cnt = torch.full((2,), 12345, dtype=torch.int32, device=DEV)
    _ok(lib, lib.rgrg_debug_ce_finalize(_p(row_loss), _p(row_valid), n, _p(loss), _p(cnt), _p(id_error), None), "ce_finalize")
    torch.cuda.synchronize()
    assert float(loss[1]) == SENT and int(cnt[1]) == 12345
    return loss[:1].cpu(), cnt[:1].cpu()


@pytest.mark.parametrize("case", list(R.ce_cases()), ids=lambda c: c["name"])
def test_cross_entropy_rows_and_mean(lib, case):
    """ce_valid_kernel + ce_rows_kernel on a chunk, then ce_finalize_kernel on what they wrote."""
    c = case
    M = c["M"]
    r64, r32 = R.ce_forward(c, F64), R.ce_forward(c, F32)
    row_loss, row_valid, row_lse, err = _ce_rows(lib, c)
    assert int(err) == 0
    lse = row_lse[:M].cpu()
    assert torch.equal(~torch.isnan(lse), r64["lse_written"]), "row_lse was written on a row that is not scored, or left out on one that is"
    got = {"row_loss": row_loss[:M].cpu(), "row_lse": torch.nan_to_num(lse, nan=0.0), "row_valid": row_valid[:M].cpu()}
    _report("ce_rows", c["name"], R.judge(got, r64, r32, R.CE_FORWARD_KINDS))
    assert torch.equal(got["row_loss"][r64["row_valid"] == 0], torch.zeros(int((r64["row_valid"] == 0).sum())))
    loss, cnt = _finalize(lib, row_loss, row_valid, M)
    assert torch.equal(cnt, r64["n_scored"].reshape(1))
    res = compare(loss, r64["loss"].reshape(1), r32["loss"].reshape(1))
    _report("ce_finalize", c["name"], {"loss": res})


def test_cross_entropy_mean_over_many_rows_no_scored_row_and_id_error(lib):
    """ce_finalize_kernel over more rows than its 256 threads; no scored row gives NaN like torch; an invalid id poisons the mean."""
    g = torch.Generator().manual_seed(9)
    for n in (300, 1000):
        valid = (torch.rand(n, generator=g) < 0.4).to(torch.int32)
        rl = (10.0 * torch.rand(n, generator=g)) * valid
        loss, cnt = _finalize(lib, _dev(rl), _dev(valid), n)
        assert int(cnt) == int(valid.sum())
        r64, r32 = (rl.double().sum() / int(valid.sum())).reshape(1), (rl.sum() / int(valid.sum())).reshape(1)
        _report("ce_finalize", f"n={n}", {"loss": compare(loss, r64, r32)})
        one = torch.ones(1, dtype=torch.int32, device=DEV)
        loss, cnt = _finalize(lib, _dev(rl), _dev(valid), n, one)
        assert math.isnan(float(loss)) and int(cnt) == int(valid.sum())
    c = next(k for k in R.ce_cases() if k["V"] == 1003 and k["row0"] == 0)
    row_loss, row_valid, row_lse, err = _ce_rows(lib, c, am=torch.zeros(3, 5))
    assert int(row_valid[:15].sum()) == 0 and bool(torch.isnan(row_lse[:15]).all()) and int(err) == 0
    loss, cnt = _finalize(lib, row_loss, row_valid, 15)
    assert math.isnan(float(loss)) and int(cnt) == 0
    # a label outside [0, V): the error word is raised, the label is clamped for the read (V -> V - 1, -1 -> 0)
    ids = c["ids"].clone()
    ids[2], ids[3] = 1003, -1
    row_loss, row_valid, row_lse, err = _ce_rows(lib, c, ids=ids)
    assert int(err) == 1
    x = c["logits"][:, :1003].double()
    lse = torch.logsumexp(x, dim=-1)
    got = row_loss[:15].cpu().double()
    # row r is scored against ids[r + 1]: row 1 reads column 1002, row 2 column 0 (losses of 160 and about 11: 1e-4 is a few fp32 ulps)
    assert abs(float(got[1] - (lse[1] - x[1, 1002]))) <= 1e-4 and abs(float(got[2] - (lse[2] - x[2, 0]))) <= 1e-4
    loss, _ = _finalize(lib, row_loss, row_valid, 15, err)
    assert math.isnan(float(loss))
    z = torch.zeros(16, device=DEV)
    zi = torch.zeros(16, dtype=torch.int32, device=DEV)
    lg = _dev(c["logits"])
    tok = _dev(c["ids"])
    call = lib.rgrg_debug_ce_rows
    assert call(_p(lg), 1024, 1003, 10, 6, _p(tok), None, 5, 15, _p(z), _p(zi), None, _p(zi), None) == RGRG_EINVAL    # chunk past M
    assert call(_p(lg), 1000, 1003, 0, 15, _p(tok), None, 5, 15, _p(z), _p(zi), None, _p(zi), None) == RGRG_EINVAL   # ld < V
    assert call(_p(lg), 1024, 1003, 0, 15, _p(tok), None, 4, 15, _p(z), _p(zi), None, _p(zi), None) == RGRG_EINVAL   # M % T
    assert lib.rgrg_debug_ce_finalize(_p(z), _p(zi), 15, None, None, None, None) == RGRG_EINVAL


def _run_ce_backward(lib, b, fp16):
    """fp16 None: ce_backward_kernel in place; 0 / 1: ce_backward16_kernel.  Returns d [rows, V] after the buffer checks."""
    rows, V, ld = b["rows"], b["V"], b["ld"]
    lg = _buf(rows, ld, 0.0, b["logits"])
    tok, valid, lse = _dev(b["ids"]), _dev(b["row_valid"]), _dev(b["row_lse"])
    n = torch.tensor([b["n_scored"]], dtype=torch.int32, device=DEV)
    err = torch.tensor([b["id_error"]], dtype=torch.int32, device=DEV)
    out16 = None if fp16 is None else _buf16(rows, ld)
    _ok(lib, lib.rgrg_debug_ce_backward(_p(lg), ld, V, b["row0"], rows, _p(tok), _p(valid), _p(lse), _p(n), b["scale"], _p(err), _p(out16),
                                        fp16 or 0, None), b["name"])
    torch.cuda.synchronize()
    if fp16 is None:
        assert _untouched(lg, rows) and bool((lg[:rows, V:] == 777.0).all()), "the padding columns or the row behind the chunk were written"
        return lg[:rows, :V].cpu()
    assert torch.equal(lg[:rows].cpu(), b["logits"]), "ce_backward16 changed the logits"
    assert _untouched(out16, rows) and bool((out16[:rows, V:] == SENT16).all()), "the padding columns or the row behind the chunk were written"
    return from_bits(out16[:rows, :V].cpu(), fp16)


@pytest.mark.parametrize("fmt", (None, 0, 1), ids=("f32", "bf16", "fp16"))
@pytest.mark.parametrize("case", list(R.ce_cases()), ids=lambda c: c["name"])
def test_cross_entropy_gradient(lib, case, fmt):
    """ce_backward_kernel (in place) and ce_backward16_kernel (16-bit copy; vector body, scalar V % 4 tail)."""
    kinds = {"d": "f32" if fmt is None else "h16"}
    variants = [("scale=3", R.ce_backward_case(case, scale=3.0))]
    if fmt == 1:   # the largest value the fp16 flow can produce: the internal 2^15 with one scored token
        variants.append(("scale=2^15,n=1", R.ce_backward_case(case, scale=32768.0, n_scored=1)))
    for tag, b in variants:
        d = _run_ce_backward(lib, b, fmt)
        assert bool(torch.isfinite(d).all())
        _report("ce_backward" if fmt is None else "ce_backward16", f"{case['name']},{tag},fmt={fmt}", R.judge({"d": d}, R.ce_backward(b, F64), R.ce_backward(b, F32), kinds, fmt))
        ignored = b["row_valid"][b["row0"]:b["row0"] + b["rows"]] == 0
        assert torch.equal(d[ignored], torch.zeros(int(ignored.sum()), b["V"])), "an ignored row is not exactly zero"
    e = R.ce_backward_case(case, scale=3.0, id_error=1)
    d = _run_ce_backward(lib, e, fmt)
    ignored = e["row_valid"][e["row0"]:e["row0"] + e["rows"]] == 0
    assert bool(torch.isnan(d[~ignored]).all()) and torch.equal(d[ignored], torch.zeros(int(ignored.sum()), e["V"])), "id_error: NaN on scored rows, 0 elsewhere"
    if fmt is not None:
        z = torch.zeros(64, device=DEV)
        zi = torch.zeros(64, dtype=torch.int32, device=DEV)
        tok = torch.zeros(64, dtype=torch.int64, device=DEV)
        o = torch.zeros(64, dtype=torch.int16, device=DEV)
        assert lib.rgrg_debug_ce_backward(_p(z), 30, 29, 0, 2, _p(tok), _p(zi), _p(z), _p(zi), 1.0, _p(zi), _p(o), fmt, None) == RGRG_EINVAL   # ld % 4


# ------------------------------------------------------------------------------------------------ element-wise kernels
@pytest.mark.parametrize("case", list(R.gelu_cases()), ids=lambda c: c["name"])
def test_gelu_new_and_its_derivative(lib, case):
    c = case
    pre, out, d = _dev(c["pre"]), torch.full((c["n"] + 4,), SENT, device=DEV), torch.full((c["n"] + 4,), SENT, device=DEV)
    d[:c["n"]] = _dev(c["d"])
    _ok(lib, lib.rgrg_debug_gelu(_p(pre), _p(out), None, c["n"], None), "gelu")
    _ok(lib, lib.rgrg_debug_gelu(_p(pre), None, _p(d), c["n"], None), "gelu backward")
    torch.cuda.synchronize()
    assert bool((out[c["n"]:] == SENT).all()) and bool((d[c["n"]:] == SENT).all()) and torch.equal(pre.cpu(), c["pre"])
    _report("gelu", c["name"], R.judge({"out": out[:c["n"]].cpu(), "d": d[:c["n"]].cpu()}, R.gelu(c, F64), R.gelu(c, F32), R.GELU_KINDS))
    assert lib.rgrg_debug_gelu(_p(pre), _p(out), _p(d), c["n"], None) == RGRG_EINVAL
    assert lib.rgrg_debug_gelu(_p(pre), _p(out), None, c["n"] + 1, None) == RGRG_EINVAL


@pytest.mark.parametrize("n", (1, 1023, 70001))
def test_dropout_add(lib, n):
    g = torch.Generator().manual_seed(n)
    src, resid = torch.randn(n, generator=g) + 0.3, torch.randn(n, generator=g) - 0.6
    for p in (0.0, 0.25):
        mask = philox_mask(R.SEED, R.SITE, p, (n,))
        for with_resid, alias in ((1, 0), (0, 0), (0, 1)):
            out = torch.full((n + 1,), SENT, device=DEV)
            if alias:
                out[:n] = _dev(src)
            s, r = out if alias else _dev(src), _dev(resid) if with_resid else None
            _ok(lib, lib.rgrg_debug_dropout_add(_p(s), _p(r), _p(out), n, R.SEED, R.SITE, p, None), "dropout_add")
            torch.cuda.synchronize()
            assert float(out[n]) == SENT
            got = out[:n].cpu()
            rs = resid if with_resid else None
            if p == 0.0:
                assert torch.equal(got, src + resid if with_resid else src), "dropout_add at p = 0 is not exact"
            _report("dropout_add", f"n={n},p={p},resid={with_resid},alias={alias}",
                    {"out": compare(got, R.dropout_add(src, rs, mask, F64), R.dropout_add(src, rs, mask, F32))})


@pytest.mark.parametrize("shape", ((1, 1, 32), (29, 128, 32), (33, 65, 64), (70, 1024, 96)))
def test_transpose_pad(lib, shape):
    rows, cols, rp = shape
    src = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows))
    dst = torch.full((cols * rp + 8,), math.nan, device=DEV)
    dst[cols * rp:] = SENT
    sd = _dev(src)
    _ok(lib, lib.rgrg_transpose_pad_f32(_p(sd), _p(dst), rows, cols, rp, None), "transpose_pad")
    torch.cuda.synchronize()
    want = torch.zeros(cols, rp)
    want[:, :rows] = src.t()
    assert torch.equal(dst[:cols * rp].cpu().reshape(cols, rp), want) and bool((dst[cols * rp:] == SENT).all())
    assert lib.rgrg_transpose_pad_f32(_p(sd), _p(dst), rows, cols, rows - 1, None) == RGRG_EINVAL


@pytest.mark.parametrize("shape", ((1, 1), (29, 1024), (300, 257)))
def test_colsum(lib, shape):
    rows, cols = shape
    src = torch.randn(rows, cols, generator=torch.Generator().manual_seed(cols)) + 0.5
    out = torch.full((cols + 1,), SENT, device=DEV)
    sd = _dev(src)
    _ok(lib, lib.rgrg_colsum_f32(_p(sd), _p(out), rows, cols, None), "colsum")
    torch.cuda.synchronize()
    seq = R.colsum_sequential(src)
    assert float(out[cols]) == SENT
    _report("colsum", f"rows={rows},cols={cols}", {"out": compare(out[:cols].cpu(), src.double().sum(dim=0), seq)})
    assert torch.equal(out[:cols].cpu(), seq), "colsum is not the row-by-row fp32 sum it documents"


@pytest.mark.parametrize("n", (9, 70001))
def test_relu_backward(lib, n):
    g = torch.Generator().manual_seed(n)
    h = torch.relu(torch.randn(n, generator=g))
    h[:9] = torch.tensor([-0.0, 0.0, math.nan, 1.4e-45, -1.4e-45, math.inf, -math.inf, 1.0, -1.0])
    d = torch.randn(n, generator=g)
    dd = torch.full((n + 1,), SENT, device=DEV)
    dd[:n] = _dev(d)
    hd = _dev(h)
    _ok(lib, lib.rgrg_relu_backward_f32(_p(dd), _p(hd), n, None), "relu_backward")
    torch.cuda.synchronize()
    assert float(h[3]) > 0.0   # the smallest subnormal survived the host
    assert float(dd[n]) == SENT and torch.equal(dd[:n].cpu(), torch.where(h > 0, d, torch.zeros(())))
    assert torch.equal(hd.cpu().view(torch.int32), h.view(torch.int32))


@pytest.mark.parametrize("w", (1.0, 6.0))
@pytest.mark.parametrize("ld", (1, 32))
@pytest.mark.parametrize("n", (1, 29, 300))
def test_bce_with_logits_masked_backward(lib, n, ld, w):
    g = torch.Generator().manual_seed(10 * n + ld)
    x = 4.0 * torch.randn(n, generator=g)
    x[0] = 90.0
    if n > 2:
        x[1], x[2] = -90.0, 0.0
    mask, tgt = (torch.rand(n, generator=g) < 0.6).to(torch.uint8), (torch.rand(n, generator=g) < 0.4).to(torch.uint8)
    mask[:3] = 1
    if n > 2:
        tgt[0], tgt[1] = 1, 1
    for m in (mask, torch.zeros(n, dtype=torch.uint8)):
        out = torch.full((n + 1, ld), SENT, device=DEV)
        xd, md, td = _dev(x), _dev(m), _dev(tgt)   # held until the launch has run
        _ok(lib, lib.rgrg_bce_with_logits_masked_backward_f32(_p(xd), _p(md), _p(td), w, n, 3.0, _p(out), ld, None), "bce backward")
        torch.cuda.synchronize()
        assert bool((out[n] == SENT).all()) and bool((out[:n, 1:] == SENT).all()), "a column other than 0 or the row behind the last was written"
        got = out[:n, 0].cpu()
        if int(m.sum()) == 0:
            assert torch.equal(got, torch.zeros(n)), "an all-zero mask must give all-zero gradients"
        else:
            _report("bce_backward", f"n={n},ld={ld},w={w}", {"d": compare(got, R.bce_backward(x, m, tgt, w, 3.0, F64), R.bce_backward(x, m, tgt, w, 3.0, F32))})
