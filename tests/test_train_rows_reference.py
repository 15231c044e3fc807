"""The reference of tests/train_rows_reference.py and the bounds of tests/test_gpu_train_rows.py, checked without a GPU:
  * every closed form equals float64 torch autograd through F.layer_norm, F.cross_entropy(ignore_index=-100) on the shifted
    tensors, F.gelu(approximate="tanh") and F.binary_cross_entropy_with_logits(pos_weight=...) to 1e-12 relative;
  * SENSITIVITY: on the inputs the GPU test uses, every named mutation of the reference, stored as a kernel would store it and
    pushed through the same judge() with the same bounds, is rejected in EVERY case it applies to (the issue asks for one);
  * the unmutated float32 evaluation passes its own bound in every case.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import train_rows_reference as R

F64, F32 = torch.float64, torch.float32
REL = 1e-12


def _close(a, b, what=""):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert float((a - b).abs().max()) <= REL * max(float(b.abs().max()), 1e-300), (what, float((a - b).abs().max()), float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ reference against torch
@pytest.mark.parametrize("rows", (1, 5))
def test_layer_norm_and_its_input_gradient_equal_torch_autograd(rows):
    c = next(iter(R.ln_backward_cases(rows)))
    b = torch.randn(R.D, generator=torch.Generator().manual_seed(1))
    x = c["x"].double().requires_grad_(True)
    y = F.layer_norm(x, (R.D,), c["g"].double(), b.double(), eps=R.LN_EPS)
    _close(R.layer_norm(c["x"], c["g"], b, F64), y.detach(), "forward")
    y.backward(c["dy"].double())
    _close(R.ln_input_grad(c["dy"], c["x"], c["g"], F64), x.grad, "input gradient")


def test_resid_dropout_ln_and_masked_backward_equal_torch_autograd():
    """x = resid + y * mask -> LayerNorm, and the backward kernel's two outputs: d(x) accumulated onto a gradient that is already
    there, and that sum times the mask of the branch it enters next (= the gradient of the branch output y' in x' + y' * mask)."""
    c = [k for k in R.resid_cases(5) if k["p"] > 0 and k["resid"] is not None and not k["y16"]][0]
    y, resid = c["y"].double().requires_grad_(True), c["resid"].double().requires_grad_(True)
    x = resid + y * c["mask"].double()
    xn = F.layer_norm(x, (R.D,), c["g"].double(), c["b"].double(), eps=R.LN_EPS)
    ev = R.resid_dropout_ln16(c, F64)
    _close(ev["x"], x.detach(), "x")
    _close(ev["xn16"], xn.detach(), "xn")
    b = [k for k in R.ln_backward_cases(5) if k["p"] > 0 and k["accumulate"] and k["with_out16"] and not k["dy16"] and not k["fp16"]][0]
    # out_in is the gradient arriving at x over the residual path; x = x_in + branch * mask
    x_in, branch = b["x"].double().requires_grad_(True), torch.zeros(5, R.D, dtype=F64, requires_grad=True)
    xm = x_in + branch * b["mask"].double()
    loss = (F.layer_norm(xm, (R.D,), b["g"].double(), None, eps=R.LN_EPS) * b["dy"].double()).sum() + (xm * b["out_in"].double()).sum()
    loss.backward()
    ev = R.ln_backward(b, F64)
    _close(ev["out"], x_in.grad, "out")
    _close(ev["out16"], branch.grad, "out16")


@pytest.mark.parametrize("case", list(R.ce_cases()), ids=lambda c: c["name"])
def test_shifted_cross_entropy_equals_torch(case):
    c = case
    S, T, V, M = c["M"] // c["T"], c["T"], c["V"], c["M"]
    full = next(k for k in R.ce_cases() if k["V"] == V and k["rows"] == M)
    logits = full["logits"][:, :V].double().reshape(S, T, V).requires_grad_(True)
    labels = c["ids"].reshape(S, T).clone()
    labels[c["am"] == 0] = -100
    scale = 3.0
    loss = F.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)
    (loss * scale).backward()
    fw = R.ce_forward(c, F64)
    ff = R.ce_forward(full, F64)
    _close(ff["loss"], loss.detach(), "mean loss")
    assert int(ff["n_scored"]) == int((labels[:, 1:] != -100).sum())
    per_row = F.cross_entropy(logits.detach()[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100, reduction="none")
    want = torch.zeros(S, T, dtype=F64)
    want[:, :-1] = per_row.reshape(S, T - 1)
    sl = slice(c["row0"], c["row0"] + c["rows"])
    _close(fw["row_loss"][sl], want.reshape(-1)[sl], "row loss")
    assert float(fw["row_loss"].abs().sum() - fw["row_loss"][sl].abs().sum()) == 0.0
    b = R.ce_backward_case(c, scale=scale)
    b["row_lse"] = ff["row_lse"]   # float64 here: the 1e-12 comparison
    _close(R.ce_backward(b, F64)["d"], logits.grad.reshape(M, V)[sl], "d logits")


def test_gelu_new_and_its_derivative_equal_torch():
    c = next(iter(R.gelu_cases()))
    x = c["pre"].double().requires_grad_(True)
    y = F.gelu(x, approximate="tanh")
    y.backward(c["d"].double())
    ev = R.gelu(c, F64)
    _close(ev["out"], y.detach(), "gelu")
    _close(ev["d"], x.grad, "gelu'")


@pytest.mark.parametrize("w", (1.0, 6.0))
def test_bce_gradient_equals_torch(w):
    g = torch.Generator().manual_seed(3)
    x = (4.0 * torch.randn(300, generator=g)).double().requires_grad_(True)
    mask, tgt = torch.rand(300, generator=g) < 0.6, torch.rand(300, generator=g) < 0.4
    loss = F.binary_cross_entropy_with_logits(x[mask], tgt[mask].double(), pos_weight=torch.tensor(w, dtype=F64))
    (loss * 5.0).backward()
    _close(R.bce_backward(x.detach(), mask, tgt, w, 5.0, F64), x.grad, "bce")
    assert float(R.bce_backward(x.detach(), torch.zeros(300, dtype=torch.bool), tgt, w, 5.0, F64).abs().max()) == 0.0


def test_ulp16_of_is_ulp16_per_element():
    from attn_reference import ulp16
    v = torch.tensor([0.0, 1e-9, 6e-5, 6.2e-5, 0.999, 1.0, 1.5, 2.0, 300.0, 65504.0])
    for fp16 in (0, 1):
        assert R.ulp16_of(v, fp16).tolist() == [ulp16(fp16, float(t)) for t in v]


# ------------------------------------------------------------------------------------------------ sensitivity and self-check
def _verdicts(cases, ev, kinds_of, mutations, applies):
    """For every case: the float32 evaluation must pass; every mutation that applies to the case must be rejected."""
    seen = {m: 0 for m in mutations}
    for c in cases:
        kinds = kinds_of(c) if callable(kinds_of) else kinds_of
        r64, r32 = ev(c, F64), ev(c, F32)
        own = R.judge(R.as_kernel(r32, kinds, c.get("fp16")), r64, r32, kinds, c.get("fp16"))
        assert all(v["ok"] for v in own.values()), (c["name"], own)
        for m in mutations:
            if not applies(m, c):
                continue
            res = R.judge(R.as_kernel(ev(c, F64, m), kinds, c.get("fp16")), r64, r32, kinds, c.get("fp16"))
            assert not all(v["ok"] for v in res.values()), f"{m} stays inside the bound at {c['name']}: {res}"
            seen[m] += 1
    assert all(n > 0 for n in seen.values()), seen


def _ln_applies(m, c):
    if m == "ignore_accumulate":
        return bool(c["accumulate"])
    if m == "mask_on_fp32_out":
        return c["p"] > 0
    if m == "mask_wrong_site":
        return c["p"] > 0 and bool(c["with_out16"])
    return True


@pytest.mark.parametrize("rows", R.ROWS)
def test_ln_backward_mutations_are_rejected(rows):
    _verdicts(R.ln_backward_cases(rows), R.ln_backward, R.ln_backward_kinds, R.MUTATIONS["ln_backward"], _ln_applies)
    fp32_only = [m for m in R.MUTATIONS["ln_backward"] if not m.startswith("mask")]
    _verdicts(R.ln_backward_cases(rows, 0), R.ln_backward, R.ln_backward_kinds, fp32_only, _ln_applies)


@pytest.mark.parametrize("rows", R.ROWS)
def test_resid_dropout_ln16_mutations_are_rejected(rows):
    _verdicts(R.resid_cases(rows), R.resid_dropout_ln16, R.RESID_KINDS, R.MUTATIONS["resid_dropout_ln16"],
              lambda m, c: c["resid"] is not None if m == "resid_dropped" else c["p"] > 0)


def test_cross_entropy_mutations_are_rejected():
    cases = list(R.ce_cases())
    fwd = ("label_off_by_one", "row0_ignored", "score_last_token")
    _verdicts(cases, R.ce_forward, R.CE_FORWARD_KINDS, fwd, lambda m, c: c["row0"] > 0 if m == "row0_ignored" else True)
    bwd = ("label_off_by_one", "row0_ignored", "scale_omitted", "tail_label_lost")
    for fp16 in (None, 0, 1):
        _verdicts([dict(R.ce_backward_case(c, scale=3.0), fp16=fp16) for c in cases], R.ce_backward, {"d": "f32" if fp16 is None else "h16"},
                  bwd, lambda m, c: c["row0"] > 0 if m == "row0_ignored" else True)
    big = [dict(R.ce_backward_case(c, scale=32768.0, n_scored=1), fp16=1) for c in cases]
    _verdicts(big, R.ce_backward, {"d": "h16"}, ("scale_omitted",), lambda m, c: True)
    for c in big:   # the largest value the fp16 flow can produce is finite
        d = R.as_kernel(R.ce_backward(c, F64), {"d": "h16"}, 1)["d"]
        assert bool(torch.isfinite(d).all()) and float(d.abs().max()) > 30000.0


def test_gelu_erf_is_rejected():
    _verdicts(R.gelu_cases(), R.gelu, R.GELU_KINDS, R.MUTATIONS["gelu"], lambda m, c: True)


def test_every_listed_mutation_is_exercised():
    assert set(R.MUTATIONS) == {"ln_backward", "resid_dropout_ln16", "ce", "gelu"}
    assert math.isclose(R.MARGIN, 8.0)
