"""The detector's target and loss kernels ALONE (rgrg_amd/csrc/det_train.hip: fastrcnn_loss_kernel, rpn_loss_sampled_kernel,
roi_gather_samples_kernel with box_encode1, roi_add_gt_kernel, the two box_match kernels), bce_logits_masked_kernel
(detector_ops.hip) and the two AdamW kernels (train_ops.hip) against the float64 reference of tests/det_loss_reference.py, through
the exported entry points.  One launch per case, every output compared; the bounds come from the reference alone
(det_loss_reference: tensors MARGIN * noise + 2^-23 max|ref| with non-finite elements matched in kind, scalar means
MARGIN * mean|t32_i - t64_i| + 2^-23 mean max(|t_i|, |operands_i|), copied and integer outputs torch.equal).  Each figure is printed
before it is asserted (lines starting with DETLOSS); the worst ones observed on the MI355X are kept in profiles/det_loss_parity.md.
Every output buffer carries a sentinel behind what the launch covers, which must stay untouched.  tests/test_det_loss_reference.py
shows without a GPU that the same bounds on the same inputs reject every mutation of det_loss_reference.MUTATIONS.
"""
import math

import pytest
import torch

import det_loss_reference as R
from oracle import tv013
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
RGRG_EINVAL = -1
SENT, ISENT = -777.25, 12345


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
        print(f"DETLOSS kernel={kernel} case={case} out={name} err={r['err']:.3e} noise={r['noise']:.3e} bound={r['bound']:.3e} "
              f"used={r['used']:.3f}")
    for name, r in res.items():
        assert r["ok"], f"{kernel} {case} {name}: err {r['err']:.3e} exceeds {r['bound']:.3e} (noise {r['noise']:.3e})"


def _out2():
    return torch.full((4,), SENT, device=DEV)


def _scalars(out, names):
    o = out.cpu()
    assert float(o[2]) == SENT and float(o[3]) == SENT, "the words behind the two losses were written"
    return {names[0]: o[0], names[1]: o[1]}


# ------------------------------------------------------------------------------------------------ fastrcnn_loss
@pytest.mark.parametrize("shape", R.FASTRCNN_SHAPES, ids=str)
def test_fastrcnn_loss(lib, shape):
    """fastrcnn_loss_kernel: 256 threads stride over the rows; NaN in the padding columns and in the row behind the data."""
    for c in R.fastrcnn_cases(*shape):
        N, C, ld = c["N"], c["C"], c["ld"]
        pred, reg, out = _dev(c["pred"]), _dev(c["reg"]), _out2()
        labels = _dev(torch.cat((c["labels"], torch.zeros(1, dtype=torch.int64))))
        _ok(lib, lib.rgrg_fastrcnn_loss_f32(_p(pred), ld, C, _p(labels), _p(reg), N, _p(out), None), c["name"])
        torch.cuda.synchronize()
        got = _scalars(out, ("cls", "box"))
        _report("fastrcnn_loss", c["name"], R.judge(got, R.fastrcnn_terms(c, F64), R.fastrcnn_terms(c, F32), R.FASTRCNN_KINDS))
        if c["kind"] == "background":
            assert float(got["box"]) == 0.0, "all background: the box loss is not exactly 0"


def test_fastrcnn_loss_no_rows_and_bad_arguments(lib):
    pred, out = torch.zeros(4, 150, device=DEV), _out2()
    _ok(lib, lib.rgrg_fastrcnn_loss_f32(_p(pred), 150, 30, None, None, 0, _p(out), None), "N=0")
    torch.cuda.synchronize()
    got = _scalars(out, ("cls", "box"))
    assert math.isnan(float(got["cls"])) and math.isnan(float(got["box"]))
    labels, reg, out = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, 4, device=DEV), _out2()
    assert lib.rgrg_fastrcnn_loss_f32(_p(pred), 149, 30, _p(labels), _p(reg), 4, _p(out), None) == RGRG_EINVAL     # ld < 5 C
    assert lib.rgrg_fastrcnn_loss_f32(_p(pred), 150, 0, _p(labels), _p(reg), 4, _p(out), None) == RGRG_EINVAL      # C <= 0
    assert lib.rgrg_fastrcnn_loss_f32(None, 150, 30, _p(labels), _p(reg), 4, _p(out), None) == RGRG_EINVAL         # no pred
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused call wrote its output"


# ------------------------------------------------------------------------------------------------ RPN compute_loss
def _rpn_call(lib, c, d, out, A=None):
    return lib.rgrg_rpn_loss_sampled_f32(_p(d["head"]), c["ld"], c["A_cell"], _p(d["matched"]), _p(d["gt"]), c["G"], _p(d["anchors"]), _p(d["mask"]),
                                         _p(d["list"]), _p(d["count"]), c["B"], c["A"] if A is None else A, c["batch"], _p(out), None)


@pytest.mark.parametrize("shape", R.RPN_SHAPES, ids=str)
def test_rpn_loss_sampled(lib, shape):
    """rpn_loss_sampled_kernel on hand-made sampler outputs: ordinary and extreme objectness logits, only negatives (the box loss is
    exactly 0), nothing sampled (NaN)."""
    for c in R.rpn_cases(*shape):
        d = {k: _dev(c[k]) for k in ("head", "matched", "gt", "anchors", "mask", "list", "count")}
        out = _out2()
        _ok(lib, _rpn_call(lib, c, d, out), c["name"])
        torch.cuda.synchronize()
        got = _scalars(out, ("obj", "box"))
        _report("rpn_loss_sampled", c["name"], R.judge(got, R.rpn_terms(c, F64), R.rpn_terms(c, F32), R.RPN_KINDS))
        if c["variant"] == "negatives":
            assert float(got["box"]) == 0.0, "only negatives: the box loss is not exactly 0"
        if c["variant"] == "empty":
            assert math.isnan(float(got["obj"])) and math.isnan(float(got["box"]))
        if c["variant"] == "ordinary":   # the cell mapping assumes whole cells per image
            out = _out2()
            assert _rpn_call(lib, c, d, out, A=c["A"] + 1) == RGRG_EINVAL
            torch.cuda.synchronize()
            assert bool((out == SENT).all()), "a refused call wrote its output"


# ------------------------------------------------------------------------------------------------ gather / encode, add_gt
@pytest.mark.parametrize("case", list(R.gather_cases()), ids=lambda c: c["name"])
def test_roi_gather_samples(lib, case):
    """roi_gather_samples_kernel: one workgroup per image, K threads (K = 1030: 1024 threads stride); rows from offsets[B] on keep
    the sentinel."""
    c = case
    B, N, K, G = c["B"], c["N"], c["K"], c["G"]
    total = int(c["count"].sum())
    d = {k: _dev(c[k]) for k in ("boxes", "matched", "gt", "gt_labels", "gt_count", "list", "count")}
    props_s = torch.full((B * K + 1, 4), SENT, device=DEV)
    offsets = torch.full((B + 2,), ISENT, dtype=torch.int32, device=DEV)
    labels = torch.full((total + 8,), ISENT, dtype=torch.int64, device=DEV)
    reg = torch.full((total + 8, 4), SENT, device=DEV)
    w = c["weights"]
    _ok(lib, lib.rgrg_roi_gather_samples_f32(_p(d["boxes"]), _p(d["matched"]), _p(d["gt"]), _p(d["gt_labels"]), _p(d["gt_count"]), G, _p(d["list"]),
                                             _p(d["count"]), B, N, K, w[0], w[1], w[2], w[3], _p(props_s), _p(offsets), _p(labels), _p(reg), None), c["name"])
    torch.cuda.synchronize()
    assert bool((props_s[B * K:] == SENT).all()) and int(offsets[B + 1]) == ISENT, "props_s or offsets were written behind their end"
    assert bool((labels[total:] == ISENT).all()) and bool((reg[total:] == SENT).all()), "rows from offsets[B] on were written"
    got = {"offsets": offsets[:B + 1].cpu(), "labels": labels[:total].cpu(), "props_s": props_s[:B * K].cpu().reshape(B, K, 4), "reg": reg[:total].cpu()}
    r64 = R.gather_samples(c, F64)
    _report("roi_gather_samples", c["name"], R.judge(got, r64, R.gather_samples(c, F32), R.GATHER_KINDS))
    o = r64["offsets"]
    assert bool((got["labels"][int(o[2]):int(o[3])] == 0).all()) and bool(torch.isinf(got["reg"][int(o[2]):int(o[3]), 2:]).all())   # no ground truth


@pytest.mark.parametrize("case", list(R.add_gt_cases()), ids=lambda c: c["name"])
def test_roi_add_gt(lib, case):
    c = case
    B, P, G = c["B"], c["P"], c["G"]
    d = {k: _dev(c[k]) for k in ("props", "counts", "gt", "gt_count")}
    boxes = torch.full((B * (P + G) + 1, 4), math.nan, device=DEV)
    boxes[B * (P + G)] = SENT
    box_count = torch.full((B + 1,), ISENT, dtype=torch.int32, device=DEV)
    _ok(lib, lib.rgrg_roi_add_gt_f32(_p(d["props"]), _p(d["counts"]), P, _p(d["gt"]), _p(d["gt_count"]), G, B, _p(boxes), _p(box_count), None), c["name"])
    torch.cuda.synchronize()
    assert bool((boxes[B * (P + G)] == SENT).all()) and int(box_count[B]) == ISENT
    got = {"boxes": boxes[:B * (P + G)].cpu().reshape(B, P + G, 4), "box_count": box_count[:B].cpu()}
    _report("roi_add_gt", c["name"], R.judge(got, R.add_gt(c), R.add_gt(c), {"boxes": "exact", "box_count": "exact"}))


# ------------------------------------------------------------------------------------------------ box matching
@pytest.mark.parametrize("G", (1, 7))
@pytest.mark.parametrize("N", (1, 200, 257))
def test_box_match_at_zero_iou_ties_across_workgroups_and_thresholds(lib, N, G):
    """box_match_kernel + box_match_low_quality_kernel bit-exact against tv013.matcher(tv013.box_iou) on the CPU: a gt that overlaps
    no box (the low-quality pass restores on IoU 0), a tie at boxes 255 / 256 and a second one in another image, each at the gt's
    best IoU between the thresholds (only the low-quality pass matches them), an IoU of exactly 0.5, an image without boxes.
    match_premises asserts that the layout really holds each of them."""
    c = R.match_case(N, G)
    B = c["B"]
    prem = R.match_premises(c, tv013.box_iou, tv013.matcher)
    d = {k: _dev(c[k]) for k in ("gt", "gt_count", "boxes", "box_count")}
    for hi, lo, lq in ((0.7, 0.3, True), (0.5, 0.5, False)):
        matched = torch.full((B * N + 1,), ISENT, dtype=torch.int32, device=DEV)
        ws = torch.empty((B, G), dtype=torch.int32, device=DEV)
        _ok(lib, lib.rgrg_box_match_f32(_p(d["gt"]), _p(d["gt_count"]), G, _p(d["boxes"]), N * 4, _p(d["box_count"]), B, N, hi, lo, int(lq),
                                        _p(matched), _p(ws), None), c["name"])
        torch.cuda.synchronize()
        assert int(matched[B * N]) == ISENT
        got = matched[:B * N].cpu().reshape(B, N)
        for b in range(B):
            n = int(c["box_count"][b])
            assert bool((got[b, n:] == R.MATCH_BELOW).all()), (b, hi)
            if n:
                iou = tv013.box_iou(c["gt"][b], c["boxes"][b, :n])
                ref = tv013.matcher(iou, hi, lo, lq)
                same = torch.equal(got[b, :n].to(torch.int64), ref)
                print(f"DETLOSS kernel=box_match case={c['name']},high={hi},lq={int(lq)},image={b} out=matched equal={int(same)} "
                      f"ties={prem['ties']} restored_at_zero_iou={prem['restored_at_zero_iou']}")
                assert same, (b, hi, got[b, :n], ref)
        if lq:
            for b, g, i, j in c["ties"]:
                assert int(got[b, i]) == g and int(got[b, j]) == g, "both boxes of a tie at the gt's best IoU keep their match"
            assert bool((got[c["zero_iou"][0]] >= 0).all()), "a gt with best IoU 0 restores the arg-max of every box"
        else:
            assert int(got[0, 0]) == 0, "an IoU of exactly 0.5 is a match at the threshold 0.5"


# ------------------------------------------------------------------------------------------------ BCE with logits, masked
@pytest.mark.parametrize("n", R.BCE_N)
def test_bce_with_logits_masked(lib, n):
    """bce_logits_masked_kernel: the forward of both region classifiers' losses."""
    for c in R.bce_cases(n):
        x, mask, tgt = _dev(c["logits"]), _dev(c["mask"]), _dev(c["target"])
        loss = torch.full((2,), SENT, device=DEV)
        _ok(lib, lib.rgrg_bce_with_logits_masked_f32(_p(x), _p(mask), _p(tgt), c["pos_weight"], n, _p(loss), None), c["name"])
        torch.cuda.synchronize()
        assert float(loss[1]) == SENT
        got = {"loss": loss[0].cpu()}
        _report("bce_logits_masked", c["name"], R.judge(got, R.bce_terms(c, F64), R.bce_terms(c, F32), R.BCE_KINDS))
        if c["variant"] == "none":
            assert math.isnan(float(got["loss"]))


# ------------------------------------------------------------------------------------------------ AdamW
def _adam_buffers(c):
    """p, g, m, v on the device, one sentinel element behind each."""
    return {k: torch.cat((c[k], torch.full((1,), SENT))).to(DEV) for k in ("p", "g", "m", "v")}


def _adam_check(kernel, c, d):
    n = c["n"]
    torch.cuda.synchronize()
    assert all(float(d[k][n]) == SENT for k in d), "the element behind the tensor was written"
    assert torch.equal(d["g"][:n].cpu(), c["g"]), "the gradient was changed"
    got = {k: d[k][:n].cpu() for k in ("p", "m", "v")}
    _report(kernel, c["name"], R.judge(got, R.adamw(c, F64), R.adamw(c, F32), R.ADAMW_KINDS))
    return got


@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw_step(lib, n):
    """adamw_kernel with given state and an explicit step; 2097152 + 77 elements run the grid-stride loop."""
    for c in R.adamw_cases(n):
        d = _adam_buffers(c)
        _ok(lib, lib.rgrg_adamw_step_f32(_p(d["p"]), _p(d["g"]), _p(d["m"]), _p(d["v"]), n, c["lr"], c["b1"], c["b2"], c["eps"], c["wd"], c["step"],
                                         c["grad_scale"], None), c["name"])
        _adam_check("adamw", c, d)


def test_adamw_multi_step(lib):
    """adamw_multi_kernel: more than 64 records (a second launch), a tensor longer than 1024 x 256 in the second launch, tensors
    behind the item count untouched."""
    for c in R.adamw_multi_cases():
        d = _adam_buffers(c)
        items = torch.tensor([[d[k].data_ptr() + 4 * s for k in ("p", "g", "m", "v")] + [sz] for s, sz in zip(c["starts"], c["sizes"])], dtype=torch.int64)
        _ok(lib, lib.rgrg_adamw_multi_step_f32(items.data_ptr(), c["items"], c["lr"], c["b1"], c["b2"], c["eps"], c["wd"], c["step"], c["grad_scale"],
                                               None), c["name"])
        got = _adam_check("adamw_multi", c, d)
        dead = ~c["live"]
        assert all(torch.equal(got[k][dead], c[k][dead]) for k in got), "a gap or a tensor behind the item count was written"


def test_adamw_bad_arguments(lib):
    c = next(iter(R.adamw_cases(255)))
    d = _adam_buffers(c)
    call = lib.rgrg_adamw_step_f32
    h = (c["lr"], c["b1"], c["b2"], c["eps"], c["wd"])
    assert call(_p(d["p"]), _p(d["g"]), _p(d["m"]), _p(d["v"]), 255, *h, 0, 1.0, None) == RGRG_EINVAL       # step 0
    assert call(_p(d["p"]), _p(d["g"]), _p(d["m"]), _p(d["v"]), 0, *h, 1, 1.0, None) == RGRG_EINVAL         # n 0
    for k in ("p", "g", "m", "v"):
        assert call(*[None if j == k else _p(d[j]) for j in ("p", "g", "m", "v")], 255, *h, 1, 1.0, None) == RGRG_EINVAL
    items = torch.tensor([[d[k].data_ptr() for k in ("p", "g", "m", "v")] + [255]], dtype=torch.int64)
    multi = lib.rgrg_adamw_multi_step_f32
    assert multi(items.data_ptr(), 1, *h, 0, 1.0, None) == RGRG_EINVAL
    assert multi(items.data_ptr(), 0, *h, 1, 1.0, None) == RGRG_EINVAL
    assert multi(None, 1, *h, 1, 1.0, None) == RGRG_EINVAL
    for bad in ([0] + [int(v) for v in items[0, 1:]], [int(v) for v in items[0, :4]] + [0]):
        record = torch.tensor([bad], dtype=torch.int64)
        assert multi(record.data_ptr(), 1, *h, 1, 1.0, None) == RGRG_EINVAL   # a null pointer, no element
    torch.cuda.synchronize()
    assert all(torch.equal(d[k][:255].cpu(), c[k]) for k in d), "a refused call changed the state"
