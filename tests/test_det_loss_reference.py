"""The reference of tests/det_loss_reference.py and the bounds of tests/test_gpu_det_loss_kernels.py, checked without a GPU:
  * every restatement equals an independent float64 evaluation to 1e-12 relative: oracle/tv013.py (rpn_compute_loss with an
    injected permutation, fastrcnn_loss, box_encode, select_training_samples), torch.nn.functional (cross_entropy, smooth_l1_loss,
    binary_cross_entropy_with_logits) and torch.optim.AdamW on float64 parameters;
  * the autograd gradient of the BCE restatement equals train_rows_reference.bce_backward, the reference of the backward kernel;
  * SENSITIVITY: on every case the GPU test uses, the float32 evaluation passes its bound and every named mutation that applies to
    the case, stored as a kernel would store it and judged with the same bounds, is rejected; every listed mutation applies somewhere.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import det_loss_reference as R
import train_rows_reference as TR
from oracle import tv013

F64, F32 = torch.float64, torch.float32
REL = 1e-12


def _close(a, b, what=""):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    nf = ~torch.isfinite(b)
    assert bool(((a[nf] == b[nf]) | (torch.isnan(a[nf]) & torch.isnan(b[nf]))).all()), what
    a, b = a[~nf], b[~nf]
    if b.numel():
        assert float((a - b).abs().max()) <= REL * max(float(b.abs().max()), 1e-300), (what, float((a - b).abs().max()), float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ reference against torch / tv013
@pytest.mark.parametrize("shape", R.FASTRCNN_SHAPES, ids=str)
def test_fastrcnn_terms_equal_tv013_and_functional(shape):
    for c in R.fastrcnn_cases(*shape):
        N, C = c["N"], c["C"]
        x, d, lab, reg = c["pred"][:N, :C].double(), c["pred"][:N, C:5 * C].double(), c["labels"], c["reg"][:N].double()
        cls, box = tv013.fastrcnn_loss(x, d, [lab], [reg])
        ev = R.fastrcnn_terms(c, F64)
        _close(ev["cls"], cls, c["name"])
        _close(ev["box"], box, c["name"])
        _close(ev["cls.terms"], F.cross_entropy(x, lab, reduction="none"), c["name"])
        pos = lab > 0
        own = d.reshape(N, C, 4)[torch.arange(N), lab]
        per_row = F.smooth_l1_loss(own, reg, beta=1 / 9, reduction="none").sum(dim=-1)
        _close(ev["box.terms"], torch.where(pos, per_row, torch.zeros((), dtype=F64)), c["name"])
        if c["kind"] == "background":
            assert float(ev["box"]) == 0.0
        assert float(ev["cls.terms"][3 if N > 3 else 0]) > 0.0
        if N > 3:
            _close(ev["cls.terms"][3], torch.tensor(math.log(C), dtype=F64), "equal logits")


@pytest.mark.parametrize("shape", R.RPN_SHAPES, ids=str)
def test_rpn_terms_equal_tv013_compute_loss(shape):
    """tv013.rpn_compute_loss samples 256 anchors per image, at most 128 positive: an image whose hand-made sample fits (every
    label >= 0 is then taken, whatever the injected permutation) is compared as drawn; a case with an image that does not fit is
    compared after dropping samples from the count (the restatement is evaluated on the same reduced case)."""
    compared = 0
    for c in R.rpn_cases(*shape):
        if c["variant"] == "empty":
            ev = R.rpn_terms(c, F64)
            assert math.isnan(float(ev["obj"])) and math.isnan(float(ev["box"]))
            continue
        B, A, A_cell, G = c["B"], c["A"], c["A_cell"], c["G"]
        fits = all(int((c["mask"][b, c["list"][b, :int(c["count"][b])].long()] == 1).sum()) <= 128 for b in range(B))
        if not fits:
            c = dict(c, count=torch.clamp(c["count"], max=100))
        head = c["head"][:B * c["cells"]].double()
        obj = head[:, :A_cell].reshape(-1, 1)
        deltas = head[:, A_cell:5 * A_cell].reshape(-1, 4)
        labels, regs = [], []
        for b in range(B):
            lab = torch.full((A,), -1.0, dtype=F64)
            idx = c["list"][b, :int(c["count"][b])].long()
            lab[idx] = (c["mask"][b, idx] == 1).double()
            labels.append(lab)
            regs.append(tv013.box_encode(c["gt"][b].double()[c["matched"][b].long().clamp(min=0, max=G - 1)], c["anchors"].double(), (1.0, 1.0, 1.0, 1.0)))
        g = torch.Generator().manual_seed(5)
        obj_loss, box_loss = tv013.rpn_compute_loss(obj, deltas, labels, regs, perm_fn=lambda n, tag: torch.randperm(n, generator=g))
        ev = R.rpn_terms(c, F64)
        _close(ev["obj"], obj_loss, c["name"])
        _close(ev["box"], box_loss, c["name"])
        if c["variant"] == "negatives":
            assert float(ev["box"]) == 0.0
        compared += 1
    assert compared == 3


def test_encode_add_gt_and_gather_equal_tv013_select_training_samples():
    g = torch.Generator().manual_seed(11)
    B, P, G = 3, 60, 4
    gt = R._boxes(g, (B, G), 20.0, 200.0)
    props = R._boxes(g, (B, P), 5.0, 300.0)
    props[:, :12] = gt.repeat(1, 3, 1) + 3.0 * torch.randn(B, 12, 4, generator=g)      # proposals that match
    gt_labels = torch.randint(1, 30, (B, G), generator=g)
    gt_count = torch.tensor([G, 0, 2], dtype=torch.int32)
    counts = torch.tensor([P, P, 41], dtype=torch.int32)
    c = {"B": B, "P": P, "G": G, "props": props, "gt": gt, "counts": counts, "gt_count": gt_count}
    added = R.add_gt(c)
    proposals = [props[b, :int(counts[b])].double() for b in range(B)]
    targets = [{"boxes": gt[b, :int(gt_count[b])].double(), "labels": gt_labels[b, :int(gt_count[b])]} for b in range(B)]
    ref_props, ref_labels, ref_reg = tv013.select_training_samples(proposals, targets, perm_fn=lambda n, tag: torch.randperm(n, generator=g))
    N = P + G
    matched = torch.full((B, N), R.MATCH_BELOW, dtype=torch.int32)
    lst, cnt = torch.zeros(B, N, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        n, ng = int(added["box_count"][b]), int(gt_count[b])
        assert n == int(counts[b]) + ng and torch.equal(added["boxes"][b, :n].double(), torch.cat((proposals[b], targets[b]["boxes"])))
        assert float(added["boxes"][b, n:].abs().max() if n < N else 0.0) == 0.0
        if ng:
            matched[b, :n] = tv013.matcher(tv013.box_iou(gt[b, :ng], added["boxes"][b, :n]), 0.5, 0.5, False).to(torch.int32)
        lst[b, :n], cnt[b] = torch.arange(n, dtype=torch.int32), n     # at most 128 positives and 512 boxes: every box is sampled
    assert int((matched[0] >= 0).sum()) > G
    case = {"B": B, "N": N, "G": G, "K": N, "weights": (10.0, 10.0, 5.0, 5.0), "boxes": added["boxes"], "gt": gt, "gt_labels": gt_labels,
            "gt_count": gt_count, "list": lst, "count": cnt, "matched": matched}
    ev = R.gather_samples(case, F64)
    assert torch.equal(ev["labels"], torch.cat(ref_labels))
    _close(ev["reg"], torch.cat(ref_reg), "regression targets")
    assert bool(torch.isinf(ev["reg"][int(ev["offsets"][1]):int(ev["offsets"][2]), 2:]).all())    # the image without ground truth
    for b in range(B):
        assert torch.equal(ev["props_s"][b, :int(cnt[b])].double(), ref_props[b]) and int(ev["offsets"][b + 1] - ev["offsets"][b]) == int(cnt[b])
    for w in ((10.0, 10.0, 5.0, 5.0), (1.0, 1.0, 1.0, 1.0)):
        _close(R.encode(gt[0], props[0, :G], w, F64), tv013.box_encode(gt[0].double(), props[0, :G].double(), w), "encode")


@pytest.mark.parametrize("n", R.BCE_N)
def test_bce_terms_equal_functional_and_their_gradient_equals_the_backward_reference(n):
    for c in R.bce_cases(n):
        keep = c["mask"] != 0
        ev = R.bce_terms(c, F64)
        if c["variant"] == "none":
            assert math.isnan(float(ev["loss"]))
            continue
        x = torch.nan_to_num(c["logits"].double(), nan=0.5).requires_grad_(True)
        y = (c["target"] != 0).double()
        loss = F.binary_cross_entropy_with_logits(x[keep], y[keep], pos_weight=torch.tensor(c["pos_weight"], dtype=F64))
        _close(ev["loss"], loss.detach(), c["name"])
        _close(ev["loss.terms"], F.binary_cross_entropy_with_logits(x[keep], y[keep], pos_weight=torch.tensor(c["pos_weight"], dtype=F64),
                                                                    reduction="none").detach(), c["name"])
        x2 = c["logits"].double().requires_grad_(True)
        (R.bce_terms(dict(c, logits=x2), F64)["loss"] * 3.0).backward()
        want = TR.bce_backward(c["logits"], c["mask"], c["target"] != 0, c["pos_weight"], 3.0, F64)
        assert float((x2.grad - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300), c["name"]


@pytest.mark.parametrize("n", (1, 255))
def test_adamw_equals_torch_optim_on_float64_parameters(n):
    """torch.optim.AdamW gets the SAME hyper-parameters, the fp32 values widened to double."""
    for c in R.adamw_cases(n):
        wide = {k: float(torch.tensor(c[k], dtype=F32)) for k in ("lr", "b1", "b2", "eps", "wd", "grad_scale")}
        p = c["p"].double().clone().requires_grad_(True)
        opt = torch.optim.AdamW([p], lr=wide["lr"], betas=(wide["b1"], wide["b2"]), eps=wide["eps"], weight_decay=wide["wd"])
        opt.state[p] = {"step": torch.tensor(float(c["step"] - 1)), "exp_avg": c["m"].double().clone(), "exp_avg_sq": c["v"].double().clone()}
        p.grad = c["g"].double() * wide["grad_scale"]
        opt.step()
        ev = R.adamw(c, F64)
        assert int(opt.state[p]["step"]) == c["step"]
        _close(ev["p"], p.detach(), c["name"])
        _close(ev["m"], opt.state[p]["exp_avg"], c["name"])
        _close(ev["v"], opt.state[p]["exp_avg_sq"], c["name"])


# ------------------------------------------------------------------------------------------------ sensitivity and self-check
def _verdicts(cases, ev, kinds, family, applies):
    """For every case: the float32 evaluation must pass; every mutation that applies to the case must be rejected."""
    for c in cases:
        r64, r32 = ev(c, F64), ev(c, F32)
        own = R.judge(R.as_kernel(r32, kinds), r64, r32, kinds)
        assert all(v["ok"] for v in own.values()), (c["name"], own)
        for m in R.MUTATIONS[family]:
            if not applies(m, c):
                continue
            res = R.judge(R.as_kernel(ev(c, F64, m), kinds), r64, r32, kinds)
            assert not all(v["ok"] for v in res.values()), f"{m} stays inside the bound at {c['name']}: {res}"


@pytest.mark.parametrize("shape", R.FASTRCNN_SHAPES, ids=str)
def test_fastrcnn_mutations_are_rejected(shape):
    _verdicts(R.fastrcnn_cases(*shape), R.fastrcnn_terms, R.FASTRCNN_KINDS, "fastrcnn", R.fastrcnn_applies)


@pytest.mark.parametrize("shape", R.RPN_SHAPES, ids=str)
def test_rpn_mutations_are_rejected(shape):
    _verdicts(R.rpn_cases(*shape), R.rpn_terms, R.RPN_KINDS, "rpn", R.rpn_applies)


def test_encode_and_gather_mutations_are_rejected():
    _verdicts(R.gather_cases(), R.gather_samples, R.GATHER_KINDS, "gather", R.gather_applies)


@pytest.mark.parametrize("n", R.BCE_N)
def test_bce_mutations_are_rejected(n):
    _verdicts(R.bce_cases(n), R.bce_terms, R.BCE_KINDS, "bce", R.bce_applies)


@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw_mutations_are_rejected(n):
    _verdicts(R.adamw_cases(n), R.adamw, R.ADAMW_KINDS, "adamw", R.adamw_applies)


def test_adamw_multi_mutations_are_rejected():
    _verdicts(R.adamw_multi_cases(), R.adamw, R.ADAMW_KINDS, "adamw", R.adamw_applies)


def test_a_non_finite_target_must_be_matched_in_kind():
    c = next(k for k in R.gather_cases() if k["K"] == 8)
    r64, r32 = R.gather_samples(c, F64), R.gather_samples(c, F32)
    assert bool(torch.isinf(r64["reg"]).any())
    got = R.as_kernel(r64, R.GATHER_KINDS)
    for bad in (0.0, math.inf, math.nan):
        g = dict(got, reg=torch.where(torch.isinf(got["reg"]), torch.tensor(bad), got["reg"]))
        assert not R.judge(g, r64, r32, R.GATHER_KINDS)["reg"]["ok"], bad


@pytest.mark.parametrize("G", (1, 7))
@pytest.mark.parametrize("N", (1, 200, 257))
def test_box_match_layouts_hold_the_ties_the_zero_iou_gt_and_the_threshold(N, G):
    """The layouts of the GPU box-matching test: the ties are their gt's best IoU between the thresholds and change their code with
    the low-quality pass, one gt overlaps no box, one IoU is exactly 0.5, one image has no box."""
    c = R.match_case(N, G)
    prem = R.match_premises(c, tv013.box_iou, tv013.matcher)
    assert prem["ties"] == (N == 257) + (N >= 200) and prem["restored_at_zero_iou"] > 0
    # a low-quality pass that keeps only the FIRST box of a tie differs from the oracle on every tie
    for b, g, i, j in c["ties"]:
        iou = tv013.box_iou(c["gt"][b], c["boxes"][b, :int(c["box_count"][b])])
        on, off = tv013.matcher(iou, 0.7, 0.3, True), tv013.matcher(iou, 0.7, 0.3, False)
        first_only = on.clone()
        first_only[j] = off[j]
        assert not torch.equal(first_only, on)


def test_every_listed_mutation_is_exercised():
    """The tests above reject a mutation wherever it applies; here: each one applies to at least one case of the GPU test."""
    families = {
        "fastrcnn": ([c for s in R.FASTRCNN_SHAPES for c in R.fastrcnn_cases(*s)], R.fastrcnn_applies),
        "rpn": ([c for s in R.RPN_SHAPES for c in R.rpn_cases(*s)], R.rpn_applies),
        "gather": (list(R.gather_cases()), R.gather_applies),
        "bce": ([c for n in R.BCE_N for c in R.bce_cases(n)], R.bce_applies),
        "adamw": ([c for n in R.ADAMW_N[:2] for c in R.adamw_cases(n)] + list(R.adamw_multi_cases()), R.adamw_applies),
    }
    assert set(families) == set(R.MUTATIONS)
    for fam, (cases, applies) in families.items():
        for m in R.MUTATIONS[fam]:
            assert sum(bool(applies(m, c)) for c in cases) > 0, (fam, m)
    want = {"fastrcnn": {"beta_one", "class0_deltas", "class_minus_one", "divide_by_positives", "label_column_plus_one", "no_max_shift"},
            "rpn": {"weights_10_10_5_5", "beta_one", "divide_by_positives", "gt_of_image0", "cell_without_image_offset", "delta_columns_transposed",
                    "negative_scored_as_positive"},
            "gather": {"wx_ww_swapped", "centre_without_half", "log_inverted", "gt_clamped_to_last", "base_offset_ignored"},
            "bce": {"weight_on_negatives", "mean_over_n", "mask_ignored"},
            "adamw": {"coupled_decay", "no_bias_correction2", "eps_inside_sqrt", "grad_scale_omitted", "decay_after_update"}}
    assert all(want[f] <= set(R.MUTATIONS[f]) for f in want) and math.isclose(R.MARGIN, 8.0)
