"""Plain torch restatements of the detector's target / loss kernels (rgrg_amd/csrc/det_train.hip: fastrcnn_loss_kernel,
rpn_loss_sampled_kernel, box_encode1 inside roi_gather_samples_kernel, roi_add_gt_kernel), of bce_logits_masked_kernel
(detector_ops.hip) and of the two AdamW kernels (train_ops.hip), the inputs the CPU and the GPU test share, the bounds they assert
with and a table of named mutations.  TEST INFRASTRUCTURE ONLY.

Every evaluation takes ``dt``: torch.float64 for the reference, torch.float32 for the noise measurement, and ``mut``: one named
mutation applied to the evaluation (tests/test_det_loss_reference.py: each must be rejected with the bounds used on the GPU).  The
formulas keep torchvision 0.13's order of operations (oracle/tv013.py is the independent restatement they are checked against):
smooth-L1 with beta 1/9 summed over the positive rows and divided by the number of ALL sampled rows, mean cross entropy, mean
BCE-with-logits (ATen's form (1 - y) x + lw (log1p(exp(-|x|)) + max(-x, 0))), det_utils.encode_boxes.

An evaluation returns a dict name -> tensor.  A scalar mean ``name`` comes with ``name.terms`` (its per-row terms t_i) and
``name.ops`` (the largest |operand| that row i reads).

Bounds (none comes from the code under test):
  tensor output  attn_reference.compare: MARGIN * max|ref32 - ref64| + 2^-23 max|ref| over the finite reference elements; a
                 non-finite reference element (log(0 / w) = -inf for an image without ground truth) must be matched in kind
  scalar mean    MARGIN * mean_i |t32_i - t64_i| + 2^-23 * mean_i max(|t64_i|, ops_i): |ref32 - ref64| of the scalar itself can vanish
                 by chance, the mean absolute error of its terms cannot; the floor is one rounding at the magnitude the rows work at
  exact output   torch.equal (NaN equals NaN)
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from attn_reference import MARGIN, compare

Tensor = torch.Tensor
F64, F32 = torch.float64, torch.float32
BETA = 1.0 / 9.0
MATCH_BELOW, MATCH_BETWEEN = -1, -2

MUTATIONS = {
    "fastrcnn": ("beta_one", "class0_deltas", "class_minus_one", "divide_by_positives", "label_column_plus_one", "no_max_shift"),
    "rpn": ("weights_10_10_5_5", "beta_one", "divide_by_positives", "gt_of_image0", "cell_without_image_offset",
            "delta_columns_transposed", "negative_scored_as_positive"),
    "gather": ("wx_ww_swapped", "centre_without_half", "log_inverted", "gt_clamped_to_last", "base_offset_ignored"),
    "bce": ("weight_on_negatives", "mean_over_n", "mask_ignored"),
    "adamw": ("coupled_decay", "no_bias_correction2", "eps_inside_sqrt", "grad_scale_omitted", "decay_after_update"),
}

# objectness / classifier logits: where log1p(exp(-|x|)) is log 2, where it leaves fp32 (exp(-20) < 2^-24), where exp(-|x|) turns
# subnormal (88) and zero (104), and where exp(x) without the |.| would overflow
LOGITS_ORDINARY = (0.0, 1e-7, -1e-7)
LOGITS_EXTREME = (0.0, 1e-7, -1e-7, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)
# differences prediction - target: 0, +-beta, inside the quadratic branch, inside the linear one
DELTA_STEPS = (0.0, BETA, -BETA, 0.05, -0.03, 0.5, -2.0, 1e-3)


# ------------------------------------------------------------------------------------------------ the comparison
def mean_bound(t64: Tensor, t32: Tensor, ops: Tensor, margin: float = MARGIN) -> Dict[str, float]:
    n = t64.numel()
    if n == 0:
        return {"noise": 0.0, "floor": 0.0, "bound": 0.0}
    noise = float((t32.double() - t64.double()).abs().mean())
    floor = 2.0 ** -23 * float(torch.maximum(t64.double().abs(), ops.double().abs()).mean())
    return {"noise": noise, "floor": floor, "bound": margin * noise + floor}


def compare_mean(got, r64: Dict[str, Tensor], r32: Dict[str, Tensor], name: str) -> Dict[str, float]:
    """A scalar mean against the bound of its terms.  A NaN reference (no row) is matched by NaN only."""
    b = mean_bound(r64[name + ".terms"], r32[name + ".terms"], r64[name + ".ops"])
    g, r = float(got), float(r64[name])
    if math.isnan(r):
        b.update(err=0.0 if math.isnan(g) else float("inf"), ok=math.isnan(g), used=0.0 if math.isnan(g) else float("inf"))
        return b
    err = abs(g - r) if math.isfinite(g) else float("inf")
    b.update(err=err, ok=err <= b["bound"], used=err / b["bound"] if b["bound"] > 0 else (0.0 if err == 0 else float("inf")))
    return b


def compare_in_kind(got: Tensor, ref64: Tensor, ref32: Tensor) -> Dict[str, float]:
    """compare() over the elements whose reference is finite; the others must be the same infinity, or NaN for NaN."""
    r, g, r32 = ref64.double(), got.detach().double().cpu(), ref32.double()
    assert g.shape == r.shape, (g.shape, r.shape)
    nf = ~torch.isfinite(r)
    same = bool(((g[nf] == r[nf]) | (torch.isnan(g[nf]) & torch.isnan(r[nf]))).all())
    z = torch.zeros((), dtype=F64)
    res = compare(torch.where(nf, z, g), torch.where(nf, z, r), torch.where(nf, z, r32))
    if not same:
        res.update(ok=False, err=float("inf"), used=float("inf"))
    return res


def judge(got: Dict[str, Tensor], r64: Dict[str, Tensor], r32: Dict[str, Tensor], kinds: Dict[str, str]) -> Dict[str, Dict]:
    """Every output of one case against its bound.  kinds[name]: "mean", "f32" or "exact"."""
    res = {}
    for k, kind in kinds.items():
        if kind == "mean":
            res[k] = compare_mean(got[k], r64, r32, k)
        elif kind == "f32":
            res[k] = compare_in_kind(got[k], r64[k], r32[k])
        else:
            want = r64[k].float() if r64[k].is_floating_point() else r64[k]
            g = got[k].cpu()
            same = g.shape == want.shape and g.dtype == want.dtype and bool(((g == want) | ((g != g) & (want != want))).all())
            res[k] = {"err": 0.0 if same else float("inf"), "noise": 0.0, "bound": 0.0, "used": 0.0 if same else float("inf"), "ok": same}
    return res


def as_kernel(ev: Dict[str, Tensor], kinds: Dict[str, str]) -> Dict[str, Tensor]:
    """What a kernel that computed the evaluation ``ev`` would store (fp32)."""
    return {k: ev[k].float() if ev[k].is_floating_point() else ev[k] for k in kinds}


def _c(x: float, dt) -> Tensor:
    """An fp32 value of the C ABI, widened to dt."""
    return torch.tensor(x, dtype=F32).to(dt)


def smooth_l1(d: Tensor, beta: float) -> Tensor:
    a = d.abs()
    return torch.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta)


def _bce(x: Tensor, y: Tensor, lw) -> Tensor:
    # max(-x, 0) written as (|x| - x) / 2: the same value bit for bit, and autograd's derivative at x = 0 is the true -1/2
    return (1.0 - y) * x + lw * (torch.log1p(torch.exp(-x.abs())) + 0.5 * (x.abs() - x))


# ------------------------------------------------------------------------------------------------ encode / gather / add_gt
def encode(ref: Tensor, props: Tensor, weights, dt, mut: Optional[str] = None) -> Tensor:
    """det_utils.encode_boxes: reference boxes [n,4] against proposals [n,4]."""
    wx, wy, ww, wh = (_c(w, dt) for w in weights)
    if mut == "wx_ww_swapped":
        wx, ww = ww, wx
    half = 1.0 if mut == "centre_without_half" else 0.5
    r, p = ref.to(dt), props.to(dt)
    ex_w, ex_h = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    ex_cx, ex_cy = p[:, 0] + half * ex_w, p[:, 1] + half * ex_h
    gt_w, gt_h = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    gt_cx, gt_cy = r[:, 0] + half * gt_w, r[:, 1] + half * gt_h
    if mut == "log_inverted":
        lw, lh = torch.log(ex_w / gt_w), torch.log(ex_h / gt_h)
    else:
        lw, lh = torch.log(gt_w / ex_w), torch.log(gt_h / ex_h)
    return torch.stack((wx * (gt_cx - ex_cx) / ex_w, wy * (gt_cy - ex_cy) / ex_h, ww * lw, wh * lh), dim=1)


def sample_label(m: Tensor, gt_labels_b: Tensor) -> Tensor:
    """assign_targets_to_proposals: the matched box's class, 0 below the threshold, -1 between."""
    lab = gt_labels_b[m.clamp(min=0).long()].clone()
    lab[m == MATCH_BELOW] = 0
    lab[m == MATCH_BETWEEN] = -1
    return lab


def gather_samples(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """The sampled rows of select_training_samples from (boxes [B,N,4], matched [B,N], list [B,K], count [B]): props_s [B,K,4]
    zero padded, offsets [B + 1], and in RoI order labels [total] and regression targets [total,4] (an image without ground truth
    encodes a zero box, like roi_heads.py)."""
    B, K, G = c["B"], c["K"], c["G"]
    total = int(c["count"].sum())
    props_s = torch.zeros(B, K, 4, dtype=F32)
    offsets = torch.zeros(B + 1, dtype=torch.int32)
    labels = torch.zeros(total, dtype=torch.int64)
    reg = torch.zeros(total, 4, dtype=dt)
    base = 0
    for b in range(B):
        ks = int(c["count"][b])
        offsets[b] = base
        at = 0 if mut == "base_offset_ignored" else base
        base += ks
        if ks == 0:
            continue
        slot = c["list"][b, :ks].long()
        p, m = c["boxes"][b, slot], c["matched"][b, slot]
        props_s[b, :ks] = p
        labels[at:at + ks] = sample_label(m, c["gt_labels"][b])
        if int(c["gt_count"][b]) > 0:
            gi = torch.full_like(m, G - 1).long() if mut == "gt_clamped_to_last" else m.clamp(min=0, max=G - 1).long()
            r = c["gt"][b, gi]
        else:
            r = torch.zeros(ks, 4)
        reg[at:at + ks] = encode(r, p, c["weights"], dt, mut)
    offsets[B] = base
    return {"offsets": offsets, "labels": labels, "props_s": props_s, "reg": reg}


GATHER_KINDS = {"offsets": "exact", "labels": "exact", "props_s": "exact", "reg": "f32"}


def _boxes(gen, shape, lo_w, hi_w, span=400.0):
    xy = torch.rand(*shape, 2, generator=gen) * span - 40.0
    wh = lo_w + torch.rand(*shape, 2, generator=gen) * (hi_w - lo_w)
    return torch.cat((xy, xy + wh), dim=-1)


def gather_cases():
    """B = 3, N = 40 boxes per image; counts [K, 0, 3]; image 2 has no ground truth (its matches are all 'below'); K = 1030 takes
    the 1024-thread strided loop.  ``extreme``: every fifth proposal is 1e-3 wide (targets of 1e6), kept out of the ordinary cases
    so that they do not set the bound of the ordinary elements."""
    B, N = 3, 40
    for G in (1, 5):
        for K in (8, 100, 1030):
            for weights in ((10.0, 10.0, 5.0, 5.0), (1.0, 1.0, 1.0, 1.0)):
                for extreme in (0, 1):
                    if extreme and (K != 100 or G != 5):
                        continue
                    gen = torch.Generator().manual_seed(100000 * G + 10 * K + int(weights[0]) + extreme)
                    boxes = _boxes(gen, (B, N), 2.0, 512.0)
                    if extreme:
                        boxes[:, ::5, 2:] = boxes[:, ::5, :2] + 1e-3
                        boxes[:, 1::5, 2:] = boxes[:, 1::5, :2] + 512.0
                    gt = _boxes(gen, (B, G), 8.0, 300.0)
                    gt_count = torch.tensor([G, max(1, G - 2), 0], dtype=torch.int32)
                    count = torch.tensor([K, 0, 3], dtype=torch.int32)
                    lst = torch.sort(torch.randint(0, N, (B, K), generator=gen), dim=1).values.to(torch.int32)
                    matched = torch.stack([torch.randint(-2, max(int(gt_count[b]), 1), (N,), generator=gen) for b in range(B)]).to(torch.int32)
                    matched[0, lst[0, 0].long()] = G - 1
                    matched[0, lst[0, 1].long()] = 0
                    matched[2] = MATCH_BELOW
                    yield {"name": f"G={G},K={K},w={int(weights[0])},extreme={extreme}", "B": B, "N": N, "G": G, "K": K, "weights": weights,
                           "boxes": boxes, "gt": gt, "gt_labels": torch.randint(1, 30, (B, G), generator=gen), "gt_count": gt_count,
                           "list": lst, "count": count, "matched": matched}


def gather_applies(m: str, c: dict) -> bool:
    if m == "wx_ww_swapped":
        return c["weights"][0] != c["weights"][2]
    if m == "gt_clamped_to_last":
        return c["G"] > 1
    return True


def add_gt(c: dict) -> Dict[str, Tensor]:
    """add_gt_proposals with static shapes: slots [0, counts) proposals, [counts, counts + gt_count) ground truth, the rest zero;
    counts clamp to P and gt_count to G."""
    B, P, G = c["B"], c["P"], c["G"]
    boxes = torch.zeros(B, P + G, 4, dtype=F32)
    box_count = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        n, g = min(int(c["counts"][b]), P), min(int(c["gt_count"][b]), G)
        boxes[b, :n] = c["props"][b, :n]
        boxes[b, n:n + g] = c["gt"][b, :g]
        box_count[b] = n + g
    return {"boxes": boxes, "box_count": box_count}


def add_gt_cases():
    for P, G in ((1, 1), (300, 7), (250, 6)):
        gen = torch.Generator().manual_seed(P)
        B = 4
        yield {"name": f"P={P},G={G}", "B": B, "P": P, "G": G, "props": _boxes(gen, (B, P), 2.0, 300.0), "gt": _boxes(gen, (B, G), 8.0, 300.0),
               "counts": torch.tensor([P + 3, P // 2, 0, P], dtype=torch.int32), "gt_count": torch.tensor([G + 2, G, 0, 1], dtype=torch.int32)}


# ------------------------------------------------------------------------------------------------ roi_heads.fastrcnn_loss
def fastrcnn_terms(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """pred [N, ld] = C class logits | C x 4 deltas | padding; labels [N] in [0, C); reg [N,4]."""
    N, C = c["N"], c["C"]
    full = c["pred"][:N].to(dt)
    x, lab = full[:, :C], c["labels"][:N].long()
    rows = torch.arange(N)
    if mut == "no_max_shift":
        lse = torch.log(torch.exp(x).sum(dim=-1))
    else:
        mx = x.max(dim=-1).values
        lse = mx + torch.log(torch.exp(x - mx[:, None]).sum(dim=-1))
    ce = lse - full[rows, lab + 1 if mut == "label_column_plus_one" else lab]
    pos = lab > 0
    cls_of = torch.zeros_like(lab) if mut == "class0_deltas" else (lab - 1 if mut == "class_minus_one" else lab)
    cols = C + 4 * cls_of[:, None] + torch.arange(4)[None, :]
    own = full.gather(1, cols.clamp(min=0))
    t = c["reg"][:N].to(dt)
    box = torch.where(pos, smooth_l1(own - t, 1.0 if mut == "beta_one" else BETA).sum(dim=-1), torch.zeros((), dtype=dt))
    n_pos = int(pos.sum())
    div = n_pos if mut == "divide_by_positives" else N
    nan = torch.tensor(math.nan, dtype=dt)
    box_ops = torch.where(pos, torch.maximum(own.abs().max(dim=-1).values, t.abs().max(dim=-1).values), torch.zeros((), dtype=dt)) if N else box
    return {"cls": ce.sum() / N if N else nan, "cls.terms": ce, "cls.ops": x.abs().max(dim=-1).values if N else ce,
            "box": box.sum() / div if div else nan, "box.terms": box, "box.ops": box_ops}


FASTRCNN_KINDS = {"cls": "mean", "box": "mean"}
FASTRCNN_SHAPES = ((1, 30, 150), (255, 30, 152), (257, 30, 150), (1000, 30, 160), (300, 2, 10), (64, 5, 29))


def fastrcnn_cases(N: int, C: int, ld: int):
    """Labels mixed / all background / all positive (class C - 1 included).  Rows: ordinary logits; every eighth row all equal
    (the term is log C); big = 1 adds rows with +1e4 on one logit and -1e4 on the others, the label on the maximum (row % 8 == 1)
    and off it (row % 8 == 2).  The positive rows' own deltas are target + DELTA_STEPS.  Columns >= 5 C and row N hold NaN."""
    for kind in ("mixed", "background", "positive"):
        for big in (0, 1):
            gen = torch.Generator().manual_seed(1000 * N + 10 * C + 2 * ("mixed", "background", "positive").index(kind) + big)
            pred = torch.full((N + 1, ld), math.nan)
            pred[:N, :C] = 3.0 * torch.randn(N, C, generator=gen)
            pred[:N, C:5 * C] = torch.randn(N, 4 * C, generator=gen)
            if kind == "mixed":
                labels = torch.randint(0, C, (N,), generator=gen)
                labels[0] = C - 1
                if N > 2:
                    labels[1], labels[2] = 0, 1
            elif kind == "background":
                labels = torch.zeros(N, dtype=torch.int64)
            else:
                labels = torch.randint(1, C, (N,), generator=gen)
                labels[0] = C - 1
            reg = torch.full((N + 1, 4), math.nan)
            reg[:N] = 0.5 * torch.randn(N, 4, generator=gen)
            for i in range(N):
                lab = int(labels[i])
                if i % 8 == 3:
                    pred[i, :C] = 0.75
                elif big and i % 8 in (1, 2):
                    pred[i, :C] = -1e4
                    pred[i, lab if i % 8 == 1 else (lab + 1) % C] = 1e4
                if lab > 0:
                    for k in range(4):
                        pred[i, C + 4 * lab + k] = reg[i, k] + DELTA_STEPS[(4 * i + k) % len(DELTA_STEPS)]
            yield {"name": f"N={N},C={C},ld={ld},labels={kind},big={big}", "N": N, "C": C, "ld": ld, "kind": kind, "big": big, "pred": pred,
                   "labels": labels, "reg": reg}


def fastrcnn_applies(m: str, c: dict) -> bool:
    n_pos = int((c["labels"] > 0).sum())
    if m == "no_max_shift":
        return bool(c["big"]) and c["N"] > 2
    if m == "label_column_plus_one":
        return True
    if m == "divide_by_positives":
        return 0 < n_pos < c["N"]
    return n_pos > 0


# ------------------------------------------------------------------------------------------------ RPN compute_loss
def rpn_rows(c: dict):
    """(image, anchor) of every sampled row, image-major in list order."""
    b = torch.cat([torch.full((int(c["count"][i]),), i, dtype=torch.int64) for i in range(c["B"])]) if c["B"] else torch.zeros(0, dtype=torch.int64)
    i = torch.cat([c["list"][k, :int(c["count"][k])].long() for k in range(c["B"])])
    return b, i


def rpn_terms(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """head [B * cells, ld]: column a < A_cell the objectness of anchor a of the cell, columns A_cell + 4 a .. + 3 its deltas; the
    sampler's mask (1 positive, 2 negative) / list / count; matched [B, A]; gt [B, G, 4]; anchors [A, 4] shared by the images."""
    A, A_cell, G = c["A"], c["A_cell"], c["G"]
    head = c["head"].to(dt)
    b, i = rpn_rows(c)
    n = b.numel()
    at = i if mut == "cell_without_image_offset" else b * A + i
    cell, a = at // A_cell, at % A_cell
    sm = c["mask"][b, i]
    pos = sm == 1
    x = head[cell, a]
    z = torch.ones_like(x) if mut == "negative_scored_as_positive" else pos.to(dt)
    bce = _bce(x, z, 1.0)
    m = c["matched"][b, i].long().clamp(min=0, max=G - 1)
    t = encode(c["gt"][torch.zeros_like(b) if mut == "gt_of_image0" else b, m], c["anchors"][i],
               (10.0, 10.0, 5.0, 5.0) if mut == "weights_10_10_5_5" else (1.0, 1.0, 1.0, 1.0), dt)
    k = torch.arange(4)[None, :]
    cols = A_cell + k * A_cell + a[:, None] if mut == "delta_columns_transposed" else A_cell + 4 * a[:, None] + k
    own = head[cell[:, None], cols]
    zero = torch.zeros((), dtype=dt)
    box = torch.where(pos, smooth_l1(own - t, 1.0 if mut == "beta_one" else BETA).sum(dim=-1), zero)
    n_pos = int(pos.sum())
    div = n_pos if mut == "divide_by_positives" else n
    nan = torch.tensor(math.nan, dtype=dt)
    box_ops = torch.where(pos, torch.maximum(own.abs().max(dim=-1).values, t.abs().max(dim=-1).values), zero) if n else box
    return {"obj": bce.sum() / n if n else nan, "obj.terms": bce, "obj.ops": x.abs(),
            "box": box.sum() / div if div else nan, "box.terms": box, "box.ops": box_ops}


RPN_KINDS = {"obj": "mean", "box": "mean"}
RPN_SHAPES = ((1, 4, 15, 75, 1, 8, (8,)), (3, 20, 15, 80, 4, 256, (256, 0, 100)), (2, 40, 3, 16, 2, 64, (64, 33)),
              (4, 20, 15, 75, 3, 256, (1, 256, 37, 256)))


def rpn_cases(B, cells, A_cell, ld, G, batch, counts):
    """Built by hand, no sampler: per image count[b] distinct anchors in ascending order, about half of them positive (variant
    "negatives": none; "empty": all counts 0), matched to gt 0, gt G - 1 and random ones.  In-range garbage everywhere a correct
    kernel does not look: mask bytes of unlisted anchors, list entries behind count[b], head columns behind 5 A_cell, the matches
    of negatives (-1 / -2) and of unlisted anchors.  Anchors reach outside the image (negative coordinates)."""
    A = cells * A_cell
    for variant in ("ordinary", "extreme", "negatives", "empty"):
        gen = torch.Generator().manual_seed(1000 * B + 10 * cells + ("ordinary", "extreme", "negatives", "empty").index(variant))
        count = torch.zeros(B, dtype=torch.int32) if variant == "empty" else torch.tensor(counts, dtype=torch.int32)
        head = torch.full((B * cells + 1, ld), math.nan)
        head[:B * cells] = 55.5 + torch.randn(B * cells, ld, generator=gen)
        head[:B * cells, :A_cell] = 2.0 * torch.randn(B * cells, A_cell, generator=gen)
        head[:B * cells, A_cell:5 * A_cell] = torch.randn(B * cells, 4 * A_cell, generator=gen)
        ctr = torch.rand(A, 2, generator=gen) * 512.0
        half = 16.0 + torch.rand(A, 2, generator=gen) * 240.0
        anchors = torch.cat((ctr - half, ctr + half), dim=1)
        gt = _boxes(gen, (B, G), 16.0, 300.0)
        mask = torch.randint(1, 3, (B, A), generator=gen).to(torch.uint8)
        matched = torch.randint(-2, G, (B, A), generator=gen).to(torch.int32)
        lst = torch.randint(0, A, (B, batch), generator=gen).to(torch.int32)
        specials = LOGITS_EXTREME if variant == "extreme" else LOGITS_ORDINARY
        seen = 0
        for b in range(B):
            ks = int(count[b])
            idx = torch.sort(torch.randperm(A, generator=gen)[:ks]).values
            lst[b, :ks] = idx.to(torch.int32)
            is_pos = (torch.rand(ks, generator=gen) < 0.5) & (variant != "negatives")
            if ks and variant != "negatives":
                is_pos[0] = True
            if ks > 3:
                is_pos[3] = False    # a negative whose logit is not one of the tiny ones
            n_p = 0
            for k in range(ks):
                i = int(idx[k])
                mask[b, i] = 1 if is_pos[k] else 2
                row, a = (b * A + i) // A_cell, (b * A + i) % A_cell
                if seen < (2 if variant == "extreme" else 1) * len(specials):   # the extreme ones twice: on either side where the draw allows
                    head[row, a] = specials[seen % len(specials)]
                seen += 1
                if is_pos[k]:
                    g = (0, G - 1)[n_p] if n_p < 2 else int(torch.randint(0, G, (1,), generator=gen))
                    matched[b, i] = g
                    t = encode(gt[b, g][None], anchors[i][None], (1.0, 1.0, 1.0, 1.0), F64)[0]
                    for q in range(4):
                        head[row, A_cell + 4 * a + q] = float(t[q]) + DELTA_STEPS[(4 * n_p + q) % len(DELTA_STEPS)]
                    n_p += 1
                else:
                    matched[b, i] = MATCH_BELOW if k % 2 else MATCH_BETWEEN
        yield {"name": f"B={B},cells={cells},A_cell={A_cell},ld={ld},G={G},batch={batch},{variant}", "B": B, "cells": cells, "A_cell": A_cell,
               "A": A, "ld": ld, "G": G, "batch": batch, "variant": variant, "head": head, "anchors": anchors, "gt": gt, "mask": mask,
               "matched": matched, "list": lst, "count": count}


def rpn_applies(m: str, c: dict) -> bool:
    b, i = rpn_rows(c)
    pos = c["mask"][b, i] == 1
    n, n_pos = b.numel(), int(pos.sum())
    if m == "negative_scored_as_positive":
        return n_pos < n
    if m == "cell_without_image_offset":
        return bool((b > 0).any())
    if m == "gt_of_image0":
        return bool((b[pos] > 0).any())
    if m == "divide_by_positives":
        return 0 < n_pos < n
    return n_pos > 0


# ------------------------------------------------------------------------------------------------ BCE with logits, masked
def bce_terms(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """nn.BCEWithLogitsLoss(pos_weight) over the rows with mask != 0, mean; a target byte != 0 is 1.  No row: NaN."""
    keep = torch.ones_like(c["mask"], dtype=torch.bool) if mut == "mask_ignored" else c["mask"] != 0
    x, y = c["logits"].to(dt)[keep], (c["target"] != 0).to(dt)[keep]
    w = _c(c["pos_weight"], dt)
    lw = 1.0 + (w - 1.0) * ((1.0 - y) if mut == "weight_on_negatives" else y)
    t = _bce(x, y, lw)
    n = c["n"] if mut == "mean_over_n" else int(keep.sum())
    return {"loss": t.sum() / n if n else torch.tensor(math.nan, dtype=dt), "loss.terms": t, "loss.ops": x.abs()}


BCE_KINDS = {"loss": "mean"}
BCE_N = (1, 29, 255, 257, 1000)


def bce_cases(n: int):
    """Mask and target bytes 0 / 1 / 2 / 255; unmasked logits hold NaN; row 0 is masked in, a positive; "none": no masked row."""
    for w in (0.25, 1.0, 6.0):
        for variant in ("ordinary", "extreme", "none"):
            if variant == "none" and w != 1.0:
                continue
            gen = torch.Generator().manual_seed(10 * n + int(4 * w) + ("ordinary", "extreme", "none").index(variant))
            x = 3.0 * torch.randn(n, generator=gen)
            sp = LOGITS_EXTREME if variant == "extreme" else LOGITS_ORDINARY
            for k in range(min(n - 1, 2 * len(sp))):
                x[1 + k] = sp[k % len(sp)]
            vals = torch.tensor([1, 2, 255], dtype=torch.uint8)
            mask = torch.where(torch.rand(n, generator=gen) < 0.7, vals[torch.randint(0, 3, (n,), generator=gen)], torch.zeros((), dtype=torch.uint8))
            tgt = torch.where(torch.rand(n, generator=gen) < 0.4, vals[torch.randint(0, 3, (n,), generator=gen)], torch.zeros((), dtype=torch.uint8))
            mask[0], tgt[0] = 1, 255
            if n > 2 * len(sp):    # the special logits count, on both sides: target 1 in the first round, 0 in the second
                mask[1:1 + 2 * len(sp)] = 2
                tgt[1:1 + len(sp)], tgt[1 + len(sp):1 + 2 * len(sp)] = 1, 0
            if n > 28:
                mask[27] = 0
            if variant == "none":
                mask[:] = 0
            x[mask == 0] = math.nan
            yield {"name": f"n={n},w={w},{variant}", "n": n, "pos_weight": w, "variant": variant, "logits": x, "mask": mask, "target": tgt}


def bce_applies(m: str, c: dict) -> bool:
    kept = int((c["mask"] != 0).sum())
    if kept == 0:
        return False
    if m == "weight_on_negatives":
        return c["pos_weight"] != 1.0
    return kept < c["n"]


# ------------------------------------------------------------------------------------------------ AdamW
def adamw(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """One torch.optim.AdamW step (decoupled decay, bias correction) on gradients that carry 1 / grad_scale:
    p *= 1 - lr wd; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
    The hyper-parameters are the fp32 values the C ABI carries, widened to dt: the float64 evaluation therefore differs from
    torch.optim.AdamW called with Python doubles (0.9 is not float32(0.9)) by design; tests/test_det_loss_reference.py hands torch
    the widened values.  Elements with live == False (gaps and tensors behind the item count of the multi kernel) keep their state."""
    lr, b1, b2, eps, wd, gs = (_c(c[k], dt) for k in ("lr", "b1", "b2", "eps", "wd", "grad_scale"))
    p0, m0, v0 = c["p"].to(dt), c["m"].to(dt), c["v"].to(dt)
    g = c["g"].to(dt) * (1.0 if mut == "grad_scale_omitted" else gs)
    if mut == "coupled_decay":
        g = g + wd * p0
    p = p0 if mut in ("coupled_decay", "decay_after_update") else p0 * (1.0 - lr * wd)
    m = b1 * m0 + (1.0 - b1) * g
    v = b2 * v0 + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** c["step"]
    bc2_sqrt = torch.ones((), dtype=dt) if mut == "no_bias_correction2" else torch.sqrt(1.0 - b2 ** c["step"])
    den = torch.sqrt(v + eps) / bc2_sqrt if mut == "eps_inside_sqrt" else torch.sqrt(v) / bc2_sqrt + eps
    p = p - (lr / bc1) * (m / den)
    if mut == "decay_after_update":
        p = p * (1.0 - lr * wd)
    live = c.get("live")
    if live is not None:
        p, m, v = torch.where(live, p, p0), torch.where(live, m, m0), torch.where(live, v, v0)
    return {"p": p, "m": m, "v": v}


ADAMW_KINDS = {"p": "f32", "m": "f32", "v": "f32"}
ADAMW_N = (1, 255, 2097152 + 77)      # 8192 x 256 threads cover 2097152 elements: the last one runs the grid-stride loop
ADAMW_HYPER = {"lr": 0.05, "b1": 0.9, "b2": 0.999, "eps": 1e-8}


def _adam_state(gen, n: int, grad_scale: float):
    """p ~ N(0,1), g x grad_scale ~ 0.3 N(0,1) with every seventh one zero, m ~ 0.1 N(0,1), v in (0.0004, 0.04); every 64th element
    works at 1e-5 (g = m = 1e-5, v = 1e-10), where eps and the second bias correction decide the update."""
    p = torch.randn(n, generator=gen)
    g = 0.3 * torch.randn(n, generator=gen)
    g[3::7] = 0.0
    m = 0.1 * torch.randn(n, generator=gen)
    v = (0.02 + 0.18 * torch.rand(n, generator=gen)) ** 2
    p[0::64], g[0::64], m[0::64], v[0::64] = 1.5, 1e-5, 1e-5, 1e-10
    return p, g / grad_scale, m, v


def adamw_variants():
    for step in (1, 2, 1000):
        for grad_scale in (1.0, 0.125):
            for wd in (0.0, 0.05):
                yield step, grad_scale, wd


def adamw_cases(n: int):
    for step, grad_scale, wd in adamw_variants():
        if n > 100000 and (step, grad_scale, wd) not in ((1, 0.125, 0.05), (1000, 1.0, 0.0)):
            continue
        gen = torch.Generator().manual_seed(n % 100003 + 10 * step + int(8 * grad_scale) + int(100 * wd))
        p, g, m, v = _adam_state(gen, n, grad_scale)
        yield dict(ADAMW_HYPER, name=f"n={n},step={step},gs={grad_scale},wd={wd}", n=n, step=step, grad_scale=grad_scale, wd=wd, p=p, g=g, m=m, v=v)


def adamw_multi_cases():
    """65 and 129 tensors of 1 - 300 elements in one flat buffer, one element of gap between them; in the 129-tensor case tensor
    100 (second launch of the 64-record batching) has 262144 + 77 elements: 1024 x 256 threads cover 262144.  ``items``: the number
    of records handed over; the tensors behind it must stay untouched."""
    for count, items, step, grad_scale, wd in ((65, 65, 1, 0.125, 0.05), (65, 64, 2, 1.0, 0.0), (129, 129, 1000, 0.125, 0.05), (129, 128, 1, 1.0, 0.05)):
        gen = torch.Generator().manual_seed(count + items + step)
        sizes = torch.randint(1, 301, (count,), generator=gen).tolist()
        sizes[0], sizes[1] = 1, 300
        if count == 129:
            sizes[100] = 262144 + 77
        starts, at = [], 0
        for s in sizes:
            starts.append(at)
            at += s + 1
        p, g, m, v = _adam_state(gen, at, grad_scale)
        live = torch.zeros(at, dtype=torch.bool)
        for k in range(items):
            live[starts[k]:starts[k] + sizes[k]] = True
        yield dict(ADAMW_HYPER, name=f"tensors={count},items={items},step={step},gs={grad_scale},wd={wd}", n=at, sizes=sizes, starts=starts,
                   items=items, step=step, grad_scale=grad_scale, wd=wd, p=p, g=g, m=m, v=v, live=live)


def adamw_applies(m: str, c: dict) -> bool:
    if m in ("coupled_decay", "decay_after_update"):
        return c["wd"] != 0.0
    if m == "grad_scale_omitted":
        return c["grad_scale"] != 1.0
    return True


# ------------------------------------------------------------------------------------------------ box matching layouts
def match_case(N: int, G: int):
    """Four images of N boxes and G ground-truth boxes for rgrg_box_match_f32 (bit-exact against tv013.matcher).  The random boxes
    are at least 5 x 5 and stay below coordinate 520; the planted boxes are built so that no random box can beat them:
      image 0: gt 0 = [0,0,1,1] and box 0 = [0,0,2,1], an IoU of exactly 0.5 (a random box reaches 1/25 at most); with N = 257
               boxes 255 and 256, in two workgroups, are the same box as box 0: a tie at gt 0's best IoU, between the thresholds
               0.3 and 0.7, which only the low-quality pass turns into a match;
      image 1: box_count N - N // 4; with N >= 200 the last gt is [2000,2000,2100,2100], out of the random boxes' reach, and
               boxes 3 and 130 are [2000,2000,2200,2100]: a second tie at a best IoU of exactly 0.5;
      image 2: the last gt lies at 5000 and overlaps NO box (best IoU 0: the low-quality pass restores the arg-max of every box);
      image 3: box_count 0 with ground truth present."""
    gen = torch.Generator().manual_seed(31 * N + G)
    B = 4
    boxes = _boxes(gen, (B, N), 5.0, 155.0)
    gxy = torch.rand(B, G, 2, generator=gen) * 300.0
    gt = torch.cat((gxy, gxy + 20.0 + torch.rand(B, G, 2, generator=gen) * 180.0), dim=-1)
    gt[0, 0] = torch.tensor([0.0, 0.0, 1.0, 1.0])
    boxes[0, 0] = torch.tensor([0.0, 0.0, 2.0, 1.0])
    ties = []                                                 # (image, gt, box, box)
    if N == 257:
        boxes[0, 255] = boxes[0, 256] = boxes[0, 0]
        ties.append((0, 0, 255, 256))
    if N >= 200:
        gt[1, G - 1] = torch.tensor([2000.0, 2000.0, 2100.0, 2100.0])
        boxes[1, 3] = boxes[1, 130] = torch.tensor([2000.0, 2000.0, 2200.0, 2100.0])
        ties.append((1, G - 1, 3, 130))
    gt[2, G - 1] = torch.tensor([5000.0, 5000.0, 5010.0, 5020.0])
    return {"name": f"N={N},G={G}", "B": B, "N": N, "G": G, "boxes": boxes, "gt": gt, "gt_count": torch.tensor([G, G, G, G], dtype=torch.int32),
            "box_count": torch.tensor([N, N - N // 4, N, 0], dtype=torch.int32), "ties": ties, "zero_iou": (2, G - 1)}


def match_premises(c: dict, iou_fn, matcher_fn, high: float = 0.7, low: float = 0.3) -> Dict[str, int]:
    """Asserts, on the CPU with the oracle's box_iou / matcher, that the layout holds what match_case promises - so that another
    seed or box range cannot quietly empty a scenario - and returns the counts the test prints.
      ties      both boxes equal their gt's best IoU over the image, that IoU lies strictly between ``low`` and ``high`` and no other
                gt gives either box more: without the low-quality pass both are 'between', with it both match the gt
      zero IoU  the gt overlaps no box; the low-quality pass turns at least one unmatched box into a match
      threshold box 0 of image 0 has an IoU of exactly 0.5 with gt 0
      empty     the last image has ground truth and no box"""
    N, G = c["N"], c["G"]
    assert float(iou_fn(c["gt"][0, :1], c["boxes"][0, :1])) == 0.5
    want_ties = (N == 257) + (N >= 200)
    assert len(c["ties"]) == want_ties, (len(c["ties"]), want_ties)
    for b, g, i, j in c["ties"]:
        n = int(c["box_count"][b])
        assert i < n and j < n and (b != 0 or i // 256 != j // 256), "the tie of image 0 spans two workgroups"
        iou = iou_fn(c["gt"][b], c["boxes"][b, :n])
        best = float(iou[g].max())
        assert float(iou[g, i]) == best and float(iou[g, j]) == best and low < best < high, (b, g, best)
        on, off = matcher_fn(iou, high, low, True), matcher_fn(iou, high, low, False)
        for k in (i, j):
            assert int(off[k]) == MATCH_BETWEEN and int(on[k]) == g, (b, k, int(off[k]), int(on[k]))
    b, g = c["zero_iou"]
    n = int(c["box_count"][b])
    iou = iou_fn(c["gt"][b], c["boxes"][b, :n])
    assert n == N and float(iou[g].max()) == 0.0
    on, off = matcher_fn(iou, high, low, True), matcher_fn(iou, high, low, False)
    restored = int(((on >= 0) & (off < 0)).sum())
    assert restored > 0 and bool((on >= 0).all()), "a gt with best IoU 0 restores the arg-max of every box"
    assert int(c["box_count"][c["B"] - 1]) == 0 and int(c["gt_count"][c["B"] - 1]) > 0
    return {"ties": len(c["ties"]), "restored_at_zero_iou": restored}
