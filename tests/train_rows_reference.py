"""Plain torch restatements of the row kernels of the teacher-forced training pass (rgrg_amd/csrc/train_ops.hip and the
cross-entropy kernels of decoder_lm.hip), the inputs the per-kernel tests share and the comparison they assert with.
TEST INFRASTRUCTURE ONLY.  Number formats and the host dropout mask come from attn_reference.

Every function takes ``dt``: torch.float64 for the reference, torch.float32 for the noise measurement.  An evaluation returns a
dict name -> tensor; a 16-bit output is returned UNROUNDED (the judge below rounds where it has to).  ``mut`` applies one named
mutation to the evaluation (tests/test_train_rows_reference.py: every one of them must be rejected with the bounds used on the GPU).

Bounds (none comes from the code under test):
  fp32 output   attn_reference.compare: MARGIN * max|ref32 - ref64| + 2^-23 max|ref|
  16-bit output per element |got_i - ref64_i| <= MARGIN * noise + ulp16(|ref64_i| + MARGIN * noise) / 2, noise = max|ref32 - ref64|:
                one correct rounding of a value within MARGIN * noise of the reference, at the element's own magnitude
  exact output  torch.equal
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from attn_reference import MARGIN, compare, philox_mask, rnd16

Tensor = torch.Tensor
F64, F32 = torch.float64, torch.float32
LN_EPS = 1e-5
D = 1024

MUTATIONS = {
    "ln_backward": ("drop_mean_t", "drop_xhat_term", "omit_gain", "biased_rstd", "ignore_accumulate", "mask_wrong_site", "mask_on_fp32_out"),
    "resid_dropout_ln16": ("resid_dropped", "mask_wrong_site"),
    "ce": ("label_off_by_one", "row0_ignored", "score_last_token", "scale_omitted", "tail_label_lost"),
    "gelu": ("gelu_erf",),
}


# ------------------------------------------------------------------------------------------------ the comparison
def ulp16_of(x: Tensor, fp16) -> Tensor:
    """attn_reference.ulp16 element by element (float64)."""
    x = x.double().abs()
    e = torch.floor(torch.log2(x.clamp(min=1e-300)))
    if fp16:
        e = e.clamp(min=-14.0)
    return torch.where(x > 0, torch.pow(torch.tensor(2.0, dtype=F64), e - (10 if fp16 else 7)), torch.zeros((), dtype=F64))


def compare16(got: Tensor, ref64: Tensor, ref32: Tensor, fp16, margin: float = MARGIN) -> Dict[str, float]:
    """The per-element bound of a 16-bit output.  ref64 / ref32: the UNROUNDED value in both evaluations.  ``used`` = the largest
    err_i / bound_i; NaN / inf anywhere fails."""
    r = ref64.double()
    noise = float((ref32.double() - r).abs().max())
    bnd = margin * noise + ulp16_of(r.abs() + margin * noise, fp16) / 2
    g = got.detach().double().cpu()
    assert g.shape == r.shape, (g.shape, r.shape)
    finite = bool(torch.isfinite(g).all())
    err = (g - r).abs()
    used = err / bnd.clamp(min=1e-300)
    used = torch.where((bnd == 0) & (err == 0), torch.zeros_like(used), used)
    i = int(used.argmax()) if finite else 0
    return {"err": float(err.reshape(-1)[i]) if finite else float("inf"), "noise": noise, "bound": float(bnd.reshape(-1)[i]),
            "used": float(used.max()) if finite else float("inf"), "ok": finite and bool((err <= bnd).all()), "max": float(r.abs().max())}


def as_kernel(ev: Dict[str, Tensor], kinds: Dict[str, str], fp16) -> Dict[str, Tensor]:
    """What a kernel that computed the evaluation ``ev`` would store: fp32, or one rounding to the 16-bit type."""
    return {k: (rnd16(ev[k].float(), fp16) if kind == "h16" else ev[k].float() if ev[k].is_floating_point() else ev[k]) for k, kind in kinds.items()}


def judge(got: Dict[str, Tensor], r64: Dict[str, Tensor], r32: Dict[str, Tensor], kinds: Dict[str, str], fp16=None) -> Dict[str, Dict]:
    """Every output of one case against its bound.  kinds[name]: "f32", "h16" or "exact" (compared with the float64 evaluation as
    the kernel would store it; NaN patterns count as equal to NaN)."""
    res = {}
    for k, kind in kinds.items():
        if kind == "f32":
            res[k] = compare(got[k], r64[k], r32[k])
        elif kind == "h16":
            res[k] = compare16(got[k], r64[k], r32[k], fp16)
        else:
            want = r64[k].float() if r64[k].is_floating_point() else r64[k]
            g = got[k].cpu()
            same = g.shape == want.shape and g.dtype == want.dtype and bool(((g == want) | ((g != g) & (want != want))).all())
            res[k] = {"err": 0.0 if same else float("inf"), "noise": 0.0, "bound": 0.0, "used": 0.0 if same else float("inf"), "ok": same}
    return res


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_stats(x: Tensor, with_eps: bool = True):
    """Two-pass mean / variance like nn.LayerNorm: (xhat, rstd)."""
    c = x - x.mean(dim=-1, keepdim=True)
    var = (c * c).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS if with_eps else var)
    return c * rstd, rstd


def layer_norm(x: Tensor, g: Tensor, b: Tensor, dt) -> Tensor:
    xhat, _ = ln_stats(x.to(dt))
    return xhat * g.to(dt) + b.to(dt)


def ln_input_grad(dy: Tensor, x: Tensor, g: Tensor, dt, mut: Optional[str] = None) -> Tensor:
    """dx = rstd (t - mean t - xhat mean(t xhat)), t = dy * g."""
    xhat, rstd = ln_stats(x.to(dt), with_eps=mut != "biased_rstd")
    t = dy.to(dt) if mut == "omit_gain" else dy.to(dt) * g.to(dt)
    m1 = torch.zeros((), dtype=dt) if mut == "drop_mean_t" else t.mean(dim=-1, keepdim=True)
    m2 = torch.zeros((), dtype=dt) if mut == "drop_xhat_term" else (t * xhat).mean(dim=-1, keepdim=True)
    return rstd * (t - m1 - xhat * m2)


def resid_dropout_ln16(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """x = resid + y * mask (fp32 store), xn16 = LayerNorm(x) * g + b before its rounding.  c["y"] is fp32 or already 16 bit."""
    mask = c["mask_alt"] if mut == "mask_wrong_site" else c["mask"]
    x = c["y"].to(dt) * mask.to(dt)
    if c["resid"] is not None and mut != "resid_dropped":
        x = c["resid"].to(dt) + x
    return {"x": x, "xn16": layer_norm(x, c["g"], c["b"], dt)}


def ln_backward(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """out = (accumulate ? out_in : 0) + dx, out16 = out * mask before its rounding."""
    out = ln_input_grad(c["dy"], c["x"], c["g"], dt, mut)
    if c["accumulate"] and mut != "ignore_accumulate":
        out = c["out_in"].to(dt) + out
    mask = (c["mask_alt"] if mut == "mask_wrong_site" else c["mask"]).to(dt)
    r = {"out": out * mask if mut == "mask_on_fp32_out" else out}
    if c["with_out16"]:
        r["out16"] = out * mask
    return r


def _gain(gen, n=D):
    """Gains drawn away from 1, biases away from 0."""
    return 0.4 + 1.6 * torch.rand(n, generator=gen), 0.5 * torch.randn(n, generator=gen) + 0.3


def _rows(gen, rows, mean, std):
    """Rows whose mean is not zero; the row mean changes sign from row to row."""
    sign = 1.0 - 2.0 * (torch.arange(rows) % 2).float()
    return (mean * sign)[:, None] + std * torch.randn(rows, D, generator=gen)


ROWS = (1, 4, 5, 131)   # one wave per row, four rows per workgroup: a partial group, a full one, one over, many groups
SEED, SITE = 0x5DEECE66D1234567, 7


def resid_cases(rows: int):
    """resid_dropout_ln16_kernel: y fp32 / 16 bit, resid NULL / given, y aliasing x (the embedding call), p, type."""
    for fp16 in (0, 1):
        for p in (0.0, 0.25):
            for y16, with_resid, alias in ((0, 0, 1), (0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0)):
                gen = torch.Generator().manual_seed(1000 * rows + 100 * fp16 + 10 * int(p > 0) + 4 * y16 + 2 * with_resid + alias)
                y = _rows(gen, rows, 0.4, 0.1 if with_resid else 1.0)
                g, b = _gain(gen)
                yield {"name": f"rows={rows},fp16={fp16},p={p},y16={y16},resid={with_resid},alias={alias}", "rows": rows, "fp16": fp16, "p": p,
                       "y16": y16, "alias": alias, "y": rnd16(y, fp16) if y16 else y, "resid": _rows(gen, rows, -0.7, 1.0) if with_resid else None,
                       "g": g, "b": b, "mask": philox_mask(SEED, SITE, p, (rows, D)), "mask_alt": philox_mask(SEED, SITE + 1, p, (rows, D))}


RESID_KINDS = {"x": "f32", "xn16": "h16"}


def ln_backward_cases(rows: int, wave_kernel: int = 1):
    """ln_backward16_kernel (wave_kernel = 1): dy fp32 / 16 bit, accumulate, out16 NULL / given, p, type; fp16 gradients carry the
    flow's 2^15.  wave_kernel = 0: the fp32 kernel's subset (dy fp32, no out16, p = 0).  x has a small row variance (0.01) so that
    the eps under the square root is visible next to it."""
    for fp16 in ((0, 1) if wave_kernel else (0,)):
        for p in ((0.0, 0.25) if wave_kernel else (0.0,)):
            for dy16 in ((0, 1) if wave_kernel else (0,)):
                for accumulate in (0, 1):
                    for with_out16 in ((0, 1) if wave_kernel else (0,)):
                        gen = torch.Generator().manual_seed(7000 * rows + 64 * fp16 + 32 * int(p > 0) + 16 * dy16 + 8 * accumulate + 4 * with_out16)
                        s = 1e-4 * 32768.0 if fp16 else 1.0
                        dy = _rows(gen, rows, 0.3, 1.0) * s
                        g, _ = _gain(gen)
                        yield {"name": f"rows={rows},fp16={fp16},p={p},dy16={dy16},acc={accumulate},out16={with_out16}", "rows": rows,
                               "fp16": fp16, "p": p, "dy16": dy16, "accumulate": accumulate, "with_out16": with_out16,
                               "dy": rnd16(dy, fp16) if dy16 else dy, "x": _rows(gen, rows, 0.25, 0.1), "g": g,
                               "out_in": _rows(gen, rows, 0.2, 5.0) * s, "mask": philox_mask(SEED, SITE, p, (rows, D)),
                               "mask_alt": philox_mask(SEED, SITE + 1, p, (rows, D))}


def ln_backward_kinds(c):
    return {"out": "f32", "out16": "h16"} if c["with_out16"] else {"out": "f32"}


# ------------------------------------------------------------------------------------------------ cross entropy
def ce_ignore(am: Optional[Tensor], T: int, M: int, mut: Optional[str] = None) -> Tensor:
    """Row r = (s, t) is ignored when t == T - 1 or attention_mask[r + 1] == 0."""
    r = torch.arange(M)
    last = (r % T) == T - 1
    nxt = torch.zeros(M, dtype=torch.bool) if am is None else torch.cat((am.reshape(-1)[1:] == 0, torch.ones(1, dtype=torch.bool)))
    if mut == "score_last_token":   # the last token of a sentence scored against the first token of the next one
        return nxt
    return last | nxt


def ce_forward(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """ce_valid over all M rows, ce_rows over the chunk [row0, row0 + rows): row_loss / row_valid [M] (0 outside the chunk and on
    ignored rows), row_lse [M] (0 where lse_written is False: the kernel leaves those entries alone), the mean loss over the M rows' entries and the count."""
    M, T, V, row0, rows = c["M"], c["T"], c["V"], c["row0"], c["rows"]
    ign = ce_ignore(c["am"], T, M, mut)
    x = c["logits"][:, :V].to(dt)                      # the chunk's rows
    lse_c = torch.logsumexp(x, dim=-1)
    ids = torch.cat((c["ids"], c["ids"][-1:]))
    row_loss, row_lse, written = torch.zeros(M, dtype=dt), torch.zeros(M, dtype=dt), torch.zeros(M, dtype=torch.bool)
    for i in range(rows):
        r = row0 + i
        if ign[r]:
            continue
        label = int(ids[r] if mut == "label_off_by_one" else ids[(i if mut == "row0_ignored" else r) + 1])
        row_loss[r] = lse_c[i] - x[i, label]
        row_lse[r] = lse_c[i]
        written[r] = True
    valid = (~ign).to(torch.int32)
    n = int(valid.sum())
    return {"row_loss": row_loss, "row_lse": row_lse, "row_valid": valid, "lse_written": written, "loss": row_loss.sum() / n if n else torch.tensor(math.nan, dtype=dt),
            "n_scored": torch.tensor(n, dtype=torch.int32)}


CE_FORWARD_KINDS = {"row_loss": "f32", "row_lse": "f32", "row_valid": "exact"}


def ce_backward(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """d logits = (softmax - onehot) * scale / n_scored on the chunk, from the forward's row_valid / row_lse / n_scored (inputs, as
    for the kernel); ignored rows 0; every scored row NaN when id_error.  The padding columns [V, ld) keep c["logits"]'s."""
    V, row0, rows = c["V"], c["row0"], c["rows"]
    x = c["logits"][:, :V].to(dt)
    ids = torch.cat((c["ids"], c["ids"][-1:]))
    f = torch.tensor(math.nan if c["id_error"] else (1.0 if mut == "scale_omitted" else c["scale"]), dtype=dt) / c["n_scored"]
    out = torch.zeros(rows, V, dtype=dt)
    for i in range(rows):
        r = row0 + i
        if not c["row_valid"][r]:
            continue
        j = i if mut == "row0_ignored" else r
        label = int(ids[r] if mut == "label_off_by_one" else ids[j + 1])
        d = torch.exp(x[i] - c["row_lse"][j].to(dt))
        if not (mut == "tail_label_lost" and label >= (V & ~3)):
            d[label] = d[label] - 1.0
        out[i] = d * f
    return {"d": out}


def ce_cases():
    """V = 50257 (ld 50432) and V = 1003 (ld 1024, V % 4 == 3); T = 5, three sequences, the middle one padded after 3 tokens; chunks
    (0, 15) and (6, 7).  Labels at 0, (V & ~3) - 1, V & ~3 and V - 1; row 1: +80 at the label, -80 elsewhere; row 12: equal logits."""
    T, M = 5, 15
    for V, ld in ((50257, 50432), (1003, 1024)):
        gen = torch.Generator().manual_seed(V)
        V4 = V & ~3
        ids = torch.randint(0, V, (M,), generator=gen)
        ids[1], ids[2], ids[3], ids[4] = 0, V4 - 1, V4, V - 1
        ids[6], ids[7], ids[11], ids[12], ids[13], ids[14] = V - 2, V - 1, V4, 0, min(V4 + 1, V - 1), V4 - 1
        am = torch.ones(3, T)
        am[1, 3:] = 0.0
        full = 3.0 * torch.randn(M, V, generator=gen)
        full[1] = -80.0
        full[1, V4 - 1] = 80.0
        full[12] = 1.25
        for row0, rows in ((0, 15), (6, 7)):
            lg = torch.full((rows, ld), 777.0)
            lg[:, :V] = full[row0:row0 + rows]
            yield {"name": f"V={V},row0={row0},rows={rows}", "V": V, "ld": ld, "T": T, "M": M, "row0": row0, "rows": rows, "ids": ids,
                   "am": am, "logits": lg, "scale": 1.0, "id_error": 0}


def ce_backward_case(c: dict, scale: float = 1.0, id_error: int = 0, n_scored: Optional[int] = None) -> dict:
    """The inputs of the gradient kernels from the float64 forward of the same case (row_lse rounded to the fp32 the kernel reads)."""
    f = ce_forward(c, F64)
    lse = f["row_lse"].float()
    return dict(c, row_valid=f["row_valid"], row_lse=lse, n_scored=int(f["n_scored"]) if n_scored is None else n_scored, scale=scale,
                id_error=id_error)


# ------------------------------------------------------------------------------------------------ element-wise kernels
K_GELU = math.sqrt(2.0 / math.pi)


def gelu_new(x: Tensor, dt, mut: Optional[str] = None) -> Tensor:
    x = x.to(dt)
    if mut == "gelu_erf":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return 0.5 * x * (1.0 + torch.tanh(K_GELU * (x + 0.044715 * x ** 3)))


def gelu_new_grad(x: Tensor, dt, mut: Optional[str] = None) -> Tensor:
    x = x.to(dt)
    if mut == "gelu_erf":
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    th = torch.tanh(K_GELU * (x + 0.044715 * x ** 3))
    return 0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * K_GELU * (1.0 + 3.0 * 0.044715 * x * x)


def gelu(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    return {"out": gelu_new(c["pre"], dt, mut), "d": c["d"].to(dt) * gelu_new_grad(c["pre"], dt, mut)}


GELU_KINDS = {"out": "f32", "d": "f32"}


def gelu_cases():
    """0, +-1e-30, +-0.5, +-3 and +-10 (tanh saturated: 1 - th^2 is 0 in fp32) on top of a normal draw; 4096 and 8192 + 4 elements."""
    special = torch.tensor([0.0, 1e-30, -1e-30, 0.5, -0.5, 3.0, -3.0, 10.0, -10.0])
    for n in (4096, 8192 + 4):
        gen = torch.Generator().manual_seed(n)
        pre = 2.0 * torch.randn(n, generator=gen)
        pre[torch.arange(len(special)) * 5 + 1] = special
        pre[-len(special):] = special
        yield {"name": f"n={n}", "n": n, "pre": pre, "d": torch.randn(n, generator=gen) + 0.5}


def dropout_add(src: Tensor, resid: Optional[Tensor], mask: Tensor, dt) -> Tensor:
    v = src.to(dt) * mask.to(dt)
    return v if resid is None else resid.to(dt) + v


def bce_backward(logits: Tensor, mask: Tensor, target: Tensor, pos_weight: float, scale: float, dt) -> Tensor:
    """d logits of BCEWithLogitsLoss(pos_weight), mean over the rows with mask != 0, times scale; other rows 0."""
    x, y, m = logits.to(dt), target.to(dt), mask != 0
    n = int(m.sum())
    lw = 1.0 + (pos_weight - 1.0) * y
    g = ((1.0 - y) - lw + lw * torch.sigmoid(x)) * torch.tensor(scale, dtype=dt) / max(n, 1)
    return torch.where(m, g, torch.zeros((), dtype=dt))


def colsum_sequential(src: Tensor) -> Tensor:
    """The order colsum_kernel documents: rows added one by one in fp32."""
    a = torch.zeros(src.shape[1], dtype=F32)
    for r in range(src.shape[0]):
        a = a + src[r]
    return a
