"""Plain torch restatements of the weight-streaming GEMMs of <= 128 token rows: the fused decode plan (rgrg_amd/csrc/skinny_direct.inc:
rgrg_skinny_direct_f32, rgrg_skinny_direct_half_f32, rgrg_lm_head_wave_f32 and the one-time packing kernels) and the prefill GEMMs
(decoder.hip: rgrg_skinny_gemm_f32, rgrg_skinny_gemm_f32_wide, skinny_reduce_kernel, pack_weights_kernel), the inputs the per-kernel
tests share and the comparison they assert with.  TEST INFRASTRUCTURE ONLY.  Number formats, frag_off and the bound come from
attn_reference, gelu_new from train_rows_reference.

Every evaluation takes ``dt``: torch.float64 for the reference, torch.float32 for the noise measurement, and ``mut``: one named
mutation (tests/test_skinny_reference.py: every one of them must be rejected on the inputs the GPU test uses).

What is evaluated:
  plain      act(x W^T + b + R)
  folded     LayerNorm in front of the GEMM.  float64: two-pass LayerNorm, then the linear.  float32 (the noise run) restates the
             kernel's FOLDED formula rstd * (x (g o W)^T - mean c1) + c2 with sums of x and x^2 in the kernel's summation order
             (row_stats says why), the one-pass variance clamped at 0, c1 = sum_k fl32(g W), c2 = sum_k beta W + bias: the bound
             then carries the cancellation the design accepts.
  16-bit weights (w16 = 1 bf16 / 2 fp16): rounded where the kernel rounds - the activations to the type (nearest even) as MFMA
             operands, the weights round16(fl32(g o W)), c1_16 = the sum of the ROUNDED weights, mean and rstd from the UNROUNDED fp32
             rows; float64 arithmetic everywhere else.
  split-K    accumulator p = sum over k in [2048 p, 2048 p + 2048) plus the bias in p = 0.
  residual stream   x = (X + acc01) + acc23, or wte[token] + wte[position]; in fp32, exactly (the kernels' xout is compared bit for
             bit), and that fp32 x is the input of the GEMM in both evaluations.
  candidates per row and 16-column tile the maximum over the tile's valid columns and the lowest column attaining it.

Bound of an fp32 output (none comes from the code under test): attn_reference.compare, MARGIN * max|ref32 - ref64| + 2^-23 max|ref|.
A constant activation row (variance 0: the folded formula multiplies pure rounding noise by 1 / sqrt(eps)) is judged apart from the
other rows, each part with its own noise, so that it does not widen the bound of the rest.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional

import torch

from attn_reference import MARGIN, bound, compare, frag_off, from_bits, rnd16, to_bits  # noqa: F401  (re-exported for the tests)
from train_rows_reference import gelu_new

Tensor = torch.Tensor
F64, F32 = torch.float64, torch.float32
LN_EPS = 1e-5
D = 1024
ACT_NONE, ACT_RELU, ACT_GELU_NEW = 0, 1, 2
DX_PLAIN, DX_COMBINE4, DX_EMBED, DX_EMBED_TOK, DX_EMBED_TOKPOS = 0, 1, 2, 3, 4
RAN_GENERIC, RAN_HALF, RAN_LM_WAVE = 0, 1, 2
WTE_ROWS = 160
VOCAB, VOCAB_SMALL = 50257, 8208 + 1
CONST_ROW, CONST_VALUE = 3, 0.7

MUTATIONS = ("drop_last_chunk_of_wave", "swap_row_halves", "omit_mean_c1", "c1_unrounded_w16", "bias_in_slices_0_and_2", "omit_acc23",
             "position_step_plus_1", "last_max_wins", "pad_columns_in_argmax", "tile1_reads_tile0_residual")


# ------------------------------------------------------------------------------------------------ layouts
def tiles_of(M: int) -> int:
    return (M + 31) // 32


@functools.lru_cache(maxsize=8)
def frag_index(rows: int, L: int) -> Tensor:
    """attn_reference.frag_off for every (row, k) of a [rows][L] matrix (rows % 32 == 0, L % 16 == 0)."""
    assert rows % 32 == 0 and L % 16 == 0
    r, k = torch.arange(rows)[:, None], torch.arange(L)[None, :]
    return ((((r >> 5) * 2 + ((r >> 4) & 1)) * (L >> 4) + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + (r & 15)) * 4 + (k & 3)


def to_frag(X: Tensor, tiles: Optional[int] = None, fill: float = 0.0) -> Tensor:
    """Row-major [M][L] -> the flat fragment-major buffer of `tiles` row tiles (default: the tiles M needs); pad rows = fill."""
    M, L = X.shape
    rows = 32 * (tiles if tiles is not None else tiles_of(M))
    full = torch.full((rows, L), fill, dtype=X.dtype)
    full[:M] = X
    flat = torch.empty(rows * L, dtype=X.dtype)
    flat[frag_index(rows, L).reshape(-1)] = full.reshape(-1)
    return flat


def from_frag(flat: Tensor, rows: int, L: int) -> Tensor:
    """The flat fragment-major buffer of rows / 32 row tiles -> row-major [rows][L]."""
    return flat[frag_index(rows, L)]


def acc_to_flat(A0: Tensor, A1: Tensor, tiles: Optional[int] = None, fill: float = 0.0) -> Tensor:
    """The two accumulators [M][N] of a split-K GEMM -> [tile][2][2 halves][N / 16][64][4]."""
    t = tiles if tiles is not None else tiles_of(A0.shape[0])
    N = A0.shape[1]
    return torch.stack((to_frag(A0, t, fill).reshape(t, 32 * N), to_frag(A1, t, fill).reshape(t, 32 * N)), dim=1).reshape(-1)


def acc_from_flat(flat: Tensor, tiles: int, N: int):
    v = flat.reshape(tiles, 2, 32 * N)
    return tuple(from_frag(v[:, p].reshape(-1), tiles * 32, N) for p in (0, 1))


def pack_direct(W: Tensor) -> Tensor:
    """[N][K] -> [NT][K / 16][64 lanes][4] of the fused plan: lane l holds W[nt * 16 + l % 16][kc * 16 + (l / 16) * 4 .. + 3]."""
    N, K = W.shape
    NT = (N + 15) // 16
    P = torch.zeros(NT * 16, K, dtype=W.dtype)
    P[:N] = W
    return P.reshape(NT, 16, K // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def pack_skinny(W: Tensor) -> Tensor:
    """[N][K] -> [NT][K / 8][64 lanes][4] of the prefill GEMMs: lane l holds W[nt * 32 + l % 32][kc * 8 + (l / 32) * 4 .. + 3]."""
    N, K = W.shape
    NT = (N + 31) // 32
    P = torch.zeros(NT * 32, K, dtype=W.dtype)
    P[:N] = W
    return P.reshape(NT, 32, K // 8, 2, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def pick_ks(N: int, K: int) -> int:
    """K slices of a prefill GEMM (decoder.hip pick_ks): narrow outputs split K over workgroups until ~256 of them stream."""
    NT, chunks, ks = (N + 31) // 32, K // 8, 1
    if NT >= 64:
        return ks
    while NT * ks < 256 and chunks % (ks * 2 * 8 * 4) == 0:
        ks *= 2
    return ks


# ------------------------------------------------------------------------------------------------ the operations
def act_fn(v: Tensor, act: int, dt) -> Tensor:
    if act == ACT_RELU:
        return torch.clamp(v, min=0.0)
    return gelu_new(v, dt) if act == ACT_GELU_NEW else v


def plain_linear(X: Tensor, W: Tensor, b: Optional[Tensor], R: Optional[Tensor], act: int, dt) -> Tensor:
    v = X.to(dt) @ W.to(dt).t()
    if b is not None:
        v = v + b.to(dt)
    if R is not None:
        v = v + R.to(dt)
    return act_fn(v, act, dt)


def fold_vectors(W: Tensor, g: Tensor, beta: Tensor, bias: Optional[Tensor], dt):
    """(c1, c2) = (sum_k fl32(g W), sum_k beta W + bias) summed in dt.  The kernel sums in double and stores fp32."""
    c1 = (W * g).to(dt).sum(dim=1)
    c2 = (W.to(dt) * beta.to(dt)).sum(dim=1)
    return c1, c2 if bias is None else c2 + bias.to(dt)


def row_sums_kernel_order(x: Tensor):
    """sum(x), sum(x^2) of fp32 rows [M][1024] in the order of dx_row_stats / dx_row_mean_rstd (skinny_direct.inc): k = wave * 128 +
    chunk * 16 + q * 4 + j; a lane adds (x0 + x1) + (x2 + x3) of its 8 chunks one after the other, the four lanes q of a row are
    added as (q0 + q1) + (q2 + q3), the 8 waves one after the other."""
    M, K = x.shape
    assert K == 1024 and x.dtype == F32
    v = x.reshape(M, 8, 8, 4, 4)                    # [row][wave][chunk][q][j]
    s1, s2 = torch.zeros(M, 8, 4), torch.zeros(M, 8, 4)
    for ch in range(8):
        a = v[:, :, ch]
        s1 = s1 + ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3]))
        s2 = s2 + ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + (a[..., 2] * a[..., 2] + a[..., 3] * a[..., 3]))
    s1, s2 = (s1[..., 0] + s1[..., 1]) + (s1[..., 2] + s1[..., 3]), (s2[..., 0] + s2[..., 1]) + (s2[..., 2] + s2[..., 3])
    S1, S2 = s1[:, 0], s2[:, 0]
    for w in range(1, 8):
        S1, S2 = S1 + s1[:, w], S2 + s2[:, w]
    return S1[:, None], S2[:, None]


def row_stats(x: Tensor, dt):
    """(mean, rstd) [M, 1] of the rows of the fp32 x: two-pass in float64; in float32 the kernel's sums of x and x^2 IN THE KERNEL'S
    ORDER with the one-pass variance clamped at 0.  The order is restated because the noise run has to carry an accepted property of
    the design: at a row variance near 0 the one-pass variance is a few ulp of E[x^2] instead of 0 (1.5e-7 at a constant 0.7), which
    against eps = 1e-5 moves rstd by ~1 %, while another summation order (torch's own) happens to cancel to exactly 0 there and would
    report no noise at all.  On the 16-bit-weight forms that rstd multiplies (round16(x) - x) c1_16, which does not vanish on a
    constant row."""
    if dt == F64:
        x = x.to(dt)
        mean = x.mean(dim=1, keepdim=True)
        var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    else:
        S1, S2 = row_sums_kernel_order(x)
        mean = S1 / x.shape[1]
        var = torch.clamp(S2 / x.shape[1] - mean * mean, min=0.0)
    return mean, 1.0 / torch.sqrt(var + LN_EPS)


def residual_stream(c: dict, mut: Optional[str] = None) -> Tensor:
    """The fp32 rows [M][K] the GEMM consumes, exactly as the kernel rebuilds them."""
    M, mode = c["M"], c["mode"]
    if mode == DX_PLAIN:
        x = c["X"]
    elif mode == DX_COMBINE4:
        x = c["X"] + c["A0"]
        if mut != "omit_acc23":
            x = x + c["A1"]
    else:
        step = c["step"] + (1 if mut == "position_step_plus_1" else 0)
        tok = c["ids"][:M, c["step"]] if mode == DX_EMBED else c["tok"][:M].long()
        if mode == DX_EMBED_TOKPOS:
            pos = (c["pos"][:M].long() + (1 if mut == "position_step_plus_1" else 0)) % WTE_ROWS
        else:
            pos = torch.full((M,), step, dtype=torch.long)
        x = c["wte"][tok] + c["wte"][pos]
    if mut == "swap_row_halves":
        x = x.clone()
        for t in range(tiles_of(M)):
            lo, hi = x[t * 32:t * 32 + 16].clone(), x[t * 32 + 16:t * 32 + 32].clone()
            n = min(len(lo), len(hi))
            if n:
                x[t * 32:t * 32 + n], x[t * 32 + 16:t * 32 + 16 + n] = hi[:n], lo[:n]
    return x


def fused_eval(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """One GEMM of the fused plan.  Returns x (fp32, the rebuilt rows), and Y [M][N], or acc0 / acc1 [M][N] of a split-K GEMM;
    vpad [M]: what a zero-padded column of the last tile would give (folded forms)."""
    M, N, K, w16 = c["M"], c["N"], c["K"], c["w16"]
    fp16 = w16 == 2
    x = residual_stream(c, mut)
    W, bias = c["W"], c["bias"]
    out = {"x": x}
    kmask = None
    if mut == "drop_last_chunk_of_wave":   # wave 2 of K slice 0 loses its chunk 7: k in [368, 384)
        kmask = torch.ones(K, dtype=dt)
        kmask[2 * 128 + 112:2 * 128 + 128] = 0.0
    if c["lnf"]:
        g, beta = c["g"], c["beta"]
        Wg = W * g                                    # fl32(g o W): what the pack kernel stores
        folded = w16 or dt == F32 or mut in ("omit_mean_c1", "drop_last_chunk_of_wave")
        if not folded:
            xd = x.to(dt)
            mean, rstd = row_stats(x, dt)
            v = ((xd - mean) * rstd * g.to(dt) + beta.to(dt)) @ W.to(dt).t()
            if bias is not None:
                v = v + bias.to(dt)
            c1, c2 = fold_vectors(W[N - 1:], g, beta, None if bias is None else bias[N - 1:], dt)
            out["vpad"] = (c2[0] - rstd * mean * c1[0]).reshape(-1)
        else:
            mean, rstd = row_stats(x, dt)
            c1, c2 = fold_vectors(W, g, beta, bias, F64)
            if dt == F32:
                c1, c2 = c1.float(), c2.float()
            xo, Wo = x, Wg
            if w16:
                xo, Wo = rnd16(x, fp16), rnd16(Wg, fp16)
                if mut != "c1_unrounded_w16":
                    c1 = Wo.double().sum(dim=1).to(dt)
            xo = xo.to(dt) * kmask if kmask is not None else xo.to(dt)
            acc = xo @ Wo.to(dt).t()
            mc1 = torch.zeros((), dtype=dt) if mut == "omit_mean_c1" else mean * c1
            v = rstd * (acc - mc1) + c2
            out["vpad"] = (rstd * (0.0 - (mc1[:, N - 1:N] if mc1.dim() else mc1)) + c2[N - 1]).reshape(-1) + torch.zeros(M, dtype=dt)
    else:
        xo, Wo = (rnd16(x, fp16), rnd16(W, fp16)) if w16 else (x, W)
        xo = xo.to(dt) * kmask if kmask is not None else xo.to(dt)
        if c["KS"] > 1:
            for p in (0, 1):
                sl = slice(2048 * p, 2048 * p + 2048)
                a = xo[:, sl] @ Wo[:, sl].to(dt).t()
                if dt == F32:   # two slices of 1024, each accumulated on its own, then added
                    a = xo[:, 2048 * p:2048 * p + 1024] @ Wo[:, 2048 * p:2048 * p + 1024].to(dt).t()
                    a = a + xo[:, 2048 * p + 1024:2048 * p + 2048] @ Wo[:, 2048 * p + 1024:2048 * p + 2048].to(dt).t()
                if bias is not None and (p == 0 or mut == "bias_in_slices_0_and_2"):
                    a = a + bias.to(dt)
                out[f"acc{p}"] = a
            return out
        v = xo @ Wo.to(dt).t()
        if bias is not None:
            v = v + bias.to(dt)
    if c.get("R") is not None:
        R = c["R"]
        if mut == "tile1_reads_tile0_residual" and M > 32:
            R = R.clone()
            R[32:min(M, 64)] = c["R"][:min(M, 64) - 32]
        v = v + R.to(dt)
    out["Y"] = act_fn(v, c["act"], dt)
    return out


def true_ln_linear(c: dict) -> Tensor:
    """float64 LayerNorm-then-linear on the UNROUNDED weights and activations (what a 16-bit-weight form approximates)."""
    return fused_eval(dict(c, w16=0), F64)["Y"]


def candidates(Y: Tensor, N: int, mut: Optional[str] = None, vpad: Optional[Tensor] = None):
    """Per row and 16-column tile of Y [M][N]: (maximum over the valid columns, lowest column attaining it) as [M][NT]."""
    M = Y.shape[0]
    NT = (N + 15) // 16
    full = torch.full((M, NT * 16), -math.inf, dtype=Y.dtype)
    if mut == "pad_columns_in_argmax":
        full[:] = vpad.to(Y.dtype)[:, None]
    full[:, :N] = Y
    t = full.reshape(M, NT, 16)
    val = t.max(dim=2).values
    col = torch.arange(16)[None, None, :]
    hit = t == val[..., None]
    j = torch.where(hit, col, -1).max(dim=2).values if mut == "last_max_wins" else torch.where(hit, col, 16).min(dim=2).values
    return val, (j + 16 * torch.arange(NT)[None, :]).to(torch.int32)


def split_const(c: dict):
    """Row groups judged apart: the constant row of a folded form, and the others."""
    M = c["M"]
    if c.get("const_row") is None:
        return {"rows": torch.arange(M)}
    r = c["const_row"]
    return {"rows": torch.tensor([i for i in range(M) if i != r], dtype=torch.long), "const_row": torch.tensor([r])}


def judge_rows(got: Tensor, r64: Tensor, r32: Tensor, c: dict, name: str) -> Dict[str, Dict]:
    """attn_reference.compare of one [M][N] output, the constant row apart from the others."""
    return {f"{name}[{k}]": compare(got[idx], r64[idx], r32[idx]) for k, idx in split_const(c).items()}


def same_bits(a: Tensor, b: Tensor) -> bool:
    """torch.equal that counts NaN as equal to NaN."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    return bool(((a == b) | ((a != a) & (b != b))).all())


# ------------------------------------------------------------------------------------------------ inputs
def _gen(*key) -> torch.Generator:
    s = 1469598103
    for k in key:
        s = (s * 1000003 + int(k)) % 2147483647
    return torch.Generator().manual_seed(s)


TIE_PAIRS = ((0, 1), (1, 2), (3, 12), (7, 8), (0, 15))   # column pairs of tiles TIE_TILE0 .. + 4 that hold the same weight row
TIE_TILE0 = 5


@functools.lru_cache(maxsize=None)
def shared_direction() -> Tensor:
    """A zero-mean +-1 pattern every non-constant lm_head activation row carries: the planted weight rows point along it."""
    u = torch.ones(D)
    u[torch.randperm(D, generator=_gen(99))[:D // 2]] = -1.0
    return u


@functools.lru_cache(maxsize=None)
def weights(form: str, N: int, K: int) -> dict:
    """Random weights with a fixed seed, GPT-2-like scale; gains away from 1 and betas away from 0 for the folded forms.  lm_head:
    tied weight rows inside one tile at TIE_PAIRS, boosted along shared_direction() so that they are the tile's maximum."""
    f = FORMS[form]
    gen = _gen(len(form), N, K, sum(map(ord, form)))
    w = {"W": 0.02 * torch.randn(N, K, generator=gen), "bias": None, "g": None, "beta": None}
    if f["bias"]:
        w["bias"] = 0.1 * torch.randn(N, generator=gen) + 0.05
    if f["lnf"]:
        w["g"] = 0.4 + 1.6 * torch.rand(K, generator=gen)
        w["beta"] = 0.5 * torch.randn(K, generator=gen) + 0.3
    if form == "lm_head":
        for i, (a, b) in enumerate(TIE_PAIRS):
            t = TIE_TILE0 + i
            w["W"][16 * t + a] = 0.05 * shared_direction() / w["g"] + 0.002 * torch.randn(K, generator=gen)
            w["W"][16 * t + b] = w["W"][16 * t + a]
    return w


FORMS = {
    # name: shape, operands (issue table); out: "Y" row-major, "Yf" fragment-major
    "c_attn_embed": dict(N=3072, K=1024, lnf=1, bias=1, mode=DX_EMBED, out="Y", act=ACT_NONE),
    "c_attn_embed_tok": dict(N=3072, K=1024, lnf=1, bias=1, mode=DX_EMBED_TOK, out="Y", act=ACT_NONE),
    "c_attn_embed_tokpos": dict(N=3072, K=1024, lnf=1, bias=1, mode=DX_EMBED_TOKPOS, out="Y", act=ACT_NONE),
    "c_attn": dict(N=3072, K=1024, lnf=1, bias=1, mode=DX_COMBINE4, out="Y", act=ACT_NONE),
    "attn_proj": dict(N=1024, K=1024, lnf=0, bias=1, mode=DX_PLAIN, out="Yf", act=ACT_NONE, resid=1),
    "c_fc": dict(N=4096, K=1024, lnf=1, bias=1, mode=DX_PLAIN, out="Yf", act=ACT_GELU_NEW),
    "mlp_proj": dict(N=1024, K=4096, lnf=0, bias=1, mode=DX_PLAIN, out="acc", act=ACT_NONE),
    "lm_head": dict(N=VOCAB, K=1024, lnf=1, bias=0, mode=DX_COMBINE4, out="Y", act=ACT_NONE, cand=1),
}
FUSED_ROWS = (1, 16, 17, 29, 32, 33, 64, 65, 97, 128)
W16_ROWS = (33, 64, 65, 128)
NAN_PAD_ROWS = (29, 65, 97)     # cases whose activation / residual / accumulator pad rows hold NaN


def _rows(gen, M, K, const_row):
    """Rows with the residual stream's character: per-row mean offsets of up to a few standard deviations, one constant row."""
    off = 3.0 * (2.0 * torch.rand(M, 1, generator=gen) - 1.0)
    x = off + torch.randn(M, K, generator=gen)
    if const_row is not None:
        x[const_row] = CONST_VALUE
    return x


def fused_case(form: str, M: int, w16: int = 0, N: Optional[int] = None) -> dict:
    f = FORMS[form]
    N = N or f["N"]
    K = f["K"]
    gen = _gen(sum(map(ord, form)), M, w16, N)
    c = dict(f, name=f"{form},N={N},M={M},w16={w16}", form=form, M=M, N=N, K=K, w16=w16, KS=K // 1024, NT=(N + 15) // 16,
             nan_pad=M in NAN_PAD_ROWS, **weights(form, N, K))
    const_row = CONST_ROW if (M > CONST_ROW and f["lnf"]) else None
    c["const_row"] = const_row
    rows = tiles_of(M) * 32
    mode = f["mode"]
    if mode >= DX_EMBED:
        c["wte"] = _rows(gen, WTE_ROWS, K, None)
        c["step"] = 0 if FUSED_ROWS.index(M) % 2 == 0 else 37
        tok = torch.randint(0, WTE_ROWS, (rows,), generator=gen)
        tok[0], tok[M - 1] = 0, WTE_ROWS - 1
        if M > 2:
            tok[1] = WTE_ROWS - 1
        c["tok"] = tok.to(torch.int32)
        c["pos"] = ((torch.arange(rows) * 37 + 11) % WTE_ROWS).to(torch.int32)   # distinct per row (37 is coprime to 160)
        ids = torch.randint(0, WTE_ROWS, (rows, c["step"] + 3), generator=gen)
        ids[:, c["step"]] = tok
        c["ids"] = ids
        c["const_row"] = None      # a sum of two embedding rows is never constant
    elif mode == DX_COMBINE4:
        x = _rows(gen, M, K, const_row)
        if form == "lm_head":
            x = x + 2.0 * shared_direction()
            if const_row is not None:
                x[const_row] = CONST_VALUE
            # row 0: the only valid logit of the last tile (column N - 1) lies below what the tile's zero-padded columns would give
            x[0] = x[0] - 100.0 * c["g"] * c["W"][N - 1]
        A0, A1 = 0.5 * torch.randn(M, K, generator=gen), 0.5 * torch.randn(M, K, generator=gen)
        if const_row is not None:
            A0[const_row], A1[const_row] = 0.0, 0.0
        c["A0"], c["A1"] = A0, A1
        c["X"] = (x - A1) - A0
    else:
        if form == "mlp_proj":
            c["X"] = gelu_new(_rows(gen, M, K, None), F32)
        else:
            c["X"] = _rows(gen, M, K, const_row)
        if f.get("resid"):
            c["R"] = _rows(gen, M, N, None)
    return c


def fused_cases():
    """Every launch of the fused plan the GPU test makes: (form, M, w16, N)."""
    for form in FORMS:
        if form == "lm_head":
            continue
        for M in FUSED_ROWS:
            yield form, M, 0, None
    for M in (1, 29, 32):
        yield "lm_head", M, 0, VOCAB            # the wave kernel
    yield "lm_head", 29, 0, VOCAB_SMALL         # NT = 514: the smallest vocabulary on the wave kernel, partial last tile
    for M in (33, 128):
        yield "lm_head", M, 0, VOCAB            # the generic kernel, shuffle arg-max
    for w16 in (1, 2):
        for form in FORMS:
            for M in W16_ROWS:
                yield form, M, w16, None


def expected_kernel(c: dict) -> int:
    """The kernel direct_dispatch picks (skinny_direct.inc / decoder.hip)."""
    mt = tiles_of(c["M"])
    if c["lnf"] and c["mode"] == DX_COMBINE4 and c["NT"] > 512 and mt == 1:
        return RAN_LM_WAVE
    if not c["lnf"] and c["mode"] == DX_PLAIN and c["KS"] == 1 and mt == 1 and c["NT"] <= 64 and c["M"] > 16 and not c.get("cand"):
        return RAN_HALF
    return RAN_GENERIC


# prefill family: (N, K, rows); fst0 = bias + ReLU, fst2 = bias, neither has a residual (decoder.hip prefill)
PREFILL_COMBOS = (("fst0", ACT_RELU), ("fst2", ACT_NONE))
PREFILL_SHAPES = tuple((1024, 1024, M) for M in (1, 29, 32, 33, 64, 97, 128)) + tuple((16400, 1024, M) for M in (1, 29, 31)) + \
    ((49152, 1024, 29),) + tuple((16400, 1024, M) for M in (32, 33, 128))


@functools.lru_cache(maxsize=None)
def prefill_weights(N: int, K: int):
    gen = _gen(7, N, K)
    return 0.02 * torch.randn(N, K, generator=gen), 0.1 * torch.randn(N, generator=gen) + 0.05


def prefill_case(N: int, K: int, M: int, combo: int = 0) -> dict:
    name, act = PREFILL_COMBOS[combo]
    W, b = prefill_weights(N, K)
    gen = _gen(11, N, K, M, combo)
    return {"name": f"{name},N={N},K={K},M={M}", "N": N, "K": K, "M": M, "act": act, "W": W, "bias": b, "X": _rows(gen, M, K, None),
            "nan_pad": M in NAN_PAD_ROWS, "KS": pick_ks(N, K), "ldy": N + 8}


def prefill_cases():
    for N, K, M in PREFILL_SHAPES:
        for combo in ((0, 1) if N == 1024 else (1,)):    # ukv (the wide shapes) runs as fst2 does: bias, no activation
            yield N, K, M, combo


def prefill_eval(c: dict, dt, mut: Optional[str] = None) -> Tensor:
    X = c["X"]
    if mut == "swap_row_halves":
        X = residual_stream({"M": c["M"], "mode": DX_PLAIN, "X": X}, mut)
    if mut == "drop_last_chunk_of_wave":
        X = X.clone()
        pw = c["K"] // (8 * c["KS"] * 8)
        X[:, (2 * pw + pw - 1) * 8:(2 * pw + pw) * 8] = 0.0     # wave 2 of K slice 0 loses its last chunk
    return plain_linear(X, c["W"], c["bias"], None, c["act"], dt)


# ------------------------------------------------------------------------------------------------ the comparison
def _exact(ok: bool) -> Dict[str, float]:
    return {"err": 0.0 if ok else math.inf, "noise": 0.0, "bound": 0.0, "used": 0.0 if ok else math.inf, "ok": bool(ok)}


def as_kernel(c: dict, ev: Dict[str, Tensor], mut: Optional[str] = None) -> Dict[str, Tensor]:
    """What a kernel that computed the evaluation ``ev`` would store: fp32 values, the rebuilt rows, the candidates of ITS logits."""
    got = {k: ev[k].float() for k in ("Y", "acc0", "acc1") if k in ev}
    if c["mode"] != DX_PLAIN:
        got["xout"] = ev["x"].float()
    if c.get("cand"):
        got["cand_val"], got["cand_idx"] = candidates(got["Y"], c["N"], mut, ev["vpad"].float())
    return got


def judge_fused(got: Dict[str, Tensor], c: dict, r64: Dict[str, Tensor], r32: Dict[str, Tensor]) -> Dict[str, Dict]:
    """Every output of one launch of the fused plan.  Y / acc0 / acc1 [M][N] against the bound; exact: xout [M][K] against the fp32
    rows of the reference, cand_val / cand_idx [M][NT] against the maxima of the Y values in ``got`` itself, cand_idx < N."""
    res = {}
    for k in ("Y", "acc0", "acc1"):
        if k in r64:
            res.update(judge_rows(got[k], r64[k], r32[k], c, k))
    if "xout" in got:
        res["xout"] = _exact(same_bits(got["xout"], r64["x"]))
    if c.get("cand"):
        val, idx = candidates(got["Y"], c["N"])
        res["cand_val"] = _exact(same_bits(got["cand_val"], val))
        res["cand_idx"] = _exact(same_bits(got["cand_idx"], idx) and bool((got["cand_idx"] < c["N"]).all()) and bool((got["cand_idx"] >= 0).all()))
    return res


def applies(mut: str, c: dict) -> bool:
    """Whether a mutation changes anything in a fused case."""
    M = c["M"]
    return {"drop_last_chunk_of_wave": True, "swap_row_halves": M > 16, "omit_mean_c1": bool(c["lnf"]),
            "c1_unrounded_w16": bool(c["lnf"] and c["w16"]), "bias_in_slices_0_and_2": c["KS"] > 1, "omit_acc23": c["mode"] == DX_COMBINE4,
            "position_step_plus_1": c["mode"] >= DX_EMBED, "last_max_wins": bool(c.get("cand")), "pad_columns_in_argmax": bool(c.get("cand")),
            "tile1_reads_tile0_residual": c.get("R") is not None and M > 32}[mut]
