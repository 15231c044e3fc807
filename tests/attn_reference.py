"""Float64 restatement of GPT2PseudoAttention._attn (src/language_model/language_model.py:84-122, forward :124-160) for the
per-kernel attention tests, the input builders those tests share, and the comparison they assert with.  TEST INFRASTRUCTURE ONLY.

The formulas (every function takes ``dt``: torch.float64 for the reference, torch.float32 for the noise measurement):
  scores = q . k / 8; in the teacher-forced forms future token columns are REPLACED by -1e4 (the image column 0 is never
  replaced); the additive padding mask is (1 - [1 | attention_mask]) * -1e4; softmax; the optional dropout mask (0 or 1/(1-p));
  the product with V.  The backward of the fp32 kernels is torch autograd through that function (tf_grads); the 16-bit training
  kernels get the closed form of that backward (tf_backward_manual) because they round inside it, and the closed form is checked
  against autograd (tests/test_attention_reference.py).

Where the reference rounds to the 16-bit type, because the kernel does:
  kv16 decode (attn_decode_kv16_wave_kernel, csrc/attn_decode.hip): the new token's k / v before they take part as the last key and are stored to the
      cache; the output when it goes to out16.
  attn16_fwd_kernel: the UNNORMALISED probabilities exp(s - max) times the dropout mask, as the MFMA operand of P V
      (attn_train16.hip:153-163); the output, after the division by the sum of the UNROUNDED exponentials (:136-147, :171-181).
  attn16_bwd_kernel: P = exp(s - lse) times the dropout mask as the operand of dV = (P mask)^T dO, and dS = P (dP mask - delta) / 8
      as the operand of dQ = dS K and dK = dS^T Q (pack8 calls of the dQ and the dK / dV loops); d_qkv16 on store.  delta =
      rowsum(dO . O) is summed in fp32 from the 16-bit dO and the 16-bit forward output; d_ukv stays fp32.
  fp32 kernels with a 16-bit copy (out16 of the prefill kernels, d_qkv16 of the fp32 backward): the final store only.

Tolerance: bound = margin * max|ref32 - ref64| + floor, floor = 2^-23 max|ref| (fp32 outputs) or the 16-bit type's ulp at max|ref|.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

Tensor = torch.Tensor
MASK_VALUE = -1e4
MARGIN = 8.0


# ------------------------------------------------------------------------------------------------ number formats
def t16(fp16) -> torch.dtype:
    return torch.float16 if fp16 else torch.bfloat16


def rnd16(x: Tensor, fp16) -> Tensor:
    """Round to the 16-bit type (nearest even) and widen back to x's dtype."""
    return x.to(torch.float32).to(t16(fp16)).to(x.dtype)


def to_bits(x: Tensor, fp16) -> Tensor:
    """fp32 values that are exactly representable -> the int16 bit pattern tensor the kernels read."""
    return x.to(t16(fp16)).view(torch.int16)


def from_bits(b: Tensor, fp16) -> Tensor:
    return b.view(t16(fp16)).to(torch.float32)


def ulp16(fp16, at: float) -> float:
    """One unit in the last place of the 16-bit type at magnitude ``at`` (bf16: 8 significand bits, fp16: 11)."""
    if at <= 0.0:
        return 0.0
    e = math.floor(math.log2(at))
    if fp16:
        e = max(e, -14)
    return 2.0 ** (e - (10 if fp16 else 7))


def bound(ref64: Tensor, ref32: Tensor, out16=None, margin: float = MARGIN, extra_floor: float = 0.0) -> Dict[str, float]:
    """The bound of one output tensor from the reference alone (see the module docstring).  extra_floor: flip_floor() below."""
    r64 = ref64.double()
    noise = float((ref32.double() - r64).abs().max())
    mx = float(r64.abs().max())
    floor = (ulp16(out16, mx) if out16 is not None else mx * 2.0 ** -23) + extra_floor
    return {"noise": noise, "floor": floor, "bound": margin * noise + floor, "max": mx}


def compare(got: Tensor, ref64: Tensor, ref32: Tensor, out16=None, margin: float = MARGIN, extra_floor: float = 0.0) -> Dict[str, float]:
    """max |got - ref64| over the WHOLE tensor against the bound; NaN / inf anywhere fails.  Returns the figures with ``ok``."""
    b = bound(ref64, ref32, out16, margin, extra_floor)
    g = got.detach().double().cpu()
    assert g.shape == ref64.shape, (g.shape, ref64.shape)
    finite = bool(torch.isfinite(g).all())
    err = float((g - ref64.double()).abs().max()) if finite else float("inf")
    b.update(err=err, ok=finite and err <= b["bound"], ratio=err / b["noise"] if b["noise"] > 0 else float("inf") if err > 0 else 0.0,
             used=err / b["bound"] if b["bound"] > 0 else (0.0 if err == 0 else float("inf")))
    return b


# ------------------------------------------------------------------------------------------------ dropout masks on the host
def philox_mask(seed: int, stream_id: int, p: float, shape, row_len: int = 0) -> Tensor:
    """rgrg_dropout_mask_f32 on the host: Philox4x32-7, key = seed, counter = (index / 4, stream_id), element index % 4; the index of
    an attention-probability mask pads a row of keys to a multiple of 4 (row_len = T + 1).  The GPU test checks it bit for bit."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    if row_len > 0:
        pitch = (row_len + 3) & ~3
        i = (i // np.uint64(row_len)) * np.uint64(pitch) + i % np.uint64(row_len)
    ctr = i >> np.uint64(2)
    M = np.uint64(0xFFFFFFFF)
    c0, c1 = ctr & M, ctr >> np.uint64(32)
    c2, c3 = np.full_like(ctr, stream_id & 0xFFFFFFFF), np.zeros_like(ctr)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    w = np.stack([c0, c1, c2, c3], axis=1)[np.arange(n), (i & np.uint64(3)).astype(np.int64)]
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(np.where(u < np.float32(p), np.float32(0.0), keep).astype(np.float32)).reshape(shape)


# ------------------------------------------------------------------------------------------------ the attention itself
def attn_core(q: Tensor, K: Tensor, V: Tensor, add: Optional[Tensor], allowed: Optional[Tensor], drop: Optional[Tensor], dt,
              scale: float = 0.125, p16=None):
    """_attn on q [B,H,Q,64], K / V [B,H,N,64]: ``allowed`` [.., Q, N] bool (False -> the score is REPLACED by -1e4), ``add``
    broadcastable additive mask, ``drop`` the dropout mask.  p16 (None / 0 bf16 / 1 fp16): the attn16_fwd_kernel rounding of the
    unnormalised probabilities.  Returns (out [B,H,Q,64], lse [B,H,Q], probabilities after softmax)."""
    q, K, V = q.to(dt), K.to(dt), V.to(dt)
    s = torch.matmul(q, K.transpose(-1, -2)) * torch.tensor(scale, dtype=dt)
    if allowed is not None:
        s = torch.where(allowed, s, torch.tensor(MASK_VALUE, dtype=dt))
    if add is not None:
        s = s + add.to(dt)
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    den = e.sum(dim=-1, keepdim=True)
    lse = (m + torch.log(den)).squeeze(-1)
    if p16 is None:
        w = e / den
        if drop is not None:
            w = w * drop.to(dt)
        return torch.matmul(w, V), lse, e / den
    ed = e if drop is None else e * drop.to(dt)
    return torch.matmul(rnd16(ed, p16), V) / den, lse, e / den


def pad_add(am: Optional[Tensor], dt) -> Optional[Tensor]:
    """attention_mask [S,T] -> additive [S,1,1,1+T]: (1 - [1 | am]) * -1e4 (language_model.py:316-334)."""
    if am is None:
        return None
    full = torch.cat((torch.ones(am.shape[0], 1, dtype=dt), am.to(dt)), dim=1)
    return ((1.0 - full) * MASK_VALUE)[:, None, None, :]


def causal_allowed(T: int) -> Tensor:
    """[T, T+1] bool: key 0 (the image) always, token key c for queries i >= c - 1."""
    i = torch.arange(T)[:, None]
    c = torch.arange(T + 1)[None, :]
    return (c == 0) | (c - 1 <= i)


# Mutations of the REFERENCE (tests/test_attention_reference.py: each must be rejected by compare() with the derived bound).
MUTATIONS = ("drop_last_key", "drop_first_of_last_chunk", "read_next_slot", "ignore_ancestor", "ignore_mask_one_key",
             "skip_causal_one_column", "wrong_dropout_stream", "scale_sqrt65", "round_v_again", "omit_ukv_scale")


def tf_forward(qkv: Tensor, ukv: Tensor, am: Optional[Tensor], drop: Optional[Tensor], dt, *, p16=None, mut: Optional[str] = None,
               mut_col: int = 1, chunk: int = 32, drop_alt: Optional[Tensor] = None):
    """Teacher-forced attention (no layer_past).  qkv [S,T,3,H,64] (q | k | v of the tokens), ukv [S,2,H,64] (image key, value),
    am [S,T] or None, drop [S,H,T,T+1] or None.  Returns out [S,T,H,64], lse [S,T,H], P [S,H,T,T+1].
    mut: one of MUTATIONS applied to this evaluation (mut_col = the key the single-key mutations touch)."""
    S, T = qkv.shape[:2]
    q = qkv[:, :, 0].permute(0, 2, 1, 3)
    K = torch.cat((ukv[:, 0][:, :, None, :], qkv[:, :, 1].permute(0, 2, 1, 3)), dim=2)
    V = torch.cat((ukv[:, 1][:, :, None, :], qkv[:, :, 2].permute(0, 2, 1, 3)), dim=2)
    allowed = causal_allowed(T)
    add = pad_add(am, dt)
    add = torch.zeros(S, 1, 1, T + 1, dtype=dt) if add is None else add
    add = add.expand(S, 1, T, T + 1).clone()
    scale = 0.125
    if mut == "drop_last_key":          # every query loses its own token, the last key it sees
        add[:, :, torch.arange(T), torch.arange(T) + 1] = -math.inf
    elif mut == "drop_first_of_last_chunk":   # the first key of the last 32-key tile
        add[..., (T // chunk) * chunk if T >= chunk else 0] = -math.inf
    elif mut == "read_next_slot":
        K, V = K.clone(), V.clone()
        K[:, :, mut_col], V[:, :, mut_col] = K[:, :, min(mut_col + 1, T)], V[:, :, min(mut_col + 1, T)]
    elif mut == "ignore_mask_one_key":
        add[..., mut_col] = 0.0
    elif mut == "skip_causal_one_column":
        allowed = allowed.clone()
        allowed[:, mut_col] = True
    elif mut == "wrong_dropout_stream":
        drop = drop_alt
    elif mut == "scale_sqrt65":
        scale = 1.0 / math.sqrt(65.0)
    elif mut == "round_v_again":
        V = rnd16(V, 0)
    out, lse, P = attn_core(q, K, V, add, allowed, drop, dt, scale, p16)
    return out.permute(0, 2, 1, 3), lse.permute(0, 2, 1), P


def tf_grads(qkv: Tensor, ukv: Tensor, am: Optional[Tensor], drop: Optional[Tensor], d_att: Tensor, dt, **kw):
    """torch autograd through tf_forward: (d_qkv [S,T,3,H,64], d_ukv [S,2,H,64]) for the output gradient d_att [S,T,H,64]."""
    a = qkv.to(dt).clone().requires_grad_(True)
    b = ukv.to(dt).clone().requires_grad_(True)
    out, _, _ = tf_forward(a, b, am, drop, dt, **kw)
    out.backward(d_att.to(dt))
    return a.grad, b.grad


def tf_backward_manual(qkv: Tensor, ukv: Tensor, am: Optional[Tensor], drop: Optional[Tensor], d_att: Tensor, att: Tensor, lse: Tensor,
                       dt, *, p16=None, mut: Optional[str] = None, mut_col: int = 1, drop_alt: Optional[Tensor] = None):
    """The closed form the backward kernels evaluate, from the forward's saved output ``att`` [S,T,H,64] and ``lse`` [S,T,H]:
    P = exp(s - lse), delta = rowsum(dO . O), dP = dO V^T, dS = P (dP mask - delta) / 8 on the columns that were not replaced,
    dV = (P mask)^T dO, dK = dS^T Q, dQ = dS K.  p16: P mask and dS rounded to the 16-bit type (attn16_bwd_kernel's operands).
    Returns (d_qkv [S,T,3,H,64], d_ukv [S,2,H,64], delta [S,T,H], the image-key column of P mask and of dS before the rounding
    [S,H,T] each)."""
    S, T = qkv.shape[:2]
    qkv, ukv, dO = qkv.to(dt), ukv.to(dt), d_att.to(dt).permute(0, 2, 1, 3)
    q = qkv[:, :, 0].permute(0, 2, 1, 3)
    K = torch.cat((ukv[:, 0][:, :, None, :], qkv[:, :, 1].permute(0, 2, 1, 3)), dim=2)
    V = torch.cat((ukv[:, 1][:, :, None, :], qkv[:, :, 2].permute(0, 2, 1, 3)), dim=2)
    allowed = causal_allowed(T)
    add = pad_add(am, dt)
    add = torch.zeros(S, 1, 1, T + 1, dtype=dt) if add is None else add
    add = add.expand(S, 1, T, T + 1).clone()
    scale = 0.125
    if mut == "drop_last_key":
        add[:, :, torch.arange(T), torch.arange(T) + 1] = -math.inf
    elif mut == "drop_first_of_last_chunk":
        add[..., (T // 32) * 32 if T >= 32 else 0] = -math.inf
    elif mut == "read_next_slot":
        K, V = K.clone(), V.clone()
        K[:, :, mut_col], V[:, :, mut_col] = K[:, :, min(mut_col + 1, T)], V[:, :, min(mut_col + 1, T)]
    elif mut == "ignore_mask_one_key":
        add[..., mut_col] = 0.0
    elif mut == "skip_causal_one_column":
        allowed = allowed.clone()
        allowed[:, mut_col] = True
    elif mut == "wrong_dropout_stream":
        drop = drop_alt
    elif mut == "scale_sqrt65":
        scale = 1.0 / math.sqrt(65.0)
    elif mut == "round_v_again":
        V = rnd16(V, 0)
    sc = torch.tensor(scale, dtype=dt)
    s = torch.where(allowed, torch.matmul(q, K.transpose(-1, -2)) * sc, torch.tensor(MASK_VALUE, dtype=dt)) + add
    P = torch.exp(s - lse.to(dt).permute(0, 2, 1)[..., None])
    delta = (dO * att.to(dt).permute(0, 2, 1, 3)).sum(-1)
    mk = torch.ones((), dtype=dt) if drop is None else drop.to(dt)
    dP = torch.matmul(dO, V.transpose(-1, -2))
    dS = torch.where(allowed, P * (dP * mk - delta[..., None]) * sc, torch.zeros((), dtype=dt))
    Pm = P * mk
    pre = (Pm[..., 0], dS[..., 0])
    if p16 is not None:
        Pm, dS = rnd16(Pm, p16), rnd16(dS, p16)
    dV = torch.matmul(Pm.transpose(-1, -2), dO)
    dK = torch.matmul(dS.transpose(-1, -2), q)
    dQ = torch.matmul(dS, K)
    d_qkv = torch.stack((dQ, dK[:, :, 1:], dV[:, :, 1:]), dim=1).permute(0, 3, 1, 2, 4)   # [S,3,H,T,64] -> [S,T,3,H,64]
    d_ukv = torch.stack((dK[:, :, 0], dV[:, :, 0]), dim=1)
    return d_qkv, d_ukv, delta.permute(0, 2, 1), pre


def flip_floor(x64: Tensor, x32: Tensor, mult: Tensor, fp16, margin: float = MARGIN) -> float:
    """An fp32 output downstream of a 16-bit MFMA operand: an operand x whose value lies within the evaluation error of a
    rounding boundary of the 16-bit type may round either way in a correct kernel, and the output element it feeds then moves by
    ulp16(x) |multiplier|.  x64 / x32 [S,H,T]: the operand (image-key column) in the float64 and the fp32 evaluation of the
    reference, before the rounding; an operand is ambiguous when its distance to the nearest boundary is at most margin *
    max(|x32 - x64|, 2^-23 |x|).  mult [S,H,T,64]: what it multiplies (dO for P, q for dS).  Returns the largest sum over the
    ambiguous operands of one output element."""
    x = x64.double()
    e = torch.floor(torch.log2(x.abs().clamp(min=1e-300)))
    if fp16:
        e = e.clamp(min=-14.0)
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - (10 if fp16 else 7))
    to_mid = ulp / 2 - (x - rnd16(x, fp16)).abs()
    amb = to_mid <= margin * torch.maximum((x32.double() - x).abs(), x.abs() * 2.0 ** -23)
    return float(((amb * ulp)[..., None] * mult.double().abs()).sum(dim=2).max())


def decode_forward(q: Tensor, kn: Tensor, vn: Tensor, K: Tensor, V: Tensor, step: int, src: Optional[Tensor], kmask: Optional[Tensor],
                   dt, *, kv16=None, out16: bool = False, mut: Optional[str] = None, mut_col: int = 1, chunk: int = 144):
    """One decode step (layer_past given).  q / kn / vn [S,H,64] (the new token), K / V [S,H,Tslots,64] the cache (the exact fp32
    widening of a 16-bit cache), keys = slots 0 .. step + 1, slot step + 1 = the new token's k / v (rounded to the cache type
    first when kv16 is 0 / 1).  src [S,Tslots] ancestor rows, kmask [S,Tslots] additive.  Returns (out [S,H,64], k stored, v stored)."""
    S, H = q.shape[:2]
    nkeys, slot = step + 2, step + 1
    if kv16 is not None:
        kn, vn = rnd16(kn, kv16), rnd16(vn, kv16)
    rows = (src[:, :nkeys] if src is not None else torch.arange(S)[:, None].expand(S, nkeys)).long().clone()
    cols = torch.arange(nkeys)[None, :].expand(S, nkeys).clone()
    add = torch.zeros(S, 1, 1, nkeys, dtype=dt) if kmask is None else kmask[:, None, None, :nkeys].to(dt).clone()
    scale = 0.125
    if mut == "ignore_ancestor":
        rows[:, mut_col] = torch.arange(S)
    elif mut == "read_next_slot":
        cols[:, mut_col] = min(mut_col + 1, slot - 1)
    Kg = K[rows, :, cols].permute(0, 2, 1, 3).clone()   # [S,nkeys,H,64] -> [S,H,nkeys,64]
    Vg = V[rows, :, cols].permute(0, 2, 1, 3).clone()
    Kg[:, :, slot], Vg[:, :, slot] = kn, vn
    if mut == "drop_last_key":
        add[..., slot] = -math.inf
    elif mut == "drop_first_of_last_chunk":
        add[..., ((nkeys - 1) // chunk) * chunk] = -math.inf
    elif mut == "ignore_mask_one_key":
        add[..., mut_col] = 0.0
    elif mut == "scale_sqrt65":
        scale = 1.0 / math.sqrt(65.0)
    elif mut == "round_v_again":
        Vg = rnd16(Vg, 0)
    out, _, P = attn_core(q[:, :, None, :], Kg, Vg, add, None, None, dt, scale)
    out = out[:, :, 0]
    if out16:
        out = rnd16(out, kv16)
    return out, kn, vn, P[:, :, 0]


# ------------------------------------------------------------------------------------------------ inputs
def edge_weight(q: Tensor, K: Tensor, desig: Tensor, visible: Tensor, add: Optional[Tensor], big: float = 0.0):
    """Edge-weighted inputs.  q [B,H,Q,64], K [B,H,N,64] (float64), desig [B,H] = the designated key of every (row, head),
    visible [Q,N] bool, add [B,1,1 or Q,N] additive mask or None.  Along one fixed unit direction u: every key loses its u
    component, the designated key becomes 8 u, and every query gets q . u = log(sum of exp(score) over its other visible,
    unmasked keys) - so the designated key's softmax weight is exactly 1/2 for every query that sees it (before any 16-bit
    rounding of the inputs).  big > 0: q . u = big instead, a score of that magnitude that holds the row's maximum."""
    B, H, Q, _ = q.shape
    N = K.shape[2]
    g = torch.Generator().manual_seed(1234)
    u = torch.randn(64, generator=g, dtype=torch.float64)
    u /= u.norm()
    K = K - (K @ u)[..., None] * u
    q = q - (q @ u)[..., None] * u
    is_d = torch.arange(N)[None, None, :] == desig[:, :, None]                      # [B,H,N]
    K = torch.where(is_d[..., None], 8.0 * u, K)
    s = torch.matmul(q, K.transpose(-1, -2)) / 8.0
    s = torch.where(visible, s, torch.tensor(-math.inf, dtype=torch.float64))
    if add is not None:
        s = s + add.double()
    s = torch.where(is_d[:, :, None, :], torch.tensor(-math.inf, dtype=torch.float64), s)
    s = torch.where(s < -5000.0, torch.tensor(-math.inf, dtype=torch.float64), s)   # keys under the padding mask weigh nothing
    lo = torch.logsumexp(s, dim=-1)                                                   # [B,H,Q]
    lo = torch.where(torch.isfinite(lo), lo, torch.zeros((), dtype=torch.float64))
    a = torch.full_like(lo, big) if big > 0 else lo
    return q + a[..., None] * u, K


def _cycle(cands, shape, offset=0):
    n = int(np.prod(shape))
    return torch.tensor([cands[(i + offset) % len(cands)] for i in range(n)]).reshape(shape)


def tile_edges(nkeys: int, tile: int):
    """Key 0 (the image), the last key, and the first and last key of every tile / chunk of ``tile`` keys."""
    c = {0, nkeys - 1}
    for b in range(tile, nkeys, tile):
        c.update((b - 1, b))
    return sorted(c)


def make_am(kind: Optional[str], S: int, T: int, g: torch.Generator) -> Optional[Tensor]:
    """attention_mask [S,T]: None, "right" / "left" padded rows of random valid length, "all": row 0 entirely masked."""
    if kind is None:
        return None
    am = torch.zeros(S, T)
    for s in range(S):
        L = int(torch.randint(1, T + 1, (1,), generator=g))
        if kind == "left":
            am[s, T - L:] = 1.0
        else:
            am[s, :L] = 1.0
    if kind == "all":
        am[0] = 0.0
    return am


def tf_inputs(S: int, T: int, H: int, seed: int, am_kind: Optional[str] = None, fmt16=None, weighted: Optional[str] = "half",
              offset: int = 0, desig_all: Optional[int] = None):
    """Inputs of a teacher-forced case: qkv [S,T,3,H,64], ukv [S,2,H,64] fp32 (exactly representable in the 16-bit type when
    fmt16 is 0 / 1), am, d_att [S,T,H,64], desig [S,H].  weighted: None (plain N(0,1)), "half" (the designated key of every
    (row, head) - cycling through tile_edges(T + 1, 32) - holds half of the softmax), "big_first" / "big_last" (a score of 60 on
    the image key / on the first key of the last 32-key tile)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(S, T, 3, H, 64, generator=g, dtype=torch.float64)
    ukv = torch.randn(S, 2, H, 64, generator=g, dtype=torch.float64)
    d_att = torch.randn(S, T, H, 64, generator=g, dtype=torch.float64)
    am = make_am(am_kind, S, T, g)
    desig = _cycle(tile_edges(T + 1, 32), (S, H), offset)
    if weighted == "big_first":
        desig = torch.zeros(S, H, dtype=torch.long)
    elif weighted == "big_last":
        desig = torch.full((S, H), (T // 32) * 32 if T >= 32 else T)
    if desig_all is not None:   # one key for every (row, head): the sensitivity tests aim a mutation at it
        desig = torch.full((S, H), desig_all)
    if am is not None:   # a masked designated key weighs nothing: fall back to the image key
        tok_ok = torch.cat((torch.ones(S, 1), am), dim=1)
        desig = torch.where(tok_ok.gather(1, desig) > 0, desig, torch.zeros_like(desig))
    if weighted:
        q = qkv[:, :, 0].permute(0, 2, 1, 3)
        K = torch.cat((ukv[:, 0][:, :, None, :], qkv[:, :, 1].permute(0, 2, 1, 3)), dim=2)
        q, K = edge_weight(q, K, desig, causal_allowed(T), pad_add(am, torch.float64), 60.0 if weighted.startswith("big") else 0.0)
        qkv[:, :, 0], qkv[:, :, 1], ukv[:, 0] = q.permute(0, 2, 1, 3), K[:, :, 1:].permute(0, 2, 1, 3), K[:, :, 0]
    cast = (lambda t: rnd16(t.float(), fmt16)) if fmt16 is not None else (lambda t: t.float())
    return {"qkv": cast(qkv), "ukv": cast(ukv), "am": am, "d_att": cast(d_att), "desig": desig, "S": S, "T": T, "H": H}


def designated_weight_ok(P: Tensor, desig: Tensor, am: Optional[Tensor] = None) -> bool:
    """Every (row, head) has a query for which the designated key holds 0.2 .. 0.8 of the softmax (rows whose tokens are all
    masked have only the image key to attend to and are exempt).  P [S,H,Q,N]."""
    w = P.gather(3, desig[:, :, None, None].expand(-1, -1, P.shape[2], 1))[..., 0]     # [S,H,Q]
    ok = ((w >= 0.2) & (w <= 0.8)).any(dim=-1)
    if am is not None:
        ok = ok | (am.sum(dim=1) == 0)[:, None]
    return bool(ok.all())


def decode_inputs(S: int, H: int, nkeys: int, slots: int, seed: int, with_src: bool = False, kmask_kind: Optional[str] = None,
                  kv16=None, weighted: Optional[str] = "half", tile: int = 144, offset: int = 0, desig_all: Optional[int] = None):
    """Inputs of a decode step with nkeys = step + 2 keys over a cache of ``slots`` slots: q / kn / vn [S,H,64], K / V
    [S,H,slots,64] (16-bit representable when kv16 is 0 / 1) with NaN in every slot >= nkeys - 1 (the new token's slot is written
    by the kernel, later slots are unused: reading either must show), src [S,slots] (ancestors inside groups of 4 rows; the
    designated slot of head 0 points at ANOTHER row where the group has one), kmask [S,slots] additive (None, "random",
    "all_tokens", "current"), desig [S,H] cycling through tile_edges(nkeys, tile), equal inside a group of 4 rows."""
    g = torch.Generator().manual_seed(seed)
    step, slot = nkeys - 2, nkeys - 1
    q, kn, vn = (torch.randn(S, H, 64, generator=g, dtype=torch.float64) for _ in range(3))
    K = torch.randn(S, H, slots, 64, generator=g, dtype=torch.float64)
    V = torch.randn(S, H, slots, 64, generator=g, dtype=torch.float64)
    grp = torch.arange(S) // 4
    desig = _cycle(tile_edges(nkeys, tile), ((S + 3) // 4, H), offset)[grp]
    if weighted == "big_first":
        desig = torch.zeros(S, H, dtype=torch.long)
    elif weighted == "big_last":
        desig = torch.full((S, H), ((nkeys - 1) // tile) * tile)
    if desig_all is not None:
        desig = torch.full((S, H), desig_all)
    src = None
    if with_src:
        size = torch.minimum(torch.full((S,), 4), S - 4 * grp)
        src = (4 * grp[:, None] + (torch.rand(S, slots, generator=g) * size[:, None]).long().clamp(max=3)).clamp(max=S - 1)
        other = 4 * grp + (torch.arange(S) % 4 + 1) % size
        src[torch.arange(S), desig[:, 0]] = other
        src[:, slot] = torch.arange(S)   # stale in the product: that key comes from the new token
        src = src.int()
    kmask = None
    if kmask_kind:
        kmask = torch.zeros(S, slots)
        if kmask_kind == "random":
            kmask[:, 1:] = (torch.rand(S, slots - 1, generator=g) < 0.3).float() * MASK_VALUE
        elif kmask_kind == "all_tokens":
            kmask[:, 1:] = MASK_VALUE
        elif kmask_kind == "current":
            kmask[:, slot] = MASK_VALUE
        masked = kmask.gather(1, desig) < 0
        desig = torch.where(masked, torch.zeros_like(desig), desig)
    if weighted:
        u = torch.randn(64, generator=torch.Generator().manual_seed(1234), dtype=torch.float64)
        u /= u.norm()
        K, kn, q = K - (K @ u)[..., None] * u, kn - (kn @ u)[..., None] * u, q - (q @ u)[..., None] * u
        for s in range(S):
            for h in range(H):
                j = int(desig[s, h])
                if j == slot:
                    kn[s, h] = 8.0 * u
                else:
                    K[4 * (s // 4):4 * (s // 4) + 4, h, j] = 8.0 * u   # whichever row of the group the table points at
        _, _, _, P = decode_forward(q, kn, vn, K, torch.zeros_like(V), step, src, kmask, torch.float64)
        # q . u = 0 so far: the designated key scores 0; log(sum of the others' exp(score)) = log((1 - P_d) / P_d)
        pd = P.gather(2, desig[:, :, None])[..., 0].clamp(min=1e-300)
        a = torch.log((1.0 - pd) / pd)
        a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
        q = q + (torch.full_like(a, 60.0) if weighted.startswith("big") else a)[..., None] * u
    K[:, :, slot:], V[:, :, slot:] = math.nan, math.nan
    c16 = (lambda t: rnd16(t.float(), kv16)) if kv16 is not None else (lambda t: t.float())
    return {"q": q.float(), "kn": kn.float(), "vn": vn.float(), "K": c16(K), "V": c16(V), "step": step, "src": src, "kmask": kmask,
            "desig": desig, "S": S, "H": H, "slots": slots, "nkeys": nkeys}


def frag_off(row: int, k: int, Kdim: int) -> int:
    """Offset of element (row, k) in the fragment-major activation layout of the fused decode plan (frag_off of csrc/common.h; the layout is
    stated in csrc/skinny_direct.inc), which attn_decode_kernel (csrc/attn_decode.hip) writes with frag_out."""
    return ((((row >> 5) * 2 + ((row >> 4) & 1)) * (Kdim >> 4) + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + (row & 15)) * 4 + (k & 3)
