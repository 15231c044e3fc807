"""Reference side of the opt-in e4m3 K/V cache (rgrg_decoder_set_kv_format, csrc/attn_kv8.hip).  TEST INFRASTRUCTURE ONLY.

The format: plain OCP e4m3fn bytes, no scales.  fp32 -> e4m3 is a clamp to +-448 in fp32 followed by ONE rounding to nearest even
(torch.float8_e4m3fn's CPU conversion rounds that way; without the clamp it returns NaN from 480 up).  Where the path rounds:
the new token's k / v before they take part as the last key and are stored, the image key / value of slot 0, nothing else - the
scores, the softmax and the accumulation are fp32, the output is rounded to the autocast type when it goes to out16.
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch
import torch.nn.functional as F

import attn_reference as R

Tensor = torch.Tensor
E4M3_MAX = 448.0
KV8_CHUNK = 144   # keys of a full chunk of attn_decode_kv8_wave_kernel; the tail advances in steps of 16
KV8_STEP = 16


def rnd8(x: Tensor) -> Tensor:
    """Clamp to +-448, round once to e4m3 (nearest even), widen back to x's dtype."""
    return x.to(torch.float32).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).to(x.dtype)


def to_bytes(x: Tensor) -> Tensor:
    """Values -> the uint8 tensor of e4m3 bytes the kernel reads (clamp + one rounding; exact for representable values)."""
    return x.to(torch.float32).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def from_bytes(b: Tensor) -> Tensor:
    return b.view(torch.float8_e4m3fn).to(torch.float32)


def rnd8_via16(x: Tensor, fp16) -> Tensor:
    """The WRONG conversion the tests must tell apart: through the 16-bit type first (double rounding)."""
    return rnd8(R.rnd16(x, fp16))


def decode_forward_kv8(q: Tensor, kn: Tensor, vn: Tensor, K: Tensor, V: Tensor, step: int, src: Optional[Tensor], dt, *,
                       out16=None, new_kv: str = "rnd8", mut: Optional[str] = None, mut_col: int = 1, chunk: int = KV8_CHUNK):
    """attn_reference.decode_forward for an e4m3 cache: K / V are the exact widening of the cache bytes, the new token's k / v are
    rounded with rnd8 before they take part (new_kv: "rnd8"; "raw" and "via_bf16" are the wrong evaluations of the power tests),
    out16 (None / 0 bf16 / 1 fp16): the output is rounded to that type.  Returns (out, k stored, v stored, P)."""
    if new_kv == "rnd8":
        kn, vn = rnd8(kn), rnd8(vn)
    elif new_kv == "via_bf16":
        kn, vn = rnd8_via16(kn, 0), rnd8_via16(vn, 0)
    else:
        assert new_kv == "raw"
    out, k, v, P = R.decode_forward(q, kn, vn, K, V, step, src, None, dt, kv16=None, out16=False, mut=mut, mut_col=mut_col, chunk=chunk)
    if out16 is not None:
        out = R.rnd16(out, out16)
    return out, k, v, P


def decode_inputs_kv8(S: int, H: int, nkeys: int, slots: int, seed: int, with_src: bool = False, weighted: Optional[str] = "half",
                      tile: int = KV8_CHUNK, offset: int = 0, desig_all: Optional[int] = None, edge_values="small"):
    """attn_reference.decode_inputs with the cache rounded to e4m3 (K / V hold exactly representable values; slots >= nkeys - 1 stay
    NaN = byte 0x7F).  edge_values: head 0 of the new token's k / v carries the conversion's edge cases - "small": ties, subnormals,
    below half the smallest subnormal, -0, a value that rounds differently through bf16; "large": also beyond +-448; None: none."""
    d = R.decode_inputs(S, H, nkeys, slots, seed, with_src, None, None, weighted, tile, offset, desig_all)
    d["K"], d["V"] = rnd8(d["K"]), rnd8(d["V"])
    small = torch.tensor([1.0625, 1.1875, -0.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, -(2.0 ** -10) * 1.0001, 2.0 ** -6 + 2.0 ** -10])
    if edge_values:
        # 14.53: 15 directly, 14 through bf16 (14.5, a tie)
        d["vn"][:, 0, :9] = torch.cat((small, torch.tensor([14.53])))
        if not (d["desig"][:, 0] == d["step"] + 1).any():
            d["kn"][:, 0, 48:56] = small   # the key path: only the edge cases of N(0,1) size, so that the designated weights stay put
    if edge_values == "large":   # the value path only: any magnitude is harmless to the softmax, but it coarsens a 16-bit output's floor
        d["vn"][:, 0, 16:24] = torch.tensor([500.0, -1e6, 448.0, 464.0, -480.0, 17.0, 19.0, 272.5])
    return d


@contextlib.contextmanager
def e4m3_cache_oracle(via16: bool = False):
    """For its duration oracle.language_model.pseudo_attention is a restatement in which k, v and the image key / value are rnd8 of
    their fp32 values in place of _r16 (via16: rnd8 of the 16-bit rounding - the other legitimate-looking evaluation, for the
    spread measurement).  Everything else - 16-bit GEMM operands, fp32 scores / softmax / accumulation - is the oracle's."""
    from oracle import language_model as o

    def patched(sd, p, x, img, add_mask, past, drop_probs=None, drop_out=None, bf16=False):
        assert bf16, "the e4m3 cache exists only in a 16-bit precision mode"
        r = (lambda t: rnd8_via16(t, 1 if bf16 == 2 else 0)) if via16 else rnd8
        q, k, v = o.conv1d(sd, p + "c_attn.", x, bf16).split(o.D_MODEL, dim=2)
        k, v = r(k), r(v)
        if past is None:
            k_img = r(F.linear(img[:, None, :], sd[p + "uk.weight"], sd[p + "uk.bias"]))
            v_img = r(F.linear(img[:, None, :], sd[p + "uv.weight"], sd[p + "uv.bias"]))
            K = o._heads(torch.cat((k_img, k), dim=1))
            V = o._heads(torch.cat((v_img, v), dim=1))
        else:
            K = torch.cat((past[0], o._heads(k)), dim=-2)
            V = torch.cat((past[1], o._heads(v)), dim=-2)
        Q = o._heads(q)
        w = torch.matmul(Q, K.transpose(-1, -2)) / (o.HEAD_DIM ** 0.5)
        ql, kl = Q.shape[-2], K.shape[-2]
        causal = torch.tril(torch.ones((kl, kl), dtype=torch.bool))[kl - ql:kl, :kl]
        w = torch.where(causal, w, torch.tensor(o.MASK_VALUE, dtype=w.dtype))
        w = F.softmax(w + add_mask, dim=-1)
        if drop_probs is not None:
            w = w * drop_probs
        a = o.conv1d(sd, p + "c_proj.", torch.matmul(w, V).permute(0, 2, 1, 3).reshape(x.shape[0], ql, o.D_MODEL), bf16)
        if drop_out is not None:
            a = a * drop_out.view_as(a)
        return a, (K, V)

    keep = o.pseudo_attention
    o.pseudo_attention = patched
    try:
        yield
    finally:
        o.pseudo_attention = keep


# The cases of tests/test_gpu_kv8_kernel.py (the power tests of tests/test_kv8_reference.py aim their mutations at the same shapes).
# both sides of every 16-key tail boundary below one chunk (16 .. 144) AND behind a full chunk (160 .. 288: the FIRST = false
# instantiations of every tail size), the 144-key chunk boundary itself, and the second chunk boundary (288 / 289)
KV8_NKEYS = (2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 143, 144, 145, 146, 160, 161, 176, 177, 192, 193,
             208, 209, 224, 225, 240, 241, 256, 257, 272, 273, 288, 289, 300)
# (S, ancestor table, out16: None fp32 / 0 bf16 / 1 fp16, weighting).  The last one is plain N(0,1): with half of the softmax on one
# key and few keys the remaining scores are (nearly) equal and a wrong score SCALE would not show - it does on unequal scores.
KV8_VARIANTS = ((33, False, None, "half"), (33, True, 0, "half"), (5, True, None, "half"), (5, False, 0, "half"), (3, False, 1, "half"),
                (3, True, 1, "half"), (3, False, None, None))
KV8_PLAIN = 6   # index of the plain variant
KV8_BIG = (("big_first", 146), ("big_last", 146), ("big_first", 289), ("big_last", 289), ("big_last", 33), ("big_last", 145))


def kv8_case(nkeys: int, ci: int):
    """The inputs of variant ``ci`` of tests/test_gpu_kv8_kernel.py::test_attn_decode_kv8 at ``nkeys`` keys.  The designated keys cycle
    through key 0, the new token's slot and both sides of every multiple of 16 - every tail boundary and, at 144 and 288, the chunk
    boundaries."""
    S, with_src, out16, weighted = KV8_VARIANTS[ci]
    return decode_inputs_kv8(S, 16, nkeys, nkeys + ci % 3, 1000 * nkeys + ci, with_src, weighted, KV8_STEP, offset=ci)
