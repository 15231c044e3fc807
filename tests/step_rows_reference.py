"""Plain torch restatements of the kernels that start a decode step and of the bookkeeping kernels between steps (embedding +
LayerNorm, the cache writes of the image slot and of a prompt, positions, masks, ancestor tables: rgrg_amd/csrc/decoder.hip,
decoder_lm.hip, decoder_prompt.hip, decoder_beam.hip), the inputs the per-kernel tests share and the tables of mutations they must
reject.  TEST INFRASTRUCTURE ONLY.  Number formats, compare and MARGIN come from attn_reference; judge, compare16, layer_norm and ROWS
from train_rows_reference; the e4m3 rounding from kv8_reference.

Every evaluation is ``ev(case, dt, mut=None) -> {name: tensor}`` with ``dt`` torch.float64 for the reference and torch.float32 for the
noise measurement; ``mut`` applies one named mutation (tests/test_step_rows_reference.py: each must be rejected with the bounds used on
the GPU).  A LayerNorm output that the kernel stores as 16 bit is returned UNROUNDED (kind "h16": the judge rounds where it has to).
An output that is a copy, a rounding of an fp32 input, an index or a mask is returned as the kernel stores it - fp32 values, int16
bit patterns of the 16-bit type, e4m3 bytes, integers - in the WHOLE buffer the launch sees, sentinels in front of, between and behind
the written elements included (kind "exact"), so one comparison covers every element the kernel must write and every one it must not.

Bounds (none comes from the code under test):
  "f32"    attn_reference.compare: MARGIN * max|ref32 - ref64| + 2^-23 max|ref|
  "h16"    train_rows_reference.compare16: per element, half an ulp of the 16-bit type on top of MARGIN * noise
  "exact"  equality of the stored values

The rules restated here, with the lines of the reference's src/language_model/language_model.py the kernels' own comments give:
  positions are embedded with the TOKEN table: wte(input_ids) + wte(position_ids), default arange(past, past + T)     :291-310
  a given position_ids [1,T] broadcasts over the sentences                                                             :294-310
  additive key mask (1 - [1 | attention_mask]) * -1e4: a ones column in front, the image slot is never masked          :316-334
  position_ids of a padded prompt = cumsum(mask) - 1, masked_fill(mask == 0, 1)                                        :506-509
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional

import torch
import torch.nn.functional as F  # noqa: F401  (the CPU self-test's independent formulations import it from here)

import kv8_reference as KV8
import train_rows_reference as T
from attn_reference import MARGIN, compare, from_bits, rnd16, to_bits  # noqa: F401
from train_rows_reference import ROWS, compare16, judge, layer_norm  # noqa: F401

Tensor = torch.Tensor
F64, F32 = torch.float64, torch.float32
D, H = 1024, 16
V_SMALL = 40
LN_EPS = T.LN_EPS
MASK_VALUE = -1e4
BOS_ID = PAD_ID = 50256
SENT, SENT16, SENT8, SENTI = -777.25, 0x7B7B, 0x7B, -12345   # fp32 / 16-bit pattern (finite in both types) / e4m3 byte / integers
GUARD = 256                                                  # sentinel elements in front of and behind a flat buffer
MASK_ROW_EMPTY, MASK_NOT_LEFT, MASK_HAS_PAD, MASK_NOT_BINARY = 1, 2, 4, 8


# ------------------------------------------------------------------------------------------------ buffers and number formats
def sentinel(dtype):
    return {torch.float32: SENT, torch.int16: SENT16, torch.uint8: SENT8, torch.int32: SENTI, torch.int64: SENTI}[dtype]


def guarded(rows: int, cols: int, dtype) -> Tensor:
    """[1 + rows + 1, cols] of the dtype's sentinel: the launch gets the address of row 1, rows 0 and rows + 1 must stay."""
    return torch.full((rows + 2, cols), sentinel(dtype), dtype=dtype)


def guarded_flat(n: int, dtype) -> Tensor:
    """[GUARD + n + GUARD] of the dtype's sentinel: the launch gets the address of element GUARD."""
    return torch.full((n + 2 * GUARD,), sentinel(dtype), dtype=dtype)


def store_dtype(fmt):
    """fmt: None fp32, 0 bf16, 1 fp16, "e4m3"."""
    return torch.float32 if fmt is None else torch.uint8 if fmt == "e4m3" else torch.int16


def trunc16_bits(x: Tensor, fp16) -> Tensor:
    """The WRONG 16-bit store: rounded toward zero."""
    x = x.float()
    if not fp16:
        return (x.view(torch.int32) >> 16).to(torch.int16)
    h = x.to(torch.float16)
    over = h.float().abs() > x.abs()
    return (h.view(torch.int16).to(torch.int32) - over.to(torch.int32)).to(torch.int16)   # one step toward zero in either sign


def store_bits(x: Tensor, fmt, mut: Optional[str] = None) -> Tensor:
    """fp32 values as a cache plane or a 16-bit activation row stores them: the value (fp32), ONE rounding to nearest even (int16 bit
    patterns), or the clamp to +-448 and one rounding to e4m3 (bytes)."""
    x = x.float()
    if fmt is None:
        return x
    if fmt == "e4m3":
        return KV8.to_bytes(rnd16(x, 0)) if mut == "e4m3_via_bf16" else KV8.to_bytes(x)
    return trunc16_bits(x, fmt) if mut == "truncate16" else to_bits(x, fmt)


def as_kernel(ev: Dict[str, Tensor], kinds: Dict[str, str], fp16, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """What a kernel that computed ``ev`` would store (train_rows_reference.as_kernel); mut == "truncate16": its 16-bit LayerNorm
    outputs rounded toward zero."""
    out = T.as_kernel(ev, kinds, fp16)
    if mut == "truncate16":
        for k, kind in kinds.items():
            if kind == "h16":
                out[k] = from_bits(trunc16_bits(ev[k].float(), fp16), fp16)
    return out


def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k) + 1
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln(x: Tensor, g: Tensor, b: Tensor, dt, mut: Optional[str] = None) -> Tensor:
    """nn.LayerNorm(1024, eps=1e-5): two-pass, variance over n (train_rows_reference.layer_norm) - or one of its two mutations."""
    if mut not in ("unbiased_variance", "missing_eps"):
        return layer_norm(x, g, b, dt)
    x = x.to(dt)
    c = x - x.mean(dim=-1, keepdim=True)
    var = (c * c).sum(dim=-1, keepdim=True) / (x.shape[-1] - 1 if mut == "unbiased_variance" else x.shape[-1])
    return c / torch.sqrt(var if mut == "missing_eps" else var + LN_EPS) * g.to(dt) + b.to(dt)


def ln_rows(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    return {"xn" if c["fp16"] is None else "xn16": ln(c["x"], c["g"], c["b"], dt, mut)}


def ln_rows_kinds(c):
    return {"xn": "f32"} if c["fp16"] is None else {"xn16": "h16"}


LN_INPUTS = ("n01", "mean30", "tiny", "const")


def ln_rows_cases(rows: int):
    """N(0,1); mean +-30 with std 0.5 (a one-pass variance would cancel); std 1e-3 around +-0.25 (the eps under the root is ten times
    the variance); constant rows of a small integer, row 0 of 3.0: every partial sum is exact in any order, x - mean is 0 and the
    output is b.  The two rows with a large mean are multiples of 2^-9 / 2^-15: their row sum (< 2^15 / 2^9) is exact in fp32 in any
    order, so the mean and x - mean are exact in every correct implementation.  Otherwise ONE rounding of the mean, 2^-20 / 0.5 or
    2^-26 / 1e-3 of every output whichever way it falls, would decide the error of the kernel and the noise of the float32
    evaluation alike, and a one-row case would compare two draws of it."""
    for kind in LN_INPUTS:
        gen = _gen(11, rows, LN_INPUTS.index(kind))
        if kind == "const":
            x = (((torch.arange(rows) + 2) % 5) + 1).float()[:, None].expand(rows, D).contiguous()
        else:
            mean, std = {"n01": (0.0, 1.0), "mean30": (30.0, 0.5), "tiny": (0.25, 1e-3)}[kind]
            x = T._rows(gen, rows, mean, std)
            if kind != "n01":
                q = 2.0 ** (-9 if kind == "mean30" else -15)
                x = torch.round(x / q) * q
        g, b = T._gain(gen)
        for fp16 in (None, 0, 1):
            yield {"name": f"rows={rows},x={kind},out={'f32' if fp16 is None else ('bf16', 'fp16')[fp16]}", "rows": rows, "kind": kind, "fp16": fp16,
                   "x": x, "g": g, "b": b}


# ------------------------------------------------------------------------------------------------ embedding + LayerNorm of a step
def table(seed: int = 5) -> Tensor:
    """wte [V_SMALL][1024], every row with its own mean so that a wrong row shows in the row statistics as well."""
    gen = _gen(3, seed)
    return torch.randn(V_SMALL, D, generator=gen) + 0.05 * torch.arange(V_SMALL).float()[:, None]


def embed_ln(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """x = wte[token] + wte[position] - ONE fp32 addition per element, so it is formed in fp32 whatever dt - then, by mode: xn fp32,
    xn16, or the raw row as 16 bit ("x16", the bits) with (sum, sum of squares) in slot 0 of the row's 16 slots and zeros behind."""
    S, step = c["S"], c["step"]
    tok = c["ids"][:S, step] if c["tok"] is None or mut == "token_from_ids" else c["tok"].long()
    pos = torch.full((S,), step) if c["pos"] is None or mut == "position_from_step" else c["pos"].long()
    x = c["wte"][tok] + c["wte"][pos]
    out = {"x": x}
    if c["mode"] == "stats":
        xs = x.to(dt)
        if mut == "stats_centred":
            xs = xs - xs.mean(dim=-1, keepdim=True)
        out["x16"] = store_bits(x, c["fp16"], mut)
        out["stats0"] = torch.stack((xs.sum(dim=-1), (xs * xs).sum(dim=-1)), dim=-1)
        out["stats_rest"] = torch.full((S, 15, 2), SENT if mut == "stats_rest_not_zeroed" else 0.0)
    else:
        out[c["mode"]] = ln(x, c["g"], c["b"], dt, mut)
    return out


def embed_ln_kinds(c):
    if c["mode"] == "stats":
        return {"x": "exact", "x16": "exact", "stats0": "f32", "stats_rest": "exact"}
    return {"x": "exact", c["mode"]: "f32" if c["mode"] == "xn" else "h16"}


def embed_ln_cases(S: int):
    """The id buffer is [S][9] with *step = 3; the override tokens and positions differ from ids[s][3] and from 3 in every row."""
    wte = table()
    for mode, types in (("xn", (None,)), ("xn16", (0, 1)), ("stats", (0, 1))):
        for fp16 in types:
            for with_tok in (0, 1):
                for with_pos in (0, 1):
                    gen = _gen(17, S, ("xn", "xn16", "stats").index(mode), fp16 or 0, with_tok, with_pos)
                    ids = torch.randint(0, V_SMALL, (S, 9), generator=gen)
                    tok = ((ids[:, 3] + 1 + torch.randint(0, V_SMALL - 1, (S,), generator=gen)) % V_SMALL).to(torch.int32)
                    pos = (4 + torch.randint(0, V_SMALL - 4, (S,), generator=gen)).to(torch.int32)
                    g, b = T._gain(gen)
                    yield {"name": f"S={S},mode={mode},fp16={fp16},tok={with_tok},pos={with_pos}", "S": S, "mode": mode, "fp16": fp16, "wte": wte,
                           "ids": ids, "ld_ids": 9, "step": 3, "tok": tok if with_tok else None, "pos": pos if with_pos else None, "g": g, "b": b}


# ------------------------------------------------------------------------------------------------ embedding + LayerNorm of S x T rows
def clamp_ids(ids: Tensor, V: int):
    """(ids clamped into [0, V): negative -> 0, else V - 1; whether any was outside)."""
    return ids.clamp(0, V - 1), bool(((ids < 0) | (ids >= V)).any())


def embed_seq_ln(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    S, Tn, V = c["S"], c["T"], V_SMALL
    tok, bad = clamp_ids(c["ids"], V)
    if c["pos_ids"] is None:
        pos, bad_pos = torch.arange(Tn)[None, :].expand(S, Tn), False
    else:
        pos, bad_pos = clamp_ids(c["pos_ids"], V)
        if pos.shape[0] == 1:   # [1,T]: every sentence takes the same positions (:294-310)
            pos = torch.cat((pos, torch.arange(Tn)[None, :].expand(S - 1, Tn))) if mut == "pos_not_broadcast" else pos.expand(S, Tn)
    x = (c["wte"][tok] + c["wte"][pos]).reshape(S * Tn, D)
    return {"x": x, "xn": ln(x, c["g"], c["b"], dt, mut), "id_error": torch.tensor([c["id_error"] | int(bad or bad_pos)], dtype=torch.int32)}


EMBED_SEQ_KINDS = {"x": "exact", "xn": "f32", "id_error": "exact"}
OUTSIDE = (-7, V_SMALL, 2 ** 40)


def embed_seq_cases():
    wte = table()
    for S, Tn in ((2, 3), (3, 5)):
        for pos_kind in ("none", "ST", "1T"):
            for dirty in ("clean0", "clean2", "ids", "pos"):
                if dirty == "pos" and pos_kind == "none":
                    continue
                gen = _gen(23, S, Tn, ("none", "ST", "1T").index(pos_kind), ("clean0", "clean2", "ids", "pos").index(dirty))
                ids = torch.randint(0, V_SMALL, (S, Tn), generator=gen)
                pos = None if pos_kind == "none" else 7 + torch.randint(0, V_SMALL - 7, (S if pos_kind == "ST" else 1, Tn), generator=gen)
                if dirty == "ids":
                    ids.reshape(-1)[torch.tensor([0, 2, S * Tn - 1])] = torch.tensor(OUTSIDE)
                if dirty == "pos":
                    pos.reshape(-1)[torch.tensor([0, 1, pos.numel() - 1])] = torch.tensor(OUTSIDE)
                g, b = T._gain(gen)
                yield {"name": f"S={S},T={Tn},pos={pos_kind},{dirty}", "S": S, "T": Tn, "wte": wte, "ids": ids, "pos_ids": pos, "g": g, "b": b,
                       "id_error": 2 if dirty in ("clean2", "ids") else 0, "dirty": dirty not in ("clean0", "clean2")}   # 2 | 1: OR-ed, not set


# ------------------------------------------------------------------------------------------------ cache writes
def plane_offsets(rows_idx: Tensor, slot_idx: Tensor, slots: int) -> Tensor:
    """Element offsets inside a plane [rows][H][slots][64] of (row, head, slot, e), broadcast over the index tensors; the head and
    element axes are the last two."""
    hd = torch.arange(H)[:, None]
    e = torch.arange(64)[None, :]
    return ((rows_idx[..., None, None] * H + hd) * slots + slot_idx[..., None, None]) * 64 + e


def kv_slot0(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """ukv [S][ld], column (l * 2 + kv) * D + d -> slot 0 of cache row s * row_mul, plane kv of layer l."""
    L, S, slots = c["L"], c["S"], c["slots"]
    rm = 1 if mut == "row_mul_ignored" else c["row_mul"]
    buf = guarded_flat(c["n"], store_dtype(c["fmt"]))
    v = store_bits(c["ukv"][:, :L * 2 * D].reshape(S, L, 2, H, 64), c["fmt"], mut)              # [s, l, kv, head, e]
    l = torch.arange(L)[None, :, None]
    kv = torch.arange(2)[None, None, :]
    if mut == "kv_swapped":
        kv = 1 - kv
    s = torch.arange(S)[:, None, None].expand(S, L, 2)
    o = GUARD + (l * c["layer_stride"] + kv * c["kv_stride"])[..., None, None] + plane_offsets(s * rm, torch.zeros_like(s), slots)
    buf[o.reshape(-1)] = v.reshape(-1)
    return {"kv": buf}


def kv_slot0_cases():
    """24 layers x 8 rows: 393 216 values for the 262 144 threads of the launch, so the stride loop runs; ld, the plane stride and the
    layer stride all larger than the data.  Row 0 carries the edge values of every format in the first head of layer 0's key."""
    L, S, slots = 24, 8, 6
    ld = L * 2 * D + 32
    ukv = torch.randn(S, ld, generator=_gen(29)) * 1.5
    edge = torch.tensor([500.0, -1e6, 448.0, 464.0, -480.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, -(2.0 ** -10) * 1.0001, -0.0, 1.0625, 1.1875,
                         14.53, 1.00390625, 1.01171875, 65520.0, 1e-8, 6e-8, 272.5, 17.0, 19.0, 3.0e38])
    ukv[0, :len(edge)] = edge
    ukv[S - 1, L * 2 * D - len(edge):L * 2 * D] = edge
    for row_mul in (1, 3):
        plane = S * row_mul * H * slots * 64
        kv_stride, layer_stride = plane + 128, 2 * plane + 128 + 64
        for fmt in (None, 0, 1, "e4m3"):
            yield {"name": f"row_mul={row_mul},fmt={fmt}", "L": L, "S": S, "slots": slots, "ld": ld, "row_mul": row_mul, "fmt": fmt, "ukv": ukv,
                   "kv_stride": kv_stride, "layer_stride": layer_stride, "n": L * layer_stride}


KV_SLOT0_KINDS = {"kv": "exact"}


def prompt_kv_store(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """The k and v thirds of qkv [S*T][3D] -> slots 1 .. T of cache row s * row_mul of the K and the V plane."""
    S, Tn, slots = c["S"], c["T"], c["slots"]
    rm = 1 if mut == "row_mul_ignored" else c["row_mul"]
    v = store_bits(c["qkv"].reshape(S, Tn, 3, H, 64)[:, :, 1:], c["fmt"], mut)                  # [s, t, kv, head, e]
    s = torch.arange(S)[:, None].expand(S, Tn)
    t = torch.arange(Tn)[None, :].expand(S, Tn)
    o = GUARD + plane_offsets(s * rm, t if mut == "slot_t" else 1 + t, slots)
    out = {}
    for i, name in enumerate(("v", "k") if mut == "kv_swapped" else ("k", "v")):
        out[name] = guarded_flat(c["n"], store_dtype(c["fmt"]))
        out[name][o.reshape(-1)] = v[:, :, i].reshape(-1)
    return out


def prompt_kv_cases(large: bool = False):
    shapes = [(8, 300, 304, 1, None)] if large else [(3, 5, 9, rm, fmt) for rm in (1, 4) for fmt in (None, 0, 1)]
    for S, Tn, slots, row_mul, fmt in shapes:
        qkv = torch.randn(S * Tn, 3 * D, generator=_gen(31, S, Tn))
        qkv[0, D:D + 4] = torch.tensor([1.00390625, 1.01171875, -0.0, 65520.0])   # bf16 ties to even (down, up), -0, fp16 overflow
        yield {"name": f"S={S},T={Tn},slots={slots},row_mul={row_mul},fmt={fmt}", "S": S, "T": Tn, "slots": slots, "row_mul": row_mul, "fmt": fmt,
               "qkv": qkv, "n": S * row_mul * H * slots * 64}


PROMPT_KV_KINDS = {"k": "exact", "v": "exact"}


def prompt_last_rows(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """Row r of the lm_head input = the last position's row of sequence r / row_div."""
    R, Tn = c["R"], c["T"]
    s = torch.arange(R) // c["row_div"]
    rows = c["xn_all"][s * Tn + (0 if mut == "first_position" else Tn - 1)]
    xn = guarded(R, D, torch.float32)
    xn[1:R + 1] = rows
    out = {"xn": xn}
    if c["fp16"] is not None:
        out["xn16"] = guarded(R, D, torch.int16)
        out["xn16"][1:R + 1] = store_bits(rows, c["fp16"], mut)
    return out


def prompt_last_kinds(c):
    return {"xn": "exact"} if c["fp16"] is None else {"xn": "exact", "xn16": "exact"}


def prompt_last_cases():
    for row_div in (1, 3):
        for fp16 in (None, 0, 1):
            Sq, Tn = 4, 3
            xn_all = torch.randn(Sq * Tn, D, generator=_gen(37, row_div))
            xn_all[Tn - 1, :3] = torch.tensor([1.00390625, 1.01171875, -0.0])
            yield {"name": f"row_div={row_div},fp16={fp16}", "R": Sq * row_div, "T": Tn, "row_div": row_div, "fp16": fp16, "xn_all": xn_all}


# ------------------------------------------------------------------------------------------------ masks and positions of a prompt
def prompt_mask_scan(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """pad[s] = the zeros in front of row s; flags = OR over the rows of: only zeros 1, a zero behind a non-zero 2, padded 4, a value
    other than 0 and 1 behind the padding 8."""
    am = c["am"]
    S, Tn = am.shape
    lead = (am != 0).cumsum(dim=1) == 0                       # still inside the zeros in front
    pad = lead.sum(dim=1) if mut != "counts_every_zero" else (am == 0).sum(dim=1)
    behind = ~lead
    f = 0
    if bool((pad == Tn).any()):
        f |= MASK_ROW_EMPTY
    if bool((pad > 0).any()):
        f |= MASK_HAS_PAD
    if bool((behind & (am == 0)).any()):
        f |= MASK_NOT_LEFT
    if bool((behind & (am != 0) & (am != 1)).any()):
        f |= MASK_NOT_BINARY
    out = guarded(S, 1, torch.int32)
    out[1:S + 1, 0] = pad.to(torch.int32)
    return {"pad": out, "flags": torch.tensor([c["flags0"] | f], dtype=torch.int32)}


MASK_SCAN_KINDS = {"pad": "exact", "flags": "exact"}
MASK_ROWS = {"ones": [1, 1, 1, 1, 1, 1, 1], "left": [0, 0, 0, 1, 1, 1, 1], "left1": [0, 1, 1, 1, 1, 1, 1], "last": [0, 0, 0, 0, 0, 0, 1],
             "zeros": [0, 0, 0, 0, 0, 0, 0], "hole": [0, 1, 1, 0, 1, 1, 1], "tail": [1, 1, 1, 1, 1, 1, 0], "half": [0, 0, 1, 0.5, 1, 1, 1]}


def mask_scan_cases():
    """257 rows = two workgroups, the last row on its own in the second; every subset of flag bits that a mask can raise; T = 1."""
    def rows(*names, S=257):
        return torch.tensor([MASK_ROWS[names[i % len(names)]] for i in range(S)], dtype=torch.float32)
    for name, am, flags0 in (("ones", rows("ones"), 0), ("left", rows("ones", "left", "left1", "last"), 0), ("mixed", rows(*MASK_ROWS), 0),
                             ("hole_only", rows("ones", "hole"), 0), ("half_last_row", torch.cat((rows("ones", S=256), rows("half", S=1))), 0),
                             ("zeros_last_row", torch.cat((rows("ones", S=256), rows("zeros", S=1))), 0), ("tail", rows("ones", "tail"), 16),
                             ("T=1,ones", torch.ones(5, 1), 0), ("T=1,zero_row", torch.tensor([[1.0], [0.0], [1.0], [1.0], [1.0]]), 0),
                             ("T=1,half", torch.tensor([[1.0], [1.0], [0.5]]), 0)):
        yield {"name": name, "am": am, "flags0": flags0}


def prompt_setup(c: dict, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """ids[s][0 .. T) = the prompt clamped into the vocabulary, *step = T - 1; with pad: pos[s][t] = cumsum(mask) - 1 = t - pad[s], 1
    where masked (:506-509); with kmask: (1 - [1 | mask | 1 ..]) * -1e4 = -1e4 on slots 1 .. pad[s], 0 on the image slot (:316-334)."""
    S, Tn, slots, ld = c["S"], c["T"], c["slots"], c["ld_ids"]
    ids = guarded(S, ld, torch.int64)
    ids[1:S + 1, :Tn] = clamp_ids(c["in"], V_SMALL)[0]
    pos, kmask = guarded(S, Tn, torch.int64), guarded(S, slots, torch.float32)
    if c["pad"] is not None:
        pad = c["pad"].long()[:, None]
        t = torch.arange(Tn)[None, :]
        mask = (t >= pad).to(dt)                                    # the left-padded attention_mask itself
        p = mask.cumsum(dim=1) - 1
        pos[1:S + 1] = torch.where(mask == 0, torch.full_like(p, 0.0 if mut == "masked_position_0" else 1.0), p).long()
        if c["kmask"]:
            full = torch.cat((torch.ones(S, 1, dtype=dt), mask, torch.ones(S, slots - 1 - Tn, dtype=dt)), dim=1)
            km = (1.0 - full) * MASK_VALUE
            kmask[1:S + 1] = (torch.roll(km, -1, dims=1) if mut == "key_mask_shifted" else km).float()
    return {"ids": ids, "step": torch.tensor([Tn if mut == "step_T" else Tn - 1], dtype=torch.int32), "pos": pos, "kmask": kmask}


PROMPT_SETUP_KINDS = {"ids": "exact", "step": "exact", "pos": "exact", "kmask": "exact"}


def prompt_setup_cases():
    """S * T below and above one workgroup, S * slots above S * T (the mask decides the grid), ids outside [0, V) in the first, a middle
    and the last element; pad 0, 1, T - 1 and in between."""
    for S, Tn, slots in ((3, 5, 9), (37, 11, 13)):
        for with_pad, with_kmask in ((0, 0), (1, 0), (1, 1)):
            gen = _gen(41, S, Tn, with_pad, with_kmask)
            inp = torch.randint(0, V_SMALL, (S, Tn), generator=gen)
            inp.reshape(-1)[torch.tensor([0, S * Tn // 2, S * Tn - 1])] = torch.tensor(OUTSIDE)
            pad = torch.randint(0, Tn, (S,), generator=gen).to(torch.int32)
            pad[:3] = torch.tensor([0, 1, Tn - 1], dtype=torch.int32)
            yield {"name": f"S={S},T={Tn},slots={slots},pad={with_pad},kmask={with_kmask}", "S": S, "T": Tn, "slots": slots, "ld_ids": Tn + 3,
                   "in": inp, "pad": pad if with_pad else None, "kmask": bool(with_kmask)}


# ------------------------------------------------------------------------------------------------ index kernels
def _col(v: Tensor, dtype=torch.int32) -> Tensor:
    out = guarded(v.shape[0], 1, dtype)
    out[1:-1, 0] = v.to(dtype)
    return out


def prompt_step_rows(c, dt, mut=None):
    step = c["step"]
    return {"tok": _col(c["ids"][:, step]), "row_pos": _col(step - (0 if mut == "pad_ignored" else 1) * c["pad"])}


def beam_row_pos(c, dt, mut=None):
    return {"row_pos": _col(c["step"] - (0 if mut == "pad_ignored" else 1) * c["pad"])}


def beam_prompt_init(c, dt, mut=None):
    """Slots 0 .. T of both tables -> the item's first row; beam_pad = the item's padding."""
    R, nb, Tn, slots = c["R"], c["nb"], c["T"], c["slots"]
    src = guarded(R, slots, torch.int32)
    r = torch.arange(R)
    src[1:R + 1, :Tn + 1] = ((r if mut == "own_row" else (r // nb) * nb)[:, None]).to(torch.int32)
    pad = torch.zeros(R, dtype=torch.int32) if c["pad"] is None else c["pad"][r // nb]
    return {"src_a": src, "src_b": src.clone(), "beam_pad": _col(pad)}


def beam_init(c, dt, mut=None):
    R, nb = c["R"], c["nb"]
    src = guarded(R, c["T"], torch.int32)
    r = torch.arange(R)
    src[1:R + 1, 0] = (r if mut == "own_row" else (r // nb) * nb).to(torch.int32)
    return {"src": src, "step": torch.zeros(1, dtype=torch.int32)}


def slot_mask(first: Tensor, slots: int, dt, mut=None) -> Tensor:
    """-1e4 on slots 1 .. first[r], 0 on the image slot and behind."""
    j = torch.arange(slots)[None, :]
    lo = 0 if mut == "key_mask_shifted" else 1
    f = first.long()[:, None]
    return torch.where((j >= lo) & (j <= f - 1 + lo), torch.tensor(MASK_VALUE, dtype=dt), torch.zeros((), dtype=dt))


def beam_first_mask(c, dt, mut=None):
    km = guarded(c["R"], c["slots"], torch.float32)
    km[1:-1] = slot_mask(c["first"], c["slots"], dt, mut).float()
    return {"kmask": km}


def key_mask(c, dt, mut=None):
    """(1 - [1 | attention_mask]) * -1e4 on slots 0 .. L, 0 behind (:316-334)."""
    S, L, slots = c["S"], c["L"], c["slots"]
    full = torch.cat((torch.ones(S, 1, dtype=dt), c["am"].to(dt), torch.ones(S, slots - 1 - L, dtype=dt)), dim=1)
    if mut == "image_slot_masked":
        full = torch.cat((c["am"].to(dt), torch.ones(S, slots - L, dtype=dt)), dim=1)
    km = guarded(S, slots, torch.float32)
    km[1:-1] = ((1.0 - full) * MASK_VALUE).float()
    return {"kmask": km}


def forward_cached_tokens(c, dt, mut=None):
    j = 0 if mut == "column_0" else c["j"]
    out = {"tok": _col(clamp_ids(c["ids"][:, j], V_SMALL)[0]), "step": torch.tensor([c["position"]], dtype=torch.int32)}
    out["row_pos"] = _col(clamp_ids(c["pos_ids"][:, j], V_SMALL)[0]) if c["pos_ids"] is not None else guarded(c["S"], 1, torch.int32)
    return out


def decode_reset(c, dt, mut=None):
    S, L, ld = c["S"], c["L"], c["ld_ids"]
    ids = guarded(S, ld, torch.int64)
    if mut == "ld_ignored":
        ids[1:S + 1].reshape(-1)[:S * L] = PAD_ID
    else:
        ids[1:S + 1, :L] = PAD_ID
        ids[1:S + 1, 0] = BOS_ID
    return {"ids": ids, "finished": _col(torch.zeros(S)), "step": torch.zeros(1, dtype=torch.int32), "done_len": torch.zeros(1, dtype=torch.int32),
            "sync": torch.zeros(2, dtype=torch.int32)}


def beam_advance(c, dt, mut=None):
    """Row r continues beam parent[r]: slots 0 .. t from the parent's table, slot t + 1 (written this step) lives in the parent's row."""
    R, Tn, t = c["R"], c["T"], c["step"]
    p = c["parent"].long()
    new = guarded(R, Tn, torch.int32)
    new[1:R + 1, :t + 1] = c["src_old"][torch.arange(R) if mut == "own_history" else p, :t + 1]
    new[1:R + 1, t + 1] = (torch.arange(R) if mut == "slot_own_row" else p).to(torch.int32)
    return {"src_new": new, "src_old": c["src_old"], "step": torch.tensor([t], dtype=torch.int32)}


def _exact(*names):
    return {n: "exact" for n in names}


RS = (5, 300)   # one-thread-per-row kernels: inside one workgroup, and across two


def step_rows_cases():
    for S in RS:
        gen = _gen(43, S)
        yield {"name": f"S={S}", "S": S, "ld_ids": 12, "step": 4, "ids": torch.randint(0, V_SMALL, (S, 12), generator=gen),
               "pad": torch.randint(0, 5, (S,), generator=gen).to(torch.int32)}


def beam_row_pos_cases():
    for R in RS:
        yield {"name": f"R={R}", "R": R, "step": 9, "pad": torch.randint(0, 9, (R,), generator=_gen(47, R)).to(torch.int32)}


def beam_prompt_init_cases():
    for R, nb in ((6, 3), (300, 4)):
        for with_pad in (0, 1):
            pad = torch.randint(1, 4, (R // nb,), generator=_gen(53, R)).to(torch.int32)
            yield {"name": f"R={R},nb={nb},pad={with_pad}", "R": R, "nb": nb, "T": 4, "slots": 8, "pad": pad if with_pad else None}


def beam_init_cases():
    for R, nb in ((5, 5), (300, 3)):
        yield {"name": f"R={R},nb={nb}", "R": R, "nb": nb, "T": 7}


def beam_first_mask_cases():
    for R in RS:
        first = torch.randint(0, 7, (R,), generator=_gen(59, R)).to(torch.int32)
        first[:2] = torch.tensor([0, 6], dtype=torch.int32)
        yield {"name": f"R={R}", "R": R, "slots": 9, "first": first}


def key_mask_cases():
    for S in RS:
        am = (torch.rand(S, 6, generator=_gen(61, S)) < 0.6).float()
        am[0], am[1] = 1.0, 0.0
        yield {"name": f"S={S}", "S": S, "L": 6, "slots": 11, "am": am}


def forward_cached_cases():
    for S in RS:
        for with_pos in (0, 1):
            gen = _gen(67, S, with_pos)
            ids, pos = torch.randint(0, V_SMALL, (S, 4), generator=gen), torch.randint(0, V_SMALL, (S, 4), generator=gen)
            ids[:3, 2] = torch.tensor(OUTSIDE)
            pos[S - 3:, 2] = torch.tensor(OUTSIDE)
            yield {"name": f"S={S},pos={with_pos}", "S": S, "T": 4, "j": 2, "position": 17, "ids": ids, "pos_ids": pos if with_pos else None}


def decode_reset_cases():
    """300 x 142 ids for the 64 x 256 threads of the launch, 300 rows for the 256-thread loop over `finished`."""
    yield {"name": "S=300,L=142", "S": 300, "L": 142, "ld_ids": 150}
    yield {"name": "S=5,L=142", "S": 5, "L": 142, "ld_ids": 150}


def beam_advance_cases():
    """A table of 300 slots; step 260 runs the 256-thread copy loop twice.  Parents: a repeat (0, 0), a fixed point (row 2), a swap."""
    R, Tn = 6, 300
    src_old = torch.randint(0, R, (R, Tn), generator=_gen(71)).to(torch.int32)
    for step in (0, 3, 260):
        yield {"name": f"step={step}", "R": R, "T": Tn, "step": step, "src_old": src_old, "parent": torch.tensor([0, 0, 2, 5, 1, 3], dtype=torch.int32)}


# ------------------------------------------------------------------------------------------------ the table of everything
class Kernel(NamedTuple):
    cases: Callable          # () -> iterable of cases
    ev: Callable             # (case, dt, mut) -> outputs
    kinds: object            # {name: kind}, or case -> that
    mutations: Dict[str, Callable]   # name -> (case -> does the mutation change this case's outputs?)


def _always(c):
    return True


def _all_rows(fn):
    return lambda: (c for rows in ROWS for c in fn(rows))


_16 = lambda c: c["fmt"] in (0, 1)   # noqa: E731

KERNELS: Dict[str, Kernel] = {
    "ln_rows": Kernel(_all_rows(ln_rows_cases), ln_rows, ln_rows_kinds,
                      {"unbiased_variance": lambda c: c["kind"] != "const", "missing_eps": lambda c: c["kind"] in ("tiny", "const"),
                       "truncate16": lambda c: c["fp16"] is not None}),
    "embed_ln": Kernel(lambda: (c for S in (1, 5) for c in embed_ln_cases(S)), embed_ln, embed_ln_kinds,
                       {"position_from_step": lambda c: c["pos"] is not None, "token_from_ids": lambda c: c["tok"] is not None,
                        "unbiased_variance": lambda c: c["mode"] != "stats", "stats_centred": lambda c: c["mode"] == "stats",
                        "stats_rest_not_zeroed": lambda c: c["mode"] == "stats", "truncate16": lambda c: c["mode"] != "xn"}),
    "embed_seq_ln": Kernel(embed_seq_cases, embed_seq_ln, EMBED_SEQ_KINDS,
                           {"pos_not_broadcast": lambda c: c["pos_ids"] is not None and c["pos_ids"].shape[0] == 1, "unbiased_variance": _always}),
    "kv_slot0": Kernel(kv_slot0_cases, kv_slot0, KV_SLOT0_KINDS,
                       {"kv_swapped": _always, "row_mul_ignored": lambda c: c["row_mul"] > 1, "truncate16": _16,
                        "e4m3_via_bf16": lambda c: c["fmt"] == "e4m3"}),
    "prompt_kv_store": Kernel(prompt_kv_cases, prompt_kv_store, PROMPT_KV_KINDS,
                              {"kv_swapped": _always, "slot_t": _always, "row_mul_ignored": lambda c: c["row_mul"] > 1, "truncate16": _16}),
    "prompt_last_rows": Kernel(prompt_last_cases, prompt_last_rows, prompt_last_kinds,
                               {"first_position": _always, "truncate16": lambda c: c["fp16"] is not None}),
    "prompt_mask_scan": Kernel(mask_scan_cases, prompt_mask_scan, MASK_SCAN_KINDS,
                               {"counts_every_zero": lambda c: c["name"] in ("mixed", "hole_only", "tail")}),
    "prompt_setup": Kernel(prompt_setup_cases, prompt_setup, PROMPT_SETUP_KINDS,
                           {"masked_position_0": lambda c: c["pad"] is not None, "key_mask_shifted": lambda c: c["kmask"], "step_T": _always}),
    "prompt_step_rows": Kernel(step_rows_cases, prompt_step_rows, _exact("tok", "row_pos"), {"pad_ignored": _always}),
    "beam_row_pos": Kernel(beam_row_pos_cases, beam_row_pos, _exact("row_pos"), {"pad_ignored": _always}),
    "beam_prompt_init": Kernel(beam_prompt_init_cases, beam_prompt_init, _exact("src_a", "src_b", "beam_pad"), {"own_row": _always}),
    "beam_init": Kernel(beam_init_cases, beam_init, _exact("src", "step"), {"own_row": _always}),
    "beam_first_mask": Kernel(beam_first_mask_cases, beam_first_mask, _exact("kmask"), {"key_mask_shifted": _always}),
    "key_mask": Kernel(key_mask_cases, key_mask, _exact("kmask"), {"image_slot_masked": _always}),
    "forward_cached_tokens": Kernel(forward_cached_cases, forward_cached_tokens, _exact("tok", "row_pos", "step"), {"column_0": _always}),
    "decode_reset": Kernel(decode_reset_cases, decode_reset, _exact("ids", "finished", "step", "done_len", "sync"), {"ld_ignored": _always}),
    "beam_advance": Kernel(beam_advance_cases, beam_advance, _exact("src_new", "src_old", "step"), {"slot_own_row": _always, "own_history": _always}),
}
MUTATIONS = {k: tuple(v.mutations) for k, v in KERNELS.items()}


def kinds_of(kernel: str, c: dict) -> Dict[str, str]:
    k = KERNELS[kernel].kinds
    return k(c) if callable(k) else k


def fp16_of(c: dict):
    """The 16-bit type of the case's "h16" outputs (None when it has none)."""
    return c.get("fp16")
