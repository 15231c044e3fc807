"""The reference of tests/step_rows_reference.py and the bounds of tests/test_gpu_step_rows.py, checked without a GPU:
  * every restatement equals an independent formulation: float64 F.layer_norm and F.embedding to 1e-12 relative, an explicit Python
    loop over (layer, plane, sequence, head, slot) for the cache layouts, the reference's own cumsum / masked_fill / (1 - mask) * -1e4
    lines for positions and masks, explicit loops for the mask scan and the ancestor tables;
  * SENSITIVITY: on the inputs the GPU test uses, every named mutation, stored as a kernel would store it (as_kernel) and pushed
    through the same judge() with the same bounds, is rejected in EVERY case it applies to;
  * the unmutated float32 evaluation passes every bound in every case, so a kernel that fails does not fail for the bound's sake.
"""
import pytest
import torch
import torch.nn.functional as F

import step_rows_reference as R
from attn_reference import pad_add, t16

F64, F32 = torch.float64, torch.float32
REL = 1e-12


def _close(a, b, what=""):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert float((a - b).abs().max()) <= REL * max(float(b.abs().max()), 1e-300), (what, float((a - b).abs().max()), float(b.abs().max()))


def _inner(t):
    """A guarded [1 + rows + 1, cols] buffer without its sentinel rows."""
    return t[1:-1]


# ------------------------------------------------------------------------------------------------ reference against torch
@pytest.mark.parametrize("rows", (1, 5))
def test_layer_norm_equals_torch(rows):
    for c in R.ln_rows_cases(rows):
        want = F.layer_norm(c["x"].double(), (R.D,), c["g"].double(), c["b"].double(), eps=R.LN_EPS)
        _close(next(iter(R.ln_rows(c, F64).values())), want, c["name"])
        if c["kind"] == "const":
            assert torch.equal(R.ln_rows(c, F32)[next(iter(R.ln_rows_kinds(c)))], c["b"].expand(rows, R.D)), "a constant row must give b"
        if c["kind"] in ("mean30", "tiny"):   # the row sums are exact in fp32: summed in the opposite order they are the same
            assert torch.equal(c["x"].sum(dim=1), c["x"].flip(1).sum(dim=1)) and torch.equal(c["x"].sum(dim=1).double(), c["x"].double().sum(dim=1))


def test_step_embedding_equals_torch_embedding():
    for c in R.embed_ln_cases(5):
        S = c["S"]
        tok = c["tok"].long() if c["tok"] is not None else c["ids"][:, c["step"]]
        pos = c["pos"].long() if c["pos"] is not None else torch.full((S,), c["step"])
        x = F.embedding(tok, c["wte"]) + F.embedding(pos, c["wte"])          # wte(input_ids) + wte(position_ids), :291-310
        ev = R.embed_ln(c, F64)
        assert torch.equal(ev["x"], x), c["name"]
        if c["mode"] == "stats":
            _close(ev["stats0"][:, 0], x.double().sum(dim=1), "sum")
            _close(ev["stats0"][:, 1], (x.double() ** 2).sum(dim=1), "sum of squares")
            assert torch.equal(R.from_bits(ev["x16"], c["fp16"]), x.to(t16(c["fp16"])).float())
            assert float(ev["stats_rest"].abs().max()) == 0.0 and ev["stats_rest"].shape == (S, 15, 2)
        else:
            _close(ev[c["mode"]], F.layer_norm(x.double(), (R.D,), c["g"].double(), c["b"].double(), eps=R.LN_EPS), c["name"])


def test_sequence_embedding_equals_torch_embedding():
    for c in R.embed_seq_cases():
        S, Tn, V = c["S"], c["T"], R.V_SMALL
        ids = torch.tensor([[min(max(int(v), 0), V - 1) for v in row] for row in c["ids"].tolist()])
        if c["pos_ids"] is None:
            pos = torch.arange(Tn).unsqueeze(0)                                               # :303-304, shape [1, T]
        else:
            pos = torch.tensor([[min(max(int(v), 0), V - 1) for v in row] for row in c["pos_ids"].tolist()]).view(-1, Tn)   # :295
        x = F.embedding(ids, c["wte"]) + F.embedding(pos, c["wte"])                           # broadcast over the batch, :310
        ev = R.embed_seq_ln(c, F64)
        assert torch.equal(ev["x"], x.reshape(S * Tn, R.D)), c["name"]
        _close(ev["xn"], F.layer_norm(x.double(), (R.D,), c["g"].double(), c["b"].double(), eps=R.LN_EPS).reshape(S * Tn, R.D), c["name"])
        outside = any(v < 0 or v >= V for t in (c["ids"], c["pos_ids"]) if t is not None for v in t.reshape(-1).tolist())
        assert outside == c["dirty"] and int(ev["id_error"]) == (c["id_error"] | int(outside)), c["name"]


def _one(x, fmt):
    """One value block as the format stores it, by torch's own conversions."""
    if fmt is None:
        return x
    if fmt == "e4m3":
        return x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return x.to(torch.float16 if fmt else torch.bfloat16).view(torch.int16)


@pytest.mark.parametrize("case", list(R.kv_slot0_cases()), ids=lambda c: c["name"])
def test_image_slot_layout_equals_an_explicit_loop(case):
    c = case
    L, S, slots, rm = c["L"], c["S"], c["slots"], c["row_mul"]
    want = R.guarded_flat(c["n"], R.store_dtype(c["fmt"]))
    for l in range(L):
        for kv in range(2):
            for s in range(S):
                for hd in range(R.H):
                    col = (l * 2 + kv) * R.D + hd * 64
                    o = R.GUARD + l * c["layer_stride"] + kv * c["kv_stride"] + ((s * rm * R.H + hd) * slots + 0) * 64
                    want[o:o + 64] = _one(c["ukv"][s, col:col + 64], c["fmt"])
    got = R.kv_slot0(c, F64)["kv"]
    assert got.dtype == want.dtype and torch.equal(got, want)
    written = L * 2 * S * R.D
    assert int((got != R.sentinel(got.dtype)).sum()) >= written - 8 and written > 1024 * 256   # (a value may equal the sentinel by chance)
    if c["fmt"] == "e4m3":   # the edge values: clamped beyond +-448, subnormals kept, below half the smallest subnormal 0
        b = R.KV8.from_bytes(got[R.GUARD:R.GUARD + 22])
        assert b[:5].tolist() == [448.0, -448.0, 448.0, 448.0, -448.0] and b[5:9].tolist() == [2.0 ** -9, 0.0, 2.0 ** -8, -(2.0 ** -9)]
        assert b[10:13].tolist() == [1.0, 1.25, 15.0] and bool(torch.isfinite(b).all())


@pytest.mark.parametrize("case", list(R.prompt_kv_cases()) + list(R.prompt_kv_cases(large=True)), ids=lambda c: c["name"])
def test_prompt_cache_layout_equals_an_explicit_loop(case):
    c = case
    S, Tn, slots, rm = c["S"], c["T"], c["slots"], c["row_mul"]
    want = {n: R.guarded_flat(c["n"], R.store_dtype(c["fmt"])) for n in ("k", "v")}
    for s in range(S):
        for hd in range(R.H):
            for t in range(Tn):
                slot = 1 + t
                o = R.GUARD + ((s * rm * R.H + hd) * slots + slot) * 64
                for i, n in enumerate(("k", "v")):
                    col = (1 + i) * R.D + hd * 64
                    want[n][o:o + 64] = _one(c["qkv"][s * Tn + t, col:col + 64], c["fmt"])
    got = R.prompt_kv_store(c, F64)
    for n in ("k", "v"):
        assert torch.equal(got[n], want[n]), n
        plane = got[n][R.GUARD:-R.GUARD].reshape(S * rm, R.H, slots, 64)
        sent = R.sentinel(plane.dtype)
        assert bool((plane[:, :, 0] == sent).all()) and bool((plane[:, :, Tn + 1:] == sent).all()), "slot 0 and the slots behind T stay"
    if c["T"] == 300:
        assert S * R.H * 2 * Tn * 16 > 4096 * 256 and 2 * c["n"] * 4 < 25e6


def test_prompt_positions_and_masks_equal_the_reference_lines():
    for c in R.prompt_setup_cases():
        S, Tn, slots = c["S"], c["T"], c["slots"]
        ev = R.prompt_setup(c, F64)
        assert int(ev["step"]) == Tn - 1
        ids = _inner(ev["ids"])
        assert bool((ids[:, Tn:] == R.SENTI).all()) and int(ids[:, :Tn].min()) >= 0 and int(ids[:, :Tn].max()) < R.V_SMALL
        inside = (c["in"] >= 0) & (c["in"] < R.V_SMALL)
        assert torch.equal(ids[:, :Tn][inside], c["in"][inside]) and ids[0, 0] == 0 and ids[-1, Tn - 1] == R.V_SMALL - 1
        if c["pad"] is None:
            assert bool((ev["pos"] == R.SENTI).all()) and bool((ev["kmask"] == R.SENT).all())
            continue
        am = (torch.arange(Tn)[None, :] >= c["pad"][:, None]).long()
        position_ids = am.long().cumsum(-1) - 1                      # :508
        position_ids.masked_fill_(am == 0, 1)                        # :509
        assert torch.equal(_inner(ev["pos"]), position_ids)
        if c["kmask"]:
            grown = torch.cat((am, am.new_ones((S, slots - 1 - Tn))), dim=-1)            # :525, once per later step
            assert torch.equal(_inner(ev["kmask"]), pad_add(grown, F64)[:, 0, 0, :].float())
        else:
            assert bool((ev["kmask"] == R.SENT).all())
    for c in R.key_mask_cases():
        grown = torch.cat((c["am"], torch.ones(c["S"], c["slots"] - 1 - c["L"])), dim=-1)
        assert torch.equal(_inner(R.key_mask(c, F64)["kmask"]), pad_add(grown, F64)[:, 0, 0, :].float())
    for c in R.beam_first_mask_cases():
        am = (torch.arange(c["slots"] - 1)[None, :] >= c["first"][:, None]).float()
        assert torch.equal(_inner(R.beam_first_mask(c, F64)["kmask"]), pad_add(am, F64)[:, 0, 0, :].float())


def test_mask_scan_equals_an_explicit_loop():
    seen = set()
    for c in R.mask_scan_cases():
        am = c["am"].tolist()
        flags, pads = c["flags0"], []
        for row in am:
            p = 0
            while p < len(row) and row[p] == 0:
                p += 1
            pads.append(p)
            flags |= (1 if p == len(row) else 0) | (4 if p > 0 else 0)
            for v in row[p:]:
                flags |= 2 if v == 0 else (8 if v != 1 else 0)
        ev = R.prompt_mask_scan(c, F64)
        assert _inner(ev["pad"])[:, 0].tolist() == pads and int(ev["flags"]) == flags, c["name"]
        seen.add(flags)
    # clean masks give 0 or "padded" alone; every refusal bit is raised by some case; a word that is not clear is OR-ed into
    assert {0, 4, 16 | 2} <= seen and all(any(f & bit for f in seen) for bit in (1, 2, 4, 8)), seen


def test_index_kernels_equal_explicit_loops():
    for c in R.beam_advance_cases():
        R_, Tn, t = c["R"], c["T"], c["step"]
        want = [[R.SENTI] * Tn for _ in range(R_)]
        for r in range(R_):
            p = int(c["parent"][r])
            for j in range(t + 1):
                want[r][j] = int(c["src_old"][p, j])
            want[r][t + 1] = p
        ev = R.beam_advance(c, F64)
        assert _inner(ev["src_new"]).tolist() == want and torch.equal(ev["src_old"], c["src_old"])
    p = next(iter(R.beam_advance_cases()))["parent"].tolist()
    assert len(set(p)) < len(p) and any(p[r] == r for r in range(len(p))) and any(p[r] != r for r in range(len(p)))
    for c in R.beam_prompt_init_cases():
        ev = R.beam_prompt_init(c, F64)
        a = _inner(ev["src_a"])
        for r in range(c["R"]):
            first = (r // c["nb"]) * c["nb"]
            assert a[r].tolist() == [first] * (c["T"] + 1) + [R.SENTI] * (c["slots"] - c["T"] - 1)
            assert int(_inner(ev["beam_pad"])[r]) == (0 if c["pad"] is None else int(c["pad"][r // c["nb"]]))
        assert torch.equal(ev["src_a"], ev["src_b"])
    for c in R.decode_reset_cases():
        ids = _inner(R.decode_reset(c, F64)["ids"])
        assert bool((ids[:, :c["L"]] == 50256).all()) and bool((ids[:, c["L"]:] == R.SENTI).all()) and c["ld_ids"] > c["L"]
    for c in R.forward_cached_cases():
        ev = R.forward_cached_tokens(c, F64)
        assert _inner(ev["tok"])[:3, 0].tolist() == [0, R.V_SMALL - 1, R.V_SMALL - 1] and int(ev["step"]) == 17
        assert bool((ev["row_pos"] == R.SENTI).all()) == (c["pos_ids"] is None)
    for c in R.step_rows_cases():
        ev = R.prompt_step_rows(c, F64)
        assert _inner(ev["row_pos"])[:, 0].tolist() == [4 - int(p) for p in c["pad"]] and _inner(ev["tok"])[:, 0].tolist() == c["ids"][:, 4].tolist()


def test_truncation_is_toward_zero_and_differs_from_nearest():
    x = torch.cat((torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 3, torch.tensor([1.00390625, -1.01171875, 65520.0, -0.0, 0.0])))
    for fp16 in (0, 1):
        t = R.from_bits(R.trunc16_bits(x, fp16), fp16)
        n = R.from_bits(R.to_bits(x, fp16), fp16)
        assert bool((t.abs() <= x.abs()).all()) and bool(torch.isfinite(t).all())
        assert bool(((t == n) | (n.abs() > x.abs())).all()) and 0.3 < float((t != n).float().mean()) < 0.7


# ------------------------------------------------------------------------------------------------ sensitivity and self-check
@pytest.mark.parametrize("kernel", list(R.KERNELS))
def test_mutations_are_rejected_and_float32_passes(kernel):
    """For every case of the kernel's GPU test: the float32 evaluation passes; every mutation that applies to it is rejected."""
    k = R.KERNELS[kernel]
    seen = {m: 0 for m in k.mutations}
    n = 0
    for c in k.cases():
        kinds, fp16 = R.kinds_of(kernel, c), R.fp16_of(c)
        r64, r32 = k.ev(c, F64), k.ev(c, F32)
        assert set(r64) == set(kinds), (c["name"], set(r64), set(kinds))
        own = R.judge(R.as_kernel(r32, kinds, fp16), r64, r32, kinds, fp16)
        assert all(v["ok"] for v in own.values()), (kernel, c["name"], own)
        n += 1
        for m, applies in k.mutations.items():
            if not applies(c):
                continue
            res = R.judge(R.as_kernel(k.ev(c, F64, m), kinds, fp16, m), r64, r32, kinds, fp16)
            assert not all(v["ok"] for v in res.values()), f"{kernel}: {m} stays inside the bound at {c['name']}: {res}"
            seen[m] += 1
    assert n > 0 and all(v > 0 for v in seen.values()), seen


def test_the_large_prompt_case_rejects_its_mutations_too():
    k = R.KERNELS["prompt_kv_store"]
    for c in R.prompt_kv_cases(large=True):
        r64 = k.ev(c, F64)
        for m in ("kv_swapped", "slot_t"):
            res = R.judge(R.as_kernel(k.ev(c, F64, m), k.kinds, None, m), r64, r64, k.kinds)
            assert not all(v["ok"] for v in res.values()), m


def test_every_required_mutation_is_in_the_table():
    """The list the tests were asked to cover, by the name it has here."""
    M = R.MUTATIONS
    required = (("embed_ln", "position_from_step"), ("embed_ln", "token_from_ids"), ("ln_rows", "unbiased_variance"), ("ln_rows", "missing_eps"),
                ("embed_ln", "stats_centred"), ("embed_ln", "stats_rest_not_zeroed"), ("prompt_setup", "masked_position_0"),
                ("prompt_setup", "key_mask_shifted"), ("beam_first_mask", "key_mask_shifted"), ("kv_slot0", "kv_swapped"),
                ("prompt_kv_store", "kv_swapped"), ("prompt_kv_store", "slot_t"), ("kv_slot0", "row_mul_ignored"),
                ("prompt_kv_store", "row_mul_ignored"), ("ln_rows", "truncate16"), ("embed_ln", "truncate16"), ("kv_slot0", "truncate16"),
                ("prompt_kv_store", "truncate16"), ("embed_seq_ln", "pos_not_broadcast"), ("beam_advance", "slot_own_row"))
    for kernel, m in required:
        assert m in M[kernel], (kernel, m)
    assert R.MARGIN == 8.0 and R.ROWS == (1, 4, 5, 131)
