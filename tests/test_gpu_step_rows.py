"""The kernels that start every decode step and the bookkeeping kernels between steps ALONE, against the float64 reference of
tests/step_rows_reference.py, through the rgrg_debug_* hooks that launch them with the product's own launchers (grids and grid-stride
loops included):
  rgrg_amd/csrc/decoder.hip         embed_ln_kernel, ln_rows_kernel, kv_slot0_kernel<float / u16 / uint8_t>, decode_reset_kernel,
                                    key_mask_kernel, beam_first_mask_kernel, forward_cached_tokens_kernel
  rgrg_amd/csrc/decoder_lm.hip      embed_seq_ln_kernel
  rgrg_amd/csrc/decoder_prompt.hip  prompt_mask_scan_kernel, prompt_setup_kernel, prompt_kv_store_kernel<float / u16>,
                                    prompt_last_rows_kernel, prompt_step_rows_kernel, beam_prompt_init_kernel, beam_row_pos_kernel
  rgrg_amd/csrc/decoder_beam.hip    beam_init_kernel, beam_advance_kernel
One launch per case, every output element compared; the bounds come from the reference alone (fp32 outputs MARGIN * noise + 2^-23
max|ref|, 16-bit LayerNorm outputs half an ulp at the element's own magnitude on top of MARGIN * noise, every copy, rounding, index and
mask exact).  Every output buffer carries sentinels in front of and behind the written range - and between the written elements where
the kernel skips some -, which must stay.  Each figure is printed before it is asserted (lines starting with STEPROWS); the worst ones
observed on the MI355X are kept in profiles/step_rows_parity.md.
"""
import pytest
import torch

import step_rows_reference as R
from attn_reference import from_bits, to_bits
from rgrg_amd import _hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
RGRG_EINVAL = -1
D, V = R.D, R.V_SMALL


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(t, dtype=None):
    return None if t is None else t.to(device=DEV, dtype=dtype or t.dtype).contiguous()


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.rgrg_last_error())
    torch.cuda.synchronize()


def _refused(lib, rc, what):
    assert rc == RGRG_EINVAL and lib.rgrg_last_error(), (what, rc)


def _report(kernel, case, res):
    for name, r in res.items():
        print(f"STEPROWS kernel={kernel} case={case} out={name} err={r['err']:.3e} noise={r['noise']:.3e} bound={r['bound']:.3e} "
              f"used={r['used']:.3f}")
    for name, r in res.items():
        assert r["ok"], f"{kernel} {case} {name}: err {r['err']:.3e} exceeds {r['bound']:.3e} (noise {r['noise']:.3e})"


def _judge(kernel, c, got):
    """The case's outputs against the float64 evaluation, with the float32 one as the noise measurement."""
    k = R.KERNELS[kernel]
    _report(kernel, c["name"], R.judge(got, k.ev(c, F64), k.ev(c, F32), R.kinds_of(kernel, c), R.fp16_of(c)))


def _buf(rows, cols, dtype):
    """[1 + rows + 1, cols] of the dtype's sentinel on the device; _row1 is what the launch gets."""
    return R.guarded(rows, cols, dtype).to(DEV)


def _row1(b):
    return None if b is None else b[1:].data_ptr()


def _untouched(*bufs):
    """The sentinel rows in front of and behind the rows of every buffer (None: skipped); whole = the buffer must not be written at all."""
    return all(bool((b[0] == R.sentinel(b.dtype)).all()) and bool((b[-1] == R.sentinel(b.dtype)).all()) for b in bufs if b is not None)


def _whole(b):
    return bool((b == R.sentinel(b.dtype)).all())


def _scalar(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ LayerNorm and the embeddings
@pytest.mark.parametrize("rows", R.ROWS)
def test_ln_rows(lib, rows):
    """ln_rows_kernel: one wave per row, four rows per workgroup; fp32, bf16 and fp16 output."""
    for c in R.ln_rows_cases(rows):
        fp16 = c["fp16"]
        x, g, b = _dev(c["x"]), _dev(c["g"]), _dev(c["b"])
        xn, xn16 = _buf(rows, D, torch.float32), _buf(rows, D, torch.int16)   # both given, as the step gives them
        _ok(lib, lib.rgrg_debug_ln_rows(_p(x), _p(g), _p(b), _row1(xn), None if fp16 is None else _row1(xn16), fp16 or 0, rows, D, None), c["name"])
        assert _untouched(xn, xn16) and _whole(xn16 if fp16 is None else xn), "a row outside the launch, or the output of the other mode, was written"
        assert torch.equal(x.cpu(), c["x"])
        got = {"xn": xn[1:-1].cpu()} if fp16 is None else {"xn16": from_bits(xn16[1:-1].cpu(), fp16)}
        _judge("ln_rows", c, got)
        if c["kind"] == "const":   # every partial sum is exact in any order: x - mean is 0 and the output is b
            want = c["b"].expand(rows, D)
            assert torch.equal(got["xn"], want) if fp16 is None else torch.equal(xn16[1:-1].cpu(), to_bits(want, fp16))


@pytest.mark.parametrize("S", (1, 5))
def test_embed_ln(lib, S):
    """embed_ln_kernel: token and position from the id buffer and *step or from the per-row overrides; the three output modes."""
    for c in R.embed_ln_cases(S):
        fp16, mode = c["fp16"], c["mode"]
        wte, ids, step, g, b = _dev(c["wte"]), _dev(c["ids"]), _scalar(c["step"]), _dev(c["g"]), _dev(c["b"])
        tok, pos = _dev(c["tok"]), _dev(c["pos"])
        x, xn, xn16, stats = _buf(S, D, torch.float32), _buf(S, D, torch.float32), _buf(S, D, torch.int16), _buf(S, 32, torch.float32)
        _ok(lib, lib.rgrg_debug_embed_ln(_p(wte), _p(ids), c["ld_ids"], _p(step), _p(tok), _p(pos), _p(g), _p(b), _row1(x), _row1(xn),
                                         None if mode == "xn" else _row1(xn16), _row1(stats) if mode == "stats" else None, fp16 or 0, S, D, None),
            c["name"])
        assert _untouched(x, xn, xn16, stats), "a row in front of or behind the launch's rows was written"
        assert int(step) == c["step"] and torch.equal(ids.cpu(), c["ids"])
        got = {"x": x[1:-1].cpu()}
        if mode == "xn":
            got["xn"] = xn[1:-1].cpu()
            assert _whole(xn16) and _whole(stats), "the fp32 mode wrote a 16-bit output or the slots"
        elif mode == "xn16":
            got["xn16"] = from_bits(xn16[1:-1].cpu(), fp16)
            assert _whole(xn) and _whole(stats), "the 16-bit mode wrote the fp32 output or the slots"
        else:
            st = stats[1:-1].cpu().reshape(S, 16, 2)
            got.update(x16=xn16[1:-1].cpu(), stats0=st[:, 0], stats_rest=st[:, 1:].contiguous())
            assert _whole(xn), "the folded mode wrote the fp32 LayerNorm output"
            assert torch.equal(got["x16"], to_bits(got["x"], fp16)), "the raw 16-bit row is not the rounding of the x the kernel stored"
        _judge("embed_ln", c, got)


@pytest.mark.parametrize("case", list(R.embed_seq_cases()), ids=lambda c: c["name"])
def test_embed_seq_ln(lib, case):
    """embed_seq_ln_kernel: default, [S,T] and broadcast [1,T] positions; ids and positions outside the table clamped and reported."""
    c = case
    S, Tn, M = c["S"], c["T"], c["S"] * c["T"]
    wte, ids, pos, g, b = _dev(c["wte"]), _dev(c["ids"]), _dev(c["pos_ids"]), _dev(c["g"]), _dev(c["b"])
    x, xn, err = _buf(M, D, torch.float32), _buf(M, D, torch.float32), _scalar(c["id_error"])
    _ok(lib, lib.rgrg_debug_embed_seq_ln(_p(wte), _p(ids), _p(pos), 0 if pos is None else pos.numel(), _p(g), _p(b), _row1(x), _row1(xn), _p(err),
                                         S, Tn, D, V, None), c["name"])
    assert _untouched(x, xn) and torch.equal(ids.cpu(), c["ids"])
    _judge("embed_seq_ln", c, {"x": x[1:-1].cpu(), "xn": xn[1:-1].cpu(), "id_error": err.cpu()})


# ------------------------------------------------------------------------------------------------ cache writes
def _flat_ptr(b):
    return b[R.GUARD:].data_ptr()


@pytest.mark.parametrize("case", list(R.kv_slot0_cases()), ids=lambda c: c["name"])
def test_kv_slot0(lib, case):
    """kv_slot0_kernel<float / u16 / uint8_t>: more values than the launch has threads; slots 1 .. and the rows between s * row_mul stay."""
    c = case
    fmt = c["fmt"]
    ukv = _dev(c["ukv"])
    kv = R.guarded_flat(c["n"], R.store_dtype(fmt)).to(DEV)
    _ok(lib, lib.rgrg_debug_kv_slot0(_p(ukv), c["ld"], _flat_ptr(kv), c["layer_stride"], c["kv_stride"], c["S"], R.H, c["slots"], c["L"],
                                     c["row_mul"], {None: 4, 0: 2, 1: 2, "e4m3": 1}[fmt], 1 if fmt == 1 else 0, None), c["name"])
    assert torch.equal(ukv.cpu(), c["ukv"])
    _judge("kv_slot0", c, {"kv": kv.cpu()})


def _run_prompt_kv(lib, c):
    fmt = c["fmt"]
    qkv = _dev(c["qkv"])
    k, v = (R.guarded_flat(c["n"], R.store_dtype(fmt)).to(DEV) for _ in range(2))
    _ok(lib, lib.rgrg_debug_prompt_kv_store(_p(qkv), _flat_ptr(k), _flat_ptr(v), c["S"], R.H, c["T"], c["slots"], c["row_mul"], 4 if fmt is None else 2,
                                            1 if fmt == 1 else 0, None), c["name"])
    assert torch.equal(qkv.cpu(), c["qkv"])
    _judge("prompt_kv_store", c, {"k": k.cpu(), "v": v.cpu()})


@pytest.mark.parametrize("case", list(R.prompt_kv_cases()), ids=lambda c: c["name"])
def test_prompt_kv_store(lib, case):
    """prompt_kv_store_kernel<float / u16>: slots 1 .. T of cache row s * row_mul; slot 0 and the slots behind T stay."""
    _run_prompt_kv(lib, case)


def test_prompt_kv_store_beyond_the_grid(lib):
    """8 x 300 prompt tokens: more 16-byte pieces than the 4096 x 256 threads of the launch."""
    for c in R.prompt_kv_cases(large=True):
        _run_prompt_kv(lib, c)


@pytest.mark.parametrize("case", list(R.prompt_last_cases()), ids=lambda c: c["name"])
def test_prompt_last_rows(lib, case):
    c = case
    R_, fp16 = c["R"], c["fp16"]
    xa = _dev(c["xn_all"])
    xn, xn16 = _buf(R_, D, torch.float32), _buf(R_, D, torch.int16)
    _ok(lib, lib.rgrg_debug_prompt_last_rows(_p(xa), c["T"], D, _row1(xn), None if fp16 is None else _row1(xn16), fp16 or 0, R_, c["row_div"], None),
        c["name"])
    got = {"xn": xn.cpu()}
    if fp16 is None:
        assert _whole(xn16)
    else:
        got["xn16"] = xn16.cpu()
    _judge("prompt_last_rows", c, got)


# ------------------------------------------------------------------------------------------------ masks and positions of a prompt
@pytest.mark.parametrize("case", list(R.mask_scan_cases()), ids=lambda c: c["name"])
def test_prompt_mask_scan(lib, case):
    c = case
    S, Tn = c["am"].shape
    am, pad, flags = _dev(c["am"]), _buf(S, 1, torch.int32), _scalar(c["flags0"])
    _ok(lib, lib.rgrg_debug_prompt_mask_scan(_p(am), S, Tn, _row1(pad), _p(flags), None), c["name"])
    _judge("prompt_mask_scan", c, {"pad": pad.cpu(), "flags": flags.cpu()})


@pytest.mark.parametrize("case", list(R.prompt_setup_cases()), ids=lambda c: c["name"])
def test_prompt_setup(lib, case):
    """prompt_setup_kernel: pos and kmask are not written when their operand is NULL."""
    c = case
    S, Tn, slots = c["S"], c["T"], c["slots"]
    inp, pad, step = _dev(c["in"]), _dev(c["pad"]), _scalar(R.SENTI)
    ids, pos, kmask = _buf(S, c["ld_ids"], torch.int64), _buf(S, Tn, torch.int64), _buf(S, slots, torch.float32)
    _ok(lib, lib.rgrg_debug_prompt_setup(_p(inp), S, Tn, V, _row1(ids), c["ld_ids"], _p(step), _p(pad), _row1(pos) if pad is not None else None,
                                         _row1(kmask) if c["kmask"] else None, slots, None), c["name"])
    assert torch.equal(inp.cpu(), c["in"])
    _judge("prompt_setup", c, {"ids": ids.cpu(), "step": step.cpu(), "pos": pos.cpu(), "kmask": kmask.cpu()})


# ------------------------------------------------------------------------------------------------ index kernels
def test_prompt_step_rows_and_beam_row_pos(lib):
    for c in R.step_rows_cases():
        S = c["S"]
        ids, step, pad = _dev(c["ids"]), _scalar(c["step"]), _dev(c["pad"])
        tok, row_pos = _buf(S, 1, torch.int32), _buf(S, 1, torch.int32)
        _ok(lib, lib.rgrg_debug_prompt_step_rows(_p(ids), c["ld_ids"], _p(step), _p(pad), _row1(tok), _row1(row_pos), S, None), c["name"])
        _judge("prompt_step_rows", c, {"tok": tok.cpu(), "row_pos": row_pos.cpu()})
    for c in R.beam_row_pos_cases():
        step, pad, row_pos = _scalar(c["step"]), _dev(c["pad"]), _buf(c["R"], 1, torch.int32)
        _ok(lib, lib.rgrg_debug_beam_row_pos(_p(step), _p(pad), _row1(row_pos), c["R"], None), c["name"])
        _judge("beam_row_pos", c, {"row_pos": row_pos.cpu()})


def test_beam_prompt_init_and_beam_init(lib):
    for c in R.beam_prompt_init_cases():
        R_, slots = c["R"], c["slots"]
        a, b, bp, pad = _buf(R_, slots, torch.int32), _buf(R_, slots, torch.int32), _buf(R_, 1, torch.int32), _dev(c["pad"])
        _ok(lib, lib.rgrg_debug_beam_prompt_init(_row1(a), _row1(b), slots, c["nb"], R_, c["T"], _p(pad), _row1(bp), None), c["name"])
        _judge("beam_prompt_init", c, {"src_a": a.cpu(), "src_b": b.cpu(), "beam_pad": bp.cpu()})
    for c in R.beam_init_cases():
        src, step = _buf(c["R"], c["T"], torch.int32), _scalar(R.SENTI)
        _ok(lib, lib.rgrg_debug_beam_init(_row1(src), c["T"], c["nb"], c["R"], _p(step), None), c["name"])
        _judge("beam_init", c, {"src": src.cpu(), "step": step.cpu()})


def test_slot_masks(lib):
    """beam_first_mask_kernel and key_mask_kernel (L < slots - 1, mask values 0 / 1): the image slot is never masked."""
    for c in R.beam_first_mask_cases():
        first, km = _dev(c["first"]), _buf(c["R"], c["slots"], torch.float32)
        _ok(lib, lib.rgrg_debug_beam_first_mask(_p(first), c["R"], c["slots"], _row1(km), None), c["name"])
        _judge("beam_first_mask", c, {"kmask": km.cpu()})
    for c in R.key_mask_cases():
        am, km = _dev(c["am"]), _buf(c["S"], c["slots"], torch.float32)
        _ok(lib, lib.rgrg_debug_key_mask(_p(am), c["L"], c["S"], c["slots"], _row1(km), None), c["name"])
        _judge("key_mask", c, {"kmask": km.cpu()})


def test_forward_cached_tokens(lib):
    for c in R.forward_cached_cases():
        S = c["S"]
        ids, pos, step = _dev(c["ids"]), _dev(c["pos_ids"]), _scalar(R.SENTI)
        tok, row_pos = _buf(S, 1, torch.int32), _buf(S, 1, torch.int32)
        _ok(lib, lib.rgrg_debug_forward_cached_tokens(_p(ids), _p(pos), c["T"], c["j"], S, V, _row1(tok), _row1(row_pos), _p(step), c["position"], None),
            c["name"])
        _judge("forward_cached_tokens", c, {"tok": tok.cpu(), "row_pos": row_pos.cpu(), "step": step.cpu()})


def test_decode_reset(lib):
    """decode_reset_kernel: more ids than the 64 x 256 threads of the launch, more rows than the 256-thread loop; columns L .. stay."""
    for c in R.decode_reset_cases():
        S = c["S"]
        ids, fin = _buf(S, c["ld_ids"], torch.int64), _buf(S, 1, torch.int32)
        step, done, sync = _scalar(R.SENTI), _scalar(R.SENTI), torch.full((2,), R.SENTI, dtype=torch.int32, device=DEV)
        _ok(lib, lib.rgrg_debug_decode_reset(_row1(ids), c["ld_ids"], _row1(fin), _p(step), _p(done), _p(sync), S, c["L"], None), c["name"])
        _judge("decode_reset", c, {"ids": ids.cpu(), "finished": fin.cpu(), "step": step.cpu(), "done_len": done.cpu(), "sync": sync.cpu()})


@pytest.mark.parametrize("case", list(R.beam_advance_cases()), ids=lambda c: c["name"])
def test_beam_advance(lib, case):
    """beam_advance_kernel: slots above *step + 1 of the new table stay, the old table and the step word are only read."""
    c = case
    R_, Tn = c["R"], c["T"]
    old, parent, step, new = _dev(c["src_old"]), _dev(c["parent"]), _scalar(c["step"]), _buf(R_, Tn, torch.int32)
    _ok(lib, lib.rgrg_debug_beam_advance(_p(old), _row1(new), _p(parent), _p(step), Tn, R_, None), c["name"])
    _judge("beam_advance", c, {"src_new": new.cpu(), "src_old": old.cpu(), "step": step.cpu()})


# ------------------------------------------------------------------------------------------------ refusals
def test_hooks_refuse_what_their_kernels_cannot_take(lib):
    """Every RGRG_EINVAL rule once, with a message; nothing is launched (the buffers would be too small for several of them)."""
    f = torch.zeros(4 * D, device=DEV)
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(64, dtype=torch.int64, device=DEV)
    F_, I, I2, L = _p(f), _p(i32), i32[32:].data_ptr(), _p(i64)
    # missing operands
    _refused(lib, lib.rgrg_debug_ln_rows(F_, None, F_, F_, None, 0, 4, D, None), "ln_rows without the gain")
    _refused(lib, lib.rgrg_debug_ln_rows(F_, F_, F_, None, None, 0, 4, D, None), "ln_rows without an output")
    _refused(lib, lib.rgrg_debug_embed_ln(F_, None, 9, I, None, None, F_, F_, F_, F_, None, None, 0, 1, D, None), "embed_ln without a token source")
    _refused(lib, lib.rgrg_debug_embed_ln(F_, L, 9, I, None, None, F_, F_, F_, F_, None, F_, 0, 1, D, None), "embed_ln: slots without the 16-bit row")
    _refused(lib, lib.rgrg_debug_embed_seq_ln(F_, L, None, 0, F_, F_, F_, F_, None, 1, 2, D, V, None), "embed_seq_ln without the error word")
    _refused(lib, lib.rgrg_debug_kv_slot0(None, 4096, F_, 8192, 4096, 1, 1, 1, 1, 1, 4, 0, None), "kv_slot0 without ukv")
    _refused(lib, lib.rgrg_debug_decode_reset(L, 8, I, I, None, I, 1, 4, None), "decode_reset without done_len")
    _refused(lib, lib.rgrg_debug_beam_first_mask(None, 1, 4, F_, None), "beam_first_mask without first")
    _refused(lib, lib.rgrg_debug_key_mask(None, 2, 1, 4, F_, None), "key_mask without the mask")
    _refused(lib, lib.rgrg_debug_forward_cached_tokens(L, L, 2, 0, 1, V, I, None, I, 0, None), "forward_cached_tokens: positions without row_pos")
    _refused(lib, lib.rgrg_debug_prompt_mask_scan(F_, 1, 2, I, None, None), "prompt_mask_scan without the flag word")
    _refused(lib, lib.rgrg_debug_prompt_setup(L, 1, 2, V, L, 4, None, None, None, None, 4, None), "prompt_setup without the step word")
    _refused(lib, lib.rgrg_debug_prompt_kv_store(F_, F_, None, 1, 1, 1, 2, 1, 4, 0, None), "prompt_kv_store without the V plane")
    _refused(lib, lib.rgrg_debug_prompt_last_rows(F_, 1, D, None, None, 0, 1, 1, None), "prompt_last_rows without xn")
    _refused(lib, lib.rgrg_debug_prompt_step_rows(L, 4, I, None, I, I, 1, None), "prompt_step_rows without pad")
    _refused(lib, lib.rgrg_debug_beam_prompt_init(I, None, 4, 1, 1, 2, None, I, None), "beam_prompt_init without the second table")
    _refused(lib, lib.rgrg_debug_beam_row_pos(I, None, I, 1, None), "beam_row_pos without beam_pad")
    _refused(lib, lib.rgrg_debug_beam_init(None, 4, 1, 1, I, None), "beam_init without the table")
    _refused(lib, lib.rgrg_debug_beam_advance(I, None, I, I, 4, 1, None), "beam_advance without the new table")
    # rows < 1
    _refused(lib, lib.rgrg_debug_ln_rows(F_, F_, F_, F_, None, 0, 0, D, None), "ln_rows, no rows")
    _refused(lib, lib.rgrg_debug_embed_ln(F_, L, 9, I, None, None, F_, F_, F_, F_, None, None, 0, 0, D, None), "embed_ln, no rows")
    _refused(lib, lib.rgrg_debug_embed_seq_ln(F_, L, None, 0, F_, F_, F_, F_, I, 0, 2, D, V, None), "embed_seq_ln, no sentences")
    _refused(lib, lib.rgrg_debug_kv_slot0(F_, 4096, F_, 8192, 4096, 0, 1, 1, 1, 1, 4, 0, None), "kv_slot0, no rows")
    _refused(lib, lib.rgrg_debug_prompt_kv_store(F_, F_, F_, 0, 1, 1, 2, 1, 4, 0, None), "prompt_kv_store, no rows")
    _refused(lib, lib.rgrg_debug_prompt_last_rows(F_, 1, D, F_, None, 0, 0, 1, None), "prompt_last_rows, no rows")
    _refused(lib, lib.rgrg_debug_decode_reset(L, 8, I, I, I, I, 0, 4, None), "decode_reset, no rows")
    _refused(lib, lib.rgrg_debug_beam_advance(I, I2, I, I, 4, 0, None), "beam_advance, no rows")
    # a row length other than the 1024 the kernels are written for
    _refused(lib, lib.rgrg_debug_ln_rows(F_, F_, F_, F_, None, 0, 4, 512, None), "ln_rows, D = 512")
    _refused(lib, lib.rgrg_debug_embed_ln(F_, L, 9, I, None, None, F_, F_, F_, F_, None, None, 0, 1, 2048, None), "embed_ln, D = 2048")
    _refused(lib, lib.rgrg_debug_embed_seq_ln(F_, L, None, 0, F_, F_, F_, F_, I, 1, 2, 768, V, None), "embed_seq_ln, D = 768")
    _refused(lib, lib.rgrg_debug_prompt_last_rows(F_, 1, 1000, F_, None, 0, 1, 1, None), "prompt_last_rows, D = 1000")
    # the key mask is made from pad[]: without it the kernel would dereference NULL
    _refused(lib, lib.rgrg_debug_prompt_setup(L, 1, 2, V, L, 4, I, None, None, F_, 4, None), "prompt_setup: a key mask without pad")
    _refused(lib, lib.rgrg_debug_prompt_setup(L, 1, 2, V, L, 4, I, I, None, None, 4, None), "prompt_setup: pad without pos")
    # the 16-bit type on a format that is not 16 bit
    _refused(lib, lib.rgrg_debug_kv_slot0(F_, 4096, F_, 8192, 4096, 1, 1, 1, 1, 1, 4, 1, None), "kv_slot0: fp16 on the fp32 cache")
    _refused(lib, lib.rgrg_debug_kv_slot0(F_, 4096, F_, 8192, 4096, 1, 1, 1, 1, 1, 1, 1, None), "kv_slot0: fp16 on the e4m3 cache")
    _refused(lib, lib.rgrg_debug_prompt_kv_store(F_, F_, F_, 1, 1, 1, 2, 1, 4, 1, None), "prompt_kv_store: fp16 on the fp32 cache")
    _refused(lib, lib.rgrg_debug_prompt_kv_store(F_, F_, F_, 1, 1, 1, 2, 1, 1, 0, None), "prompt_kv_store: the e4m3 cache takes no prompt")
    _refused(lib, lib.rgrg_debug_ln_rows(F_, F_, F_, F_, None, 1, 4, D, None), "ln_rows: fp16 with the fp32 output")
    _refused(lib, lib.rgrg_debug_prompt_last_rows(F_, 1, D, F_, None, 1, 1, 1, None), "prompt_last_rows: fp16 without xn16")
    # shapes the launches would run out of their buffers with
    _refused(lib, lib.rgrg_debug_embed_seq_ln(F_, L, L, 3, F_, F_, F_, F_, I, 2, 2, D, V, None), "embed_seq_ln: pos_rows neither T nor S * T")
    _refused(lib, lib.rgrg_debug_kv_slot0(F_, 100, F_, 8192, 4096, 1, 1, 1, 1, 1, 4, 0, None), "kv_slot0: ld below L * 2 * D")
    _refused(lib, lib.rgrg_debug_kv_slot0(F_, 4096, F_, 8192, 32, 1, 1, 1, 1, 1, 4, 0, None), "kv_slot0: overlapping planes")
    _refused(lib, lib.rgrg_debug_prompt_kv_store(F_, F_, F_, 1, 1, 2, 2, 1, 4, 0, None), "prompt_kv_store: slots <= T")
    _refused(lib, lib.rgrg_debug_decode_reset(L, 3, I, I, I, I, 1, 4, None), "decode_reset: ld_ids < L")
    _refused(lib, lib.rgrg_debug_beam_prompt_init(I, I, 4, 2, 3, 2, None, I, None), "beam_prompt_init: R % nb")
    step = _scalar(3)
    _refused(lib, lib.rgrg_debug_beam_advance(I, I2, I, _p(step), 4, 2, None), "beam_advance: *step + 1 outside the table")
    parent = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    _refused(lib, lib.rgrg_debug_beam_advance(I, I2, _p(parent), I, 4, 2, None), "beam_advance: a parent outside the rows")
    _refused(lib, lib.rgrg_debug_beam_advance(I, I, I, I, 4, 2, None), "beam_advance in place")
    torch.cuda.synchronize()
