"""Prompted greedy search on the MI355X (rgrg_decoder_generate_prompted; LanguageModel.greedy_search, Engine.greedy_decode_prompted,
ReportGenerationModel.generate_from_prompts): the batched prompt pass into the decode cache and the decode loop behind it, on every
step plan.  fp32 ids are held to the REAL reference's (tests/golden/lm_prompt_greedy.pt) and to the oracle loop of
tests/prompt_reference.py bit for bit; the 16-bit plans to the acceptance rule of the existing 16-bit decode tests
(tests/test_gpu_fp16.py, tests/test_gpu_parity_r03.py: every emitted token is the oracle's arg-max or a tie within 6e-3 (fp16) /
3e-2 (bf16) of the logit range), applied to the fp32 oracle teacher-forced on the GPU's own history."""
import math

import pytest
import torch

import attn_reference as R
import prompt_reference as pr
from conftest import gpu_model, load_golden, synth_sd
from oracle import language_model as o_lm
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = 50256
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def fx():
    return load_golden("lm_prompt_greedy.pt")


def _lm():
    return gpu_model("ragged").language_model


def _search(lm, ids, feats, max_length, mask, **kw):
    return lm.greedy_search(ids.to(DEV), feats.to(DEV), max_length, attention_mask=mask.to(DEV), use_cache=True, **kw).cpu()


def _prompt(S, T, seed, pads=None):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 50000, (S, T), generator=g)
    mask = torch.ones((S, T), dtype=torch.int64)
    if pads is not None:
        for s in range(S):
            p = int(pads[s % len(pads)])
            mask[s, :p] = 0
            ids[s, :p] = EOS
    return ids, mask, torch.randn((S, 1024), generator=g)


def _same_rows(got, ref, rows):
    """ids of ``rows`` of a wide GPU call against a reference run on those rows alone: the rows are independent up to the length at
    which the whole batch has finished, so the common columns are equal and whatever one side has beyond them is PAD."""
    L = min(got.shape[1], ref.shape[1])
    assert torch.equal(got[rows, :L], ref[:, :L]), (got[rows, :L].tolist(), ref[:, :L].tolist())
    assert (got[rows, L:] == EOS).all() and (ref[:, L:] == EOS).all()


# ------------------------------------------------------------------------------------------------ fp32 against the real reference
@pytest.mark.parametrize("case", ["ones_s3_t4", "leftpad_s4_t5", "eos_inside_s3_t4", "one_token_s3_t4"])
def test_fixture_ids_fp32(fx, case):
    c = fx["cases"][case]
    got = _search(_lm(), c["input_ids"], c["feats"], c["max_length"], c["attention_mask"])
    assert got.dtype == torch.int64 and torch.equal(got, c["output_ids"]), (got.tolist(), c["output_ids"].tolist())


def test_fixture_all_rows_finish_early_fp32(fx):
    """wte[EOS] x 1.05: every row emits EOS within two tokens - PAD behind a row's EOS and the early exit, with a prompt."""
    import rgrg_amd
    c = fx["cases"]["allfinish_s4_t3"]
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.load_state_dict(pr.eos_boosted(synth_sd("ragged"), fx["meta"]["eos_boost"]))
    m.to(DEV).eval()
    try:
        got = _search(m.language_model, c["input_ids"], c["feats"], c["max_length"], c["attention_mask"])
    finally:
        m.invalidate_engine()
    assert got.shape[1] < c["max_length"] and torch.equal(got, c["output_ids"]), (got.tolist(), c["output_ids"].tolist())


def test_no_mask_is_refused_like_the_reference(fx):
    """The reference's greedy_search cannot run without model_kwargs['attention_mask'] (recorded in the fixture); same exception type."""
    c, raised = fx["cases"][fx["no_mask"]["case"]], fx["no_mask"]["raised"]
    assert raised is not None and raised["type"] == "AttributeError"
    with pytest.raises(AttributeError):
        _lm().greedy_search(c["input_ids"].to(DEV), c["feats"].to(DEV), c["max_length"], use_cache=True)


def test_prompt_cache_planes_and_last_logits_fp32(fx):
    """The prompt's keys / values in the decode cache (slots 1 .. T, and the image in slot 0) against the oracle's ``past``, and the
    logits of the last prompt position (T = max_length: the only step is the prompt pass) within the tolerance of the cached-forward
    tests (2e-3, tests/test_gpu_lm_forms.py) of the REAL reference's."""
    c = fx["cases"]["leftpad_s4_t5"]
    ids, mask, feats = c["input_ids"], c["attention_mask"], c["feats"]
    S, T = ids.shape
    m = gpu_model("ragged")
    got = _search(m.language_model, ids, feats, T, mask)
    assert got.shape == (S, T + 1) and torch.equal(got[:, :T + 1], c["output_ids"][:, :T + 1])
    eng = m.engine()
    last = eng.last_logits(S).cpu()
    stride = fx["meta"]["probe_stride"]
    assert (last[:, ::stride] - c["last_logits_probe"]).abs().max().item() <= 2e-3
    assert (last[3] - c["last_logits_row3"]).abs().max().item() <= 2e-3
    _, _, past = pr.greedy_search(synth_sd("ragged"), ids, feats, T, mask, return_prompt_pass=True)
    for l in (0, 11, 23):
        for j in (0, 1):
            plane = eng._kv[l, j, :S, :, :T + 1].cpu()
            assert (plane - past[l][j]).abs().max().item() <= 2e-3, (l, j)   # the bound of the presents in tests/test_gpu_lm_forms.py


# ------------------------------------------------------------------------------------------------ a BOS column is generate()
@pytest.mark.parametrize("S", [3, 129])
def test_bos_column_prompt_equals_generate(S):
    lm = _lm()
    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(83)).to(DEV)
    ref = lm.generate(feats, max_length=8)
    bos = torch.full((S, 1), EOS, dtype=torch.int64, device=DEV)
    got = lm.greedy_search(bos, feats, 8, attention_mask=torch.ones((S, 1), dtype=torch.int64, device=DEV), use_cache=True)
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ every step plan, ragged mask
def test_ragged_prompt_many_sequence_fp32():
    """129 rows without autocast: one more than the fused plan takes - tiled fp32 GEMMs, masked fp32 attention, per-row positions."""
    S, T, L = 129, 4, 7
    ids, mask, feats = _prompt(S, T, 91, pads=(0, 1, 3, 2, 0))
    m = gpu_model("ragged")
    got = _search(m.language_model, ids, feats, L, mask)
    assert m.engine().fused_row_limit() == 128 and m.engine().kv_format_in_use(S) == 0
    rows = [0, 1, 2, 3, 31, 32, 127, 128]
    ref = pr.greedy_search(synth_sd("ragged"), ids[rows], feats[rows], L, mask[rows])
    _same_rows(got, ref, rows)


def test_ragged_prompt_longer_than_one_key_chunk_fp32():
    """A prompt of 150 tokens at S = 2: more than the 144 keys of one chunk of attn_decode_kernel (ATT_NI = 9) in every decode step, the
    register kernel with 8 key tiles in the prompt pass."""
    S, T, L = 2, 150, 153
    ids, mask, feats = _prompt(S, T, 93, pads=(0, 5))
    got = _search(_lm(), ids, feats, L, mask)
    ref = pr.greedy_search(synth_sd("ragged"), ids, feats, L, mask)
    assert torch.equal(got, ref), (got[:, T:].tolist(), ref[:, T:].tolist())


_SELF_RULE = {}


def _rule_16bit(got, ids, mask, feats, rows, tie_frac):
    """The acceptance rule of the 16-bit decode tests on the fp32 oracle, teacher-forced on the GPU's own history ``got``: every
    generated token of ``rows`` is the oracle's arg-max at its position, or within tie_frac x logit range of it."""
    T = ids.shape[1]
    hist = got[rows]
    Lh = hist.shape[1]
    am = torch.cat([mask[rows], torch.ones((len(rows), Lh - 1 - T), dtype=torch.int64)], dim=1)
    with torch.no_grad():
        logits, _ = o_lm.lm_forward(synth_sd("ragged"), hist[:, :-1], am, feats[rows], None, pr.positions_from_mask(am))
    pred = logits[:, T - 1:]                      # positions that predicted the generated tokens
    rng = pred.abs().max().item()
    chosen = hist[:, T:]
    done = torch.zeros(len(rows), dtype=torch.bool)
    for k in range(chosen.shape[1]):
        top = pred[:, k].max(-1).values
        margin = top - pred[:, k].gather(-1, chosen[:, k:k + 1]).squeeze(-1)
        bad = (margin > tie_frac * rng) & ~done   # PAD behind a row's EOS is bookkeeping, not a prediction
        print(f"PROMPT16 step={k} max margin {margin[~done].max().item() if (~done).any() else 0.0:.4e} of range {rng:.3f}")
        assert not bad.any(), (k, margin.tolist(), rng)
        done |= chosen[:, k] == EOS
    return rng


@pytest.mark.parametrize("dtype,S,tie", [(torch.float16, 40, 6e-3), (torch.bfloat16, 70, 3e-2), (torch.float16, 70, 6e-3)])
def test_ragged_prompt_16bit_plans(dtype, S, tie):
    """40 rows under fp16 autocast: the fused plan on 16-bit weights (fp32 cache, masked fp32 attention, DX_EMBED_TOKPOS); 70 rows =
    row limit + 6 under bf16 and fp16: the many-sequence 16-bit step - 16-bit cache filled by the prompt pass, the padded-prompt
    variant of attn_decode_kv16_wave_kernel, c_attn's K/V-cache epilogue."""
    T, L = 5, 9
    ids, mask, feats = _prompt(S, T, 97, pads=(0, 2, 4, 1))
    m = gpu_model("ragged")
    with torch.autocast("cuda", dtype=dtype):
        got = _search(m.language_model, ids, feats, L, mask)
        again = _search(m.language_model, ids, feats, L, mask)
        assert m.engine().fused_row_limit() == 64
        assert m.engine().kv_format_in_use(S) == (0 if S <= 64 else (2 if dtype == torch.float16 else 1))
    assert torch.equal(got, again) and torch.equal(got[:, :T], ids) and got.shape[1] <= L
    rows = [0, 1, 2, 3, S - 2, S - 1]
    _rule_16bit(got, ids, mask, feats, rows, tie)
    # the fp32 oracle against itself passes the rule on these seeds (margin 0 everywhere) - checked once
    if "done" not in _SELF_RULE:
        ref = pr.greedy_search(synth_sd("ragged"), ids[rows], feats[rows], L, mask[rows])
        _rule_16bit(ref, ids[rows], mask[rows], feats[rows], list(range(len(rows))), 0.0)
        _SELF_RULE["done"] = True


def test_graph_equals_eager():
    S, T, L = 5, 4, 9
    ids, mask, feats = _prompt(S, T, 101, pads=(0, 2, 1))
    eng = gpu_model("ragged").engine()
    a = eng.greedy_decode_prompted(feats.to(DEV), ids.to(DEV), mask.to(DEV), L, use_graph=True)
    b = eng.greedy_decode_prompted(feats.to(DEV), ids.to(DEV), mask.to(DEV), L, use_graph=False)
    ones = torch.ones_like(mask).to(DEV)
    c = eng.greedy_decode_prompted(feats.to(DEV), ids.to(DEV), ones, L, use_graph=True)
    d = eng.greedy_decode_prompted(feats.to(DEV), ids.to(DEV), ones, L, use_graph=False)
    e = eng.greedy_decode_prompted(feats.to(DEV), ids.to(DEV), None, L, use_graph=False)   # the engine's None = ones
    assert torch.equal(a, b) and torch.equal(c, d) and torch.equal(c, e)


# ------------------------------------------------------------------------------------------------ the masked 16-bit kernel alone
def _p(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("q_only", (0, 1))
@pytest.mark.parametrize("nkeys", (2, 9, 48, 72, 73, 145, 217))
def test_attn_decode_kv16_padded_prompt_variant(nkeys, q_only, fp16):
    """attn_decode_kv16_wave_kernel<false, F16, QONLY, HAS_FIRST> alone against the float64 reference with the additive -1e4 mask
    on slots 1 .. first[s]: shapes (33 rows, 16 heads; one full wave-per-item grid and a capped one) and bound of
    tests/test_gpu_attention_kernels.py::test_attn_decode_kv16.  first = 0 (no padding), 1, the whole prompt but one key, and a
    chunk edge."""
    lib = _hip.load()
    S, H = 33, 16
    D = H * 64
    slots = nkeys + 1
    d = R.decode_inputs(S, H, nkeys, slots, 7000 * nkeys + 10 * fp16 + q_only, False, None, fp16, "half", tile=8 if nkeys < 40 else 72)
    step = d["step"]
    slot = step + 1
    cands = [0, 1, max(0, nkeys - 2), min(max(0, nkeys - 2), 8), min(max(0, nkeys - 2), 72), max(0, nkeys - 2) // 2]
    first = torch.tensor([cands[s % len(cands)] for s in range(S)], dtype=torch.int32)
    kmask = torch.zeros((S, slots))
    for s in range(S):
        kmask[s, 1:1 + int(first[s])] = -10000.0
    Kc, Vc = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])
    r64 = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, step, None, kmask, F64, kv16=fp16)
    r32 = R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, step, None, kmask, F32, kv16=fp16)
    Kb, Vb = d["K"].clone(), d["V"].clone()
    if q_only:
        Kb[:, :, slot], Vb[:, :, slot] = R.rnd16(d["kn"], fp16), R.rnd16(d["vn"], fp16)
        ld = D
        x = d["q"].reshape(S, D).contiguous()
    else:
        ld = 3 * D + 64
        x = torch.zeros(S, ld)
        x[:, :D], x[:, D:2 * D], x[:, 2 * D:3 * D] = d["q"].reshape(S, D), d["kn"].reshape(S, D), d["vn"].reshape(S, D)
    step_dev = torch.tensor([step], dtype=torch.int32, device=DEV)
    xd, fd = x.to(DEV), first.to(DEV)
    outs = []
    for cap in (0, 50):
        K, V = R.to_bits(Kb, fp16).to(DEV), R.to_bits(Vb, fp16).to(DEV)
        out = torch.full((S * D,), math.nan, dtype=F32, device=DEV)
        _hip.check(lib.rgrg_debug_attn_decode_first(_p(xd), ld, _p(K), _p(V), _p(step_dev), _p(out), None, S, H, slots, _p(fd), fp16, q_only,
                                                    cap, None), "rgrg_debug_attn_decode_first")
        torch.cuda.synchronize()
        outs.append(out.cpu().reshape(S, H, 64))
        if not q_only:
            assert torch.equal(R.from_bits(K.cpu(), fp16)[:, :, slot], r64[1].float()) and torch.equal(R.from_bits(V.cpu(), fp16)[:, :, slot], r64[2].float())
    r = R.compare(outs[0], r64[0], r32[0])
    print(f"ATTNPARITY kernel=attn_decode_kv16_first_{'f16' if fp16 else 'bf16'} case=nkeys={nkeys},q_only={q_only} err={r['err']:.3e} "
          f"noise={r['noise']:.3e} bound={r['bound']:.3e} used={r['used']:.3f}")
    assert r["ok"], f"max|got - ref64| = {r['err']:.3e} exceeds {r['bound']:.3e}"
    assert torch.equal(outs[0], outs[1]), "grid capped at 50 workgroups differs"


def test_attn_decode_first_einval():
    lib = _hip.load()
    z = torch.zeros(4 * 6 * 4 * 64, dtype=torch.int16, device=DEV)
    q = torch.zeros(4, 3 * 6 * 64, device=DEV)
    i = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.rgrg_debug_attn_decode_first(_p(q), 3 * 6 * 64, _p(z), _p(z), _p(i), _p(q), None, 4, 6, 4, _p(i), 0, 0, 0, None) != 0   # H % 4
    assert lib.rgrg_debug_attn_decode_first(_p(q), 64, _p(z), _p(z), _p(i), _p(q), None, 4, 4, 4, _p(i), 0, 1, 0, None) != 0           # ld < H * 64
    assert lib.rgrg_debug_attn_decode_first(_p(q), 3 * 6 * 64, _p(z), _p(z), _p(i), _p(q), None, 4, 4, 4, None, 0, 0, 0, None) != 0    # no first


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    m = gpu_model("ragged")
    lm = m.language_model
    ids, mask, feats = _prompt(3, 4, 103)
    idd, md, fd = ids.to(DEV), mask.to(DEV), feats.to(DEV)
    with pytest.raises(ValueError):
        lm.greedy_search(idd, fd, 8, attention_mask=md, use_cache=False)
    with pytest.raises(TypeError):
        lm.greedy_search(idd, fd, 8, attention_mask=md, use_cache=True, position_ids=None)
    with pytest.raises(RuntimeError):                       # "no CPU fallback"
        lm.greedy_search(ids, feats, 8, attention_mask=mask, use_cache=True)
    zero_row = md.clone()
    zero_row[1] = 0
    with pytest.raises(_hip.RgrgHipError, match="zeros only"):
        lm.greedy_search(idd, fd, 8, attention_mask=zero_row, use_cache=True)
    right = md.clone()
    right[2, -1] = 0
    with pytest.raises(_hip.RgrgHipError, match="left padding"):
        lm.greedy_search(idd, fd, 8, attention_mask=right, use_cache=True)
    bad = idd.clone()
    bad[0, 1] = 50257
    with pytest.raises(IndexError):
        lm.greedy_search(bad, fd, 8, attention_mask=md, use_cache=True)
    with pytest.raises(ValueError):
        lm.greedy_search(idd, fd[:2], 8, attention_mask=md, use_cache=True)
    # the e4m3 cache where it would be used (16-bit mode, more rows than the fused plan takes): refused before any work
    ids70, mask70, feats70 = _prompt(70, 3, 105)
    lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with pytest.raises(_hip.RgrgHipError, match="e4m3"):
                lm.greedy_search(ids70.to(DEV), feats70.to(DEV), 6, attention_mask=mask70.to(DEV), use_cache=True)
    finally:
        lm.set_kv_cache_dtype(None)
    assert torch.equal(lm.greedy_search(idd, fd, 6, attention_mask=md, use_cache=True)[:, :4], idd)   # still works afterwards


# ------------------------------------------------------------------------------------------------ the model-level form
def test_generate_from_prompts():
    import rgrg_amd
    m = gpu_model("ragged")
    B, T = 2, 3
    images = synth.make_images(B, 1234).to(DEV)
    g = torch.Generator().manual_seed(107)
    prompts = torch.randint(0, 50000, (B, 29, T), generator=g)
    mask = torch.ones((B, 29, T), dtype=torch.int64)
    mask[:, ::3, 0] = 0
    prompts[:, ::3, 0] = EOS
    prompts, mask = prompts.to(DEV), mask.to(DEV)
    ids, sel, det, cd = m.generate_from_prompts(images, prompts, mask, max_length=7)
    _, sel_g, det_g, cd_g = m.generate(images, max_length=4)
    assert torch.equal(sel, sel_g) and torch.equal(cd, cd_g) and torch.equal(det["top_region_boxes"], det_g["top_region_boxes"])
    _, _, top, cd2 = m.object_detector(images)
    _, feats = m.binary_classifier_region_selection(top, cd2, return_loss=False)
    flat = sel.reshape(-1)
    want = m.language_model.greedy_search(prompts.reshape(B * 29, T)[flat], feats, 7, attention_mask=mask.reshape(B * 29, T)[flat], use_cache=True)
    assert ids.shape[0] == int(sel.sum()) > 0 and torch.equal(ids, want)
    # nothing selected: the -1 of generate()
    sd0 = dict(synth_sd("ragged"))
    sd0["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m0 = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m0.load_state_dict(sd0)
    m0.to(DEV).eval()
    try:
        assert m0.generate_from_prompts(images[:1], prompts[:1], mask[:1], max_length=6) == -1
    finally:
        m0.invalidate_engine()
