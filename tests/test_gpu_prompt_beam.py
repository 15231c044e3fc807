"""Beam search and sampling from a prompt on the MI355X (rgrg_decoder_beam_search_prompted / rgrg_decoder_sample_prompted;
LanguageModel.beam_search / sample_from_prompt, ReportGenerationModel.beam_search_from_prompts / sample_from_prompts): one prompt
pass per item whose keys / values every beam row reaches through the ancestor table, on every step plan.  fp32 sequences are held to
the REAL reference's (tests/golden/lm_prompt_beam.pt) and to the CPU loop of tests/prompt_beam_reference.py bit for bit, the 16-bit
plans to the thresholds tests/test_gpu_parity_gaps.py puts on 16-bit beams against fp32 beams, the two new attention variants alone
to the float64 reference of tests/attn_reference.py."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_reference as R
import prompt_beam_reference as pbr
import prompt_reference as pr
import sample_reference as sr
from conftest import gpu_model, load_golden, synth_sd
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = PAD = 50256
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def fx():
    return load_golden("lm_prompt_beam.pt")


def _lm():
    return gpu_model("ragged").language_model


def _scorer(S, nb, early=False, keep=1):
    """What LanguageModel.beam_search reads of a transformers BeamSearchScorer."""
    return SimpleNamespace(num_beams=nb, _beam_hyps=[None] * S, length_penalty=1.0, do_early_stopping=early, num_beam_hyps_to_keep=keep,
                           num_beam_groups=1)


def _beam(lm, ids, mask, feats, max_length, nb, early=False, keep=1):
    """ids / mask [S,T]: one prompt per item, expanded here as the reference's callers do."""
    return lm.beam_search(pbr.expand(ids, nb).to(DEV), feats.to(DEV), max_length, _scorer(ids.shape[0], nb, early, keep),
                          attention_mask=pbr.expand(mask, nb).to(DEV), use_cache=True).cpu()


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


# ------------------------------------------------------------------------------------------------ 1. the real reference's sequences
@pytest.mark.parametrize("case", ["ones_s3_t4_b4", "leftpad_s3_t5_b4", "padded_s2_t4_b3_k2", "one_iter_s3_t4_b4"])
def test_fixture_sequences_fp32(fx, case):
    c = fx["cases"][case]
    got = _beam(_lm(), c["input_ids"], c["attention_mask"], c["feats"], c["max_length"], c["num_beams"], c["early_stopping"],
                c["num_return_sequences"])
    assert got.dtype == torch.int64 and torch.equal(got, c["sequences"]), (got.tolist(), c["sequences"].tolist())


def test_fixture_every_item_finishes_early_fp32(fx):
    import rgrg_amd
    c = fx["cases"]["allfinish_s3_t3_b4"]
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.load_state_dict(pr.eos_boosted(synth_sd("ragged"), fx["meta"]["eos_boost"]))
    m.to(DEV).eval()
    try:
        got = _beam(m.language_model, c["input_ids"], c["attention_mask"], c["feats"], c["max_length"], c["num_beams"],
                    c["early_stopping"], c["num_return_sequences"])
    finally:
        m.invalidate_engine()
    assert got.shape[1] < c["max_length"] and torch.equal(got, c["sequences"]), (got.tolist(), c["sequences"].tolist())


# ------------------------------------------------------------------------------------------------ 2. a BOS column is generate(num_beams)
@pytest.mark.parametrize("S", [3, 33])
def test_bos_column_equals_generate_num_beams_4(S):
    """3 items: 12 beam rows, the fused plan; 33 items: 132 rows, the tiled fp32 plan.  The steps are the captured beam steps of
    generate(num_beams=4); only the first ranking comes from the prompt pass."""
    lm = _lm()
    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(84)).to(DEV)
    ref = lm.generate(feats, max_length=8, num_beams=4)
    bos = torch.full((S, 1), EOS, dtype=torch.int64)
    got = _beam(lm, bos, torch.ones_like(bos), feats, 8, 4)
    assert torch.equal(got, ref.cpu())


# ------------------------------------------------------------------------------------------------ 3. ragged prompt, fp32, 132 rows
def _same_items(got, ref, rows):
    L = min(got.shape[1], ref.shape[1])
    assert torch.equal(got[rows, :L], ref[:, :L]), (got[rows, :L].tolist(), ref[:, :L].tolist())
    assert (got[rows, L:] == PAD).all() and (ref[:, L:] == PAD).all()


def test_ragged_prompt_many_rows_fp32():
    """33 items x 4 beams = 132 rows without autocast: tiled fp32 GEMMs, attn_decode_kernel<true, ., true> (table and mask), per-row
    positions.  Items are independent up to the padded length: the common columns equal the CPU loop run on the items alone."""
    S, T, L = 33, 4, 8
    ids, mask, feats = _prompt(S, T, 191, pads=(0, 1, 3, 2))
    m = gpu_model("ragged")
    got = _beam(m.language_model, ids, mask, feats, L, 4)
    assert m.engine().kv_format_in_use(S * 4) == 0
    assert got.shape[0] == S and torch.equal(got[:, :T], ids)
    rows = [0, 1, 32]
    ref = pbr.beam_search(synth_sd("ragged"), ids[rows], mask[rows], feats[rows], L, 4)
    _same_items(got, ref, rows)


# ------------------------------------------------------------------------------------------------ 4. the 16-bit plans
_FP32_BEAMS = {}


@pytest.mark.parametrize("dtype,S", [(torch.float16, 10), (torch.bfloat16, 20), (torch.float16, 20)])
def test_ragged_prompt_16bit_plans(dtype, S):
    """10 items under fp16: 40 rows, the fused plan on an fp32 cache - attn_decode_kernel<true, 9, true>; 20 items under bf16 / fp16:
    80 rows, the 16-bit cache - attn_decode_kv16_wave_kernel<true, F16, false, true>.  Against the fp32 beams of the same inputs,
    over the generated columns: the thresholds of tests/test_gpu_parity_gaps.py (16-bit beams against fp32 beams)."""
    T, L, nb = 5, 11, 4
    ids, mask, feats = _prompt(S, T, 197, pads=(0, 2, 4, 1))
    m = gpu_model("ragged")
    lm = m.language_model
    if S not in _FP32_BEAMS:
        _FP32_BEAMS[S] = _beam(lm, ids, mask, feats, L, nb)
    a = _FP32_BEAMS[S]
    with torch.autocast("cuda", dtype=dtype):
        b = _beam(lm, ids, mask, feats, L, nb)
        again = _beam(lm, ids, mask, feats, L, nb)
        assert m.engine().fused_row_limit() == 64
        assert m.engine().kv_format_in_use(S * nb) == (0 if S * nb <= 64 else (2 if dtype == torch.float16 else 1))
    assert torch.equal(b, again)
    assert b.dtype == torch.int64 and b.shape[0] == S and torch.equal(b[:, :T], ids) and torch.equal(a[:, :T], ids)
    Lc = min(a.shape[1], b.shape[1])
    same = a[:, T:Lc] == b[:, T:Lc]
    tok, seq = same.float().mean().item(), same.all(1).float().mean().item()
    print(f"PROMPTBEAM16 dtype={dtype} rows={S * nb} tokens equal to the fp32 beams {tok:.4f} sequences {seq:.4f}")
    assert tok >= 0.85 and seq >= 0.75, (tok, seq)


# ------------------------------------------------------------------------------------------------ 5. the two kernel variants alone
def _p(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _run_beam_first(lib, d, first, kv16, ni=0, cap=0):
    """-> (out [S,H,64], K after, V after, K before, V before) with the caches as the kernel's own element type."""
    S, H, slots = d["S"], d["H"], d["slots"]
    D = H * 64
    ld = 3 * D + 64
    x = torch.zeros(S, ld)
    x[:, :D], x[:, D:2 * D], x[:, 2 * D:3 * D] = d["q"].reshape(S, D), d["kn"].reshape(S, D), d["vn"].reshape(S, D)
    K0 = d["K"].clone() if kv16 is None else R.to_bits(d["K"], kv16)
    V0 = d["V"].clone() if kv16 is None else R.to_bits(d["V"], kv16)
    K, V = K0.to(DEV), V0.to(DEV)
    out = torch.full((S * D,), math.nan, dtype=F32, device=DEV)
    step_dev = torch.tensor([d["step"]], dtype=torch.int32, device=DEV)
    src, fd, xd = d["src"].to(DEV).contiguous(), first.to(DEV), x.to(DEV)
    _hip.check(lib.rgrg_debug_attn_decode_beam_first(_p(xd), ld, _p(K), _p(V), _p(step_dev), _p(out), None, S, H, slots, _p(src), _p(fd),
                                                     0 if kv16 is None else 1, int(bool(kv16)), ni, cap, None),
               "rgrg_debug_attn_decode_beam_first")
    torch.cuda.synchronize()
    return out.cpu().reshape(S, H, 64), K.cpu(), V.cpu(), K0, V0


def _check_cache(Ka, Va, K0, V0, slot, kn, vn, kv16):
    """The new k / v are in slot step + 1 exactly (rounded once for a 16-bit cache); every other slot holds the bits it held."""
    if kv16 is None:
        assert torch.equal(Ka[:, :, slot], kn) and torch.equal(Va[:, :, slot], vn)
    else:
        assert torch.equal(R.from_bits(Ka, kv16)[:, :, slot], R.rnd16(kn, kv16)) and torch.equal(R.from_bits(Va, kv16)[:, :, slot], R.rnd16(vn, kv16))
    keep = torch.ones(Ka.shape[2], dtype=torch.bool)
    keep[slot] = False
    assert torch.equal(_bits(Ka)[:, :, keep], _bits(K0)[:, :, keep]) and torch.equal(_bits(Va)[:, :, keep], _bits(V0)[:, :, keep])


@pytest.mark.parametrize("kv16", [None, 0, 1])
@pytest.mark.parametrize("nkeys", pbr.BEAM_FIRST_NKEYS)
def test_attn_decode_beam_first(nkeys, kv16):
    """attn_decode_kernel<true, 9 | 2, true> (kv16 None: the two instantiations give the same bits) and
    attn_decode_kv16_wave_kernel<true, F16, false, true> (bf16 / fp16: the full grid and one capped at 50 workgroups give the same
    bits) against the float64 reference with the ancestor table and the additive -1e4 mask on slots 1 .. first[s], under
    attn_reference.compare's bound.  tests/test_prompt_beam_reference.py shows that these inputs notice a dropped operand."""
    lib = _hip.load()
    d, first, kmask = pbr.beam_first_inputs(nkeys, kv16)
    slot = d["step"] + 1
    r64 = pbr.beam_first_reference(d, kmask, F64, kv16)
    r32 = pbr.beam_first_reference(d, kmask, F32, kv16)
    runs = [_run_beam_first(lib, d, first, kv16, **kw) for kw in ((dict(ni=9), dict(ni=2)) if kv16 is None else (dict(cap=0), dict(cap=50)))]
    for out, Ka, Va, K0, V0 in runs:
        _check_cache(Ka, Va, K0, V0, slot, d["kn"], d["vn"], kv16)
    r = R.compare(runs[0][0], r64[0], r32[0])
    name = "attn_decode_f32_src_mask" if kv16 is None else f"attn_decode_kv16_src_first_{'f16' if kv16 else 'bf16'}"
    print(f"ATTNPARITY kernel={name} case=nkeys={nkeys} err={r['err']:.3e} noise={r['noise']:.3e} bound={r['bound']:.3e} used={r['used']:.3f}")
    assert r["ok"], f"max|got - ref64| = {r['err']:.3e} exceeds {r['bound']:.3e}"
    assert torch.equal(runs[0][0], runs[1][0]), "ni 9 and ni 2 differ" if kv16 is None else "grid capped at 50 workgroups differs"


def test_attn_decode_beam_first_einval():
    lib = _hip.load()
    z = torch.zeros(4 * 6 * 4 * 64, dtype=torch.int16, device=DEV)
    q = torch.zeros(4, 3 * 6 * 64, device=DEV)
    i = torch.zeros(16, dtype=torch.int32, device=DEV)
    f = lib.rgrg_debug_attn_decode_beam_first
    assert f(_p(q), 3 * 6 * 64, _p(z), _p(z), _p(i), _p(q), None, 4, 6, 4, _p(i), _p(i), 1, 0, 0, 0, None) != 0     # H % 4, 16-bit cache
    assert f(_p(q), 3 * 6 * 64, _p(z), _p(z), _p(i), _p(q), None, 4, 6, 4, None, _p(i), 1, 0, 0, 0, None) != 0      # no src
    assert f(_p(q), 3 * 6 * 64, _p(z), _p(z), _p(i), _p(q), None, 4, 6, 4, _p(i), None, 1, 0, 0, 0, None) != 0      # no first
    assert f(_p(q), 64, _p(z), _p(z), _p(i), _p(q), None, 4, 4, 4, _p(i), _p(i), 1, 0, 0, 0, None) != 0             # ld < 3 * H * 64


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    m = gpu_model("ragged")
    lm = m.language_model
    S, T, nb = 3, 4, 4
    ids, mask, feats = _prompt(S, T, 203)
    idx, mx, fd = pbr.expand(ids, nb).to(DEV), pbr.expand(mask, nb).to(DEV), feats.to(DEV)
    sc = _scorer(S, nb)
    differ = idx.clone()
    differ[5, 2] += 1
    with pytest.raises(ValueError, match="beam group"):
        lm.beam_search(differ, fd, 8, sc, attention_mask=mx)
    differ_m = mx.clone()
    differ_m[6, 0] = 0
    with pytest.raises(ValueError, match="beam group"):
        lm.beam_search(idx, fd, 8, sc, attention_mask=differ_m)
    with pytest.raises(ValueError, match="max_length"):
        lm.beam_search(idx, fd, T, sc, attention_mask=mx)
    with pytest.raises(ValueError, match="Batch dimension of 'input_ids' should be 8, but is 12"):
        lm.beam_search(idx, fd, 8, _scorer(2, nb), attention_mask=mx)
    zero_row = mask.clone()
    zero_row[1] = 0
    with pytest.raises(_hip.RgrgHipError, match="zeros only"):
        lm.beam_search(idx, fd, 8, sc, attention_mask=pbr.expand(zero_row, nb).to(DEV))
    right = mask.clone()
    right[2, -1] = 0
    with pytest.raises(_hip.RgrgHipError, match="left padding"):
        lm.beam_search(idx, fd, 8, sc, attention_mask=pbr.expand(right, nb).to(DEV))
    with pytest.raises(_hip.RgrgHipError, match="left padding"):
        lm.sample_from_prompt(ids.to(DEV), fd, 8, attention_mask=right.to(DEV))
    bad = ids.clone()
    bad[0, 1] = 50257
    with pytest.raises(IndexError):
        lm.beam_search(pbr.expand(bad, nb).to(DEV), fd, 8, sc, attention_mask=mx)
    with pytest.raises(IndexError):
        lm.sample_from_prompt(bad.to(DEV), fd, 8, attention_mask=mask.to(DEV))
    with pytest.raises(RuntimeError):                       # "no CPU fallback"
        lm.beam_search(idx.cpu(), feats, 8, sc, attention_mask=mx.cpu())
    with pytest.raises(RuntimeError):
        lm.sample_from_prompt(ids, feats, 8, attention_mask=mask)
    # the e4m3 cache where it would be used (16-bit mode, more rows than the fused plan takes): refused, naming the format
    ids20, mask20, feats20 = _prompt(20, 3, 205)
    ids70, mask70, feats70 = _prompt(70, 3, 207)
    lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with pytest.raises(_hip.RgrgHipError, match="e4m3"):
                _beam(lm, ids20, mask20, feats20, 8, nb)                # 80 rows
            with pytest.raises(_hip.RgrgHipError, match="e4m3"):
                lm.sample_from_prompt(ids70.to(DEV), feats70.to(DEV), 8, attention_mask=mask70.to(DEV))
    finally:
        lm.set_kv_cache_dtype(None)
    got = _beam(lm, ids, mask, feats, 8, nb)                            # a normal call works afterwards
    assert got.shape[0] == S and torch.equal(got[:, :T], ids)


# ------------------------------------------------------------------------------------------------ 7. sampling from a prompt
@pytest.mark.parametrize("S", [5, 129])
def test_sample_top_k_1_equals_greedy_search_fp32(S):
    """5 rows: the fused plan; 129 rows: the tiled fp32 plan, masked fp32 attention."""
    lm = _lm()
    ids, mask, feats = _prompt(S, 4, 211, pads=(0, 1, 3, 2, 0))
    idd, md, fd = ids.to(DEV), mask.to(DEV), feats.to(DEV)
    ref = lm.greedy_search(idd, fd, 9, attention_mask=md, use_cache=True)
    got, lp = lm.sample_from_prompt(idd, fd, 9, attention_mask=md, top_k=1, seed=5, return_logprobs=True)
    assert torch.equal(got, ref)
    assert (lp[:, :4] == 0).all() and (lp <= 0).all()


def test_sample_logprobs_seeds_and_last_draw():
    """temperature 1, no filters, fp32, a ragged prompt: log-probs against log_softmax of the teacher-forced logits on the returned
    history with positions from the mask (2e-3, the bound of tests/test_gpu_sample.py); 0 in the prompt columns; the same seed gives
    the same bits, another seed other draws; the last step's draw is the reference sampler's on the decoder's own last logits."""
    m = gpu_model("ragged")
    lm = m.language_model
    S, T, L = 5, 4, 10
    ids, mask, feats = _prompt(S, T, 213, pads=(0, 2, 1))
    idd, md, fd = ids.to(DEV), mask.to(DEV), feats.to(DEV)
    got, lp = lm.sample_from_prompt(idd, fd, L, attention_mask=md, seed=4, return_logprobs=True)
    logits_last = m.engine().last_logits(S).cpu().numpy()
    assert got.shape == lp.shape and torch.equal(got[:, :T], idd) and (lp[:, :T] == 0).all()
    Lh = got.shape[1]
    am = torch.cat([md, torch.ones((S, Lh - T), dtype=md.dtype, device=DEV)], 1)
    pos = pr.positions_from_mask(am)
    ref = torch.log_softmax(lm.teacher_forced_logits(got, am.float(), fd, position_ids=pos).double(), -1)
    pred = ref[:, T - 1:-1].gather(2, got[:, T:, None])[..., 0]
    live = torch.cat([torch.ones_like(got[:, :1], dtype=torch.bool), (got[:, T:-1] == PAD).cumsum(1) == 0], 1)
    err = (pred - lp[:, T:].double()).abs()[live].max().item()
    print(f"largest |log-prob - teacher-forced log-softmax| behind a ragged prompt: {err:.3e}")
    assert err <= 2e-3, err
    again, lp2 = lm.sample_from_prompt(idd, fd, L, attention_mask=md, seed=4, return_logprobs=True)
    assert torch.equal(got, again) and torch.equal(lp, lp2)
    other = lm.sample_from_prompt(idd, fd, L, attention_mask=md, seed=5)
    assert not torch.equal(other, got)
    # the Philox counter of row r for the token in column c is (r, c - 1)
    g, l = got.cpu().numpy(), lp.cpu().numpy()
    checked = 0
    for s in range(S):
        if (g[s, T:Lh - 1] == PAD).any():
            continue
        ok, why = sr.Row(logits_last[s]).accept(4, s, Lh - 2, g[s, Lh - 1], l[s, Lh - 1])
        assert ok, (s, why)
        checked += 1
    assert checked >= 1


def test_sample_bos_prompt_is_sample_and_row_order():
    """A [S,1] BOS prompt uses sample()'s counters; num_return_sequences = 3 returns rows in order s * 3 + j."""
    lm = gpu_model("bench").language_model
    S = 4
    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(6)).to(DEV)
    bos = torch.full((S, 1), EOS, dtype=torch.int64, device=DEV)
    ones = torch.ones_like(bos)
    a, la = lm.sample(feats, max_length=10, seed=17, return_logprobs=True)
    b, lb = lm.sample_from_prompt(bos, feats, 10, attention_mask=ones, seed=17, return_logprobs=True)
    assert torch.equal(a, b) and (la - lb).abs().max().item() <= 2e-3
    ids, mask, _ = _prompt(S, 3, 215, pads=(0, 1))
    idd, md = ids.to(DEV), mask.to(DEV)
    three = lm.sample_from_prompt(idd, feats, 10, attention_mask=md, num_return_sequences=3, seed=17)
    rep = lm.sample_from_prompt(idd.repeat_interleave(3, 0), feats.repeat_interleave(3, 0), 10, attention_mask=md.repeat_interleave(3, 0), seed=17)
    assert three.shape[0] == 12 and torch.equal(three, rep)
    assert len({tuple(r.tolist()) for r in three[:3]}) > 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sample_autocast_top_k_1_against_greedy_search(dtype):
    """70 rows under autocast: the many-sequence 16-bit step behind a padded prompt, two 16-bit evaluations of the same step - the
    agreement bounds of tests/test_gpu_sample.py (>= 0.95 of the generated tokens under fp16, >= 0.85 under bf16)."""
    lm = gpu_model("bench").language_model
    S, T = 70, 4
    ids, mask, feats = _prompt(S, T, 217, pads=(0, 2, 3, 1))
    idd, md, fd = ids.to(DEV), mask.to(DEV), feats.to(DEV)
    with torch.autocast("cuda", dtype=dtype):
        greedy = lm.greedy_search(idd, fd, 10, attention_mask=md, use_cache=True)
        one = lm.sample_from_prompt(idd, fd, 10, attention_mask=md, top_k=1, seed=31)
    L = min(greedy.shape[1], one.shape[1])
    agree = (greedy[:, T:L] == one[:, T:L]).float().mean().item()
    print(f"top_k = 1 vs greedy_search behind a padded prompt under {dtype}: {agree:.4f} of the generated tokens equal")
    assert torch.equal(one[:, :T], idd)
    assert agree >= (0.95 if dtype == torch.float16 else 0.85) - 1e-6, agree


# ------------------------------------------------------------------------------------------------ 8. model level
def test_report_model_prompted_beam_and_sample():
    m = gpu_model("bench")
    lm = m.language_model
    images = synth.make_images(2, 77).to(DEV)
    T, L, nb = 3, 8, 4
    g = torch.Generator().manual_seed(219)
    rp = torch.randint(0, 50000, (2, 29, T), generator=g)
    rm = torch.ones((2, 29, T), dtype=torch.int64)
    rm[:, ::3, 0] = 0
    rp[:, ::3, 0] = EOS
    rp, rm = rp.to(DEV), rm.to(DEV)
    out = m.beam_search_from_prompts(images, rp, rm, L, nb, early_stopping=True, num_return_sequences=2)
    assert isinstance(out, tuple) and len(out) == 4
    seqs, sel, det, cd = out
    ref = m.generate(images, max_length=L)
    assert torch.equal(sel, ref[1]) and torch.equal(cd, ref[3]) and all(torch.equal(det[k], ref[2][k]) for k in ref[2])
    _, _, top_feats, cd2 = m.object_detector(images)
    sel2, feats = m.binary_classifier_region_selection(top_feats, cd2, return_loss=False)
    flat = sel2.reshape(-1)
    ids, mask = rp.reshape(58, T)[flat], rm.reshape(58, T)[flat]
    S = ids.shape[0]
    assert S > 0 and feats.shape[0] == S
    direct = lm.beam_search(pbr.expand(ids.cpu(), nb).to(DEV), feats, L, _scorer(S, nb, True, 2), attention_mask=pbr.expand(mask.cpu(), nb).to(DEV))
    assert seqs.shape[0] == 2 * S and torch.equal(seqs, direct)
    (sids, slp), sel3, _, _ = m.sample_from_prompts(images, rp, rm, L, top_k=50, seed=3, return_logprobs=True)
    d_ids, d_lp = lm.sample_from_prompt(ids, feats, L, attention_mask=mask, top_k=50, seed=3, return_logprobs=True)
    assert torch.equal(sel3, sel) and torch.equal(sids, d_ids) and torch.equal(slp, d_lp)
    from conftest import synth_sd as _sd
    sd = dict(_sd("bench"))
    sd["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m.load_state_dict(sd)
    m.to(DEV)
    try:
        one = synth.make_images(1, 77).to(DEV)
        assert m.beam_search_from_prompts(one, rp[:1], rm[:1], L, nb) == -1
        assert m.sample_from_prompts(one, rp[:1], rm[:1], L) == -1
    finally:
        m.load_state_dict(_sd("bench"))
        m.to(DEV)
