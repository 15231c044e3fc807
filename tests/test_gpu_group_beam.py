"""Diverse beam search on the MI355X (rgrg_decoder_group_beam_search[_prompted]; LanguageModel.group_beam_search,
ReportGenerationModel.generate_diverse): beam_group_merge_kernel alone against its contract in numpy float32, bit for bit; one group
against plain beam search, bit for bit, on the fused and the tiled plan; fp32 sequences against the CPU loop of
tests/group_beam_reference.py on the recorded cases (gaps >= 2e-3, recomputed without a GPU by tests/test_group_beam_reference.py);
the 16-bit plans to the thresholds tests/test_gpu_parity_gaps.py puts on 16-bit beams against fp32 beams.  Sixteen beams are covered
by the kernel test only: the CPU loop found no 16-beam case whose gaps an fp32 ranking can be held to."""
import numpy as np
import pytest
import torch

import group_beam_reference as gbr
from conftest import gpu_model, synth_sd
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = PAD = gbr.EOS


def _p(t):
    return t.data_ptr()


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("lam", [0.3, 0.5])
@pytest.mark.parametrize("nb,G", gbr.MERGE_CASES)
def test_group_merge_kernel_bits(nb, G, lam):
    """S = 3 items, V = 50257: scores (as bits), tokens and beams equal ``merge_reference``.  What the inputs contain is asserted
    without a GPU (test_kernel_test_inputs_reach_every_branch)."""
    lib = _hip.load()
    S, K = gbr.MERGE_S, 2 * nb
    d = gbr.merge_inputs(nb, G)
    ref_s, ref_t, ref_b = gbr.merge_reference(d["row_max"], d["row_logsum"], d["top_val"], d["top_tok"], d["beam_scores"], S, nb, G, lam,
                                              gbr.V_MODEL)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
    out_s = torch.full((S, K), float("nan"), dtype=torch.float32, device=DEV)
    out_t = torch.full((S, K), -1, dtype=torch.int32, device=DEV)
    out_b = torch.full((S, K), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    _hip.check(lib.rgrg_debug_beam_group_merge(_p(dev["row_max"]), _p(dev["row_logsum"]), _p(dev["top_val"]), _p(dev["top_tok"]),
                                               _p(dev["beam_scores"]), S, nb, G, lam, gbr.V_MODEL, _p(out_s), _p(out_t), _p(out_b), None),
               "rgrg_debug_beam_group_merge")
    torch.cuda.synchronize()
    got_s, got_t, got_b = out_s.cpu().numpy(), out_t.cpu().numpy(), out_b.cpu().numpy()
    assert np.array_equal(got_t, ref_t), (got_t.tolist(), ref_t.tolist())
    assert np.array_equal(got_b, ref_b), (got_b.tolist(), ref_b.tolist())
    assert np.array_equal(got_s.view(np.int32), ref_s.view(np.int32)), np.abs(got_s - ref_s).max()


# ------------------------------------------------------------------------------------------------ 2. one group is plain beam search
@pytest.mark.parametrize("S", [3, 33])
def test_one_group_equals_generate_num_beams_4(S):
    """3 items: 12 beam rows, the fused plan; 33 items: 132 rows, the tiled fp32 plan.  The group step (beam_group_merge_kernel) and
    the plain beam step (beam_merge_kernel) of the same rows are captured under keys of their own: generate() afterwards replays
    its own."""
    lm = gpu_model("ragged").language_model
    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(84)).to(DEV)
    ref = lm.generate(feats, max_length=8, num_beams=4)
    got = lm.group_beam_search(feats, 8, 4, 1, 0.0)
    assert got.dtype == torch.int64 and torch.equal(got, ref)
    two = lm.group_beam_search(feats, 8, 4, 2, 0.5)            # a group step of the same rows in between
    assert two.shape[0] == S
    assert torch.equal(lm.generate(feats, max_length=8, num_beams=4), ref)
    assert torch.equal(lm.group_beam_search(feats, 8, 4, 1, 0.0), ref)


# ------------------------------------------------------------------------------------------------ 3. fp32 ids equal the CPU loop
def _model_for(name):
    """-> (language model, cleanup): the cached model, or one with the EOS-boosted weights of the case."""
    c = gbr.CASES[name]
    if "eos_boost" not in c:
        return gpu_model(c["profile"]).language_model, lambda: None
    import rgrg_amd
    m = rgrg_amd.ReportGenerationModel(pretrain_without_lm_model=True)
    m.load_state_dict(gbr.case_weights(name, synth_sd))
    m.to(DEV).eval()
    return m.language_model, m.invalidate_engine


def _same_items(got, ref):
    L = min(got.shape[1], ref.shape[1])
    assert torch.equal(got[:, :L], ref[:, :L]), (got[:, :L].tolist(), ref[:, :L].tolist())
    assert (got[:, L:] == PAD).all() and (ref[:, L:] == PAD).all()


@pytest.mark.parametrize("name", ["ragged_s2_b4_g2", "bench_s1_b6_g3", "early_s2_b4_g2", "done_flip_s2_b4_g2"])
def test_recorded_case_fp32(name):
    """num_return_sequences = num_beams: every hypothesis of every item's heap, in order."""
    c = gbr.CASES[name]
    r = gbr.case_reference(name, synth_sd)
    lm, cleanup = _model_for(name)
    try:
        got = lm.group_beam_search(r["feats"].to(DEV), c["L"], c["nb"], c["G"], c["lam"], early_stopping=c["early"],
                                   num_return_sequences=c["nb"]).cpu()
    finally:
        cleanup()
    assert got.dtype == torch.int64 and torch.equal(got, r["seq"]), (got.tolist(), r["seq"].tolist())


# ------------------------------------------------------------------------------------------------ 4. many rows
def test_many_rows_fp32():
    """33 items x 4 beams in 2 groups = 132 rows without autocast (the tiled fp32 plan): items [0, 1, 32] equal the CPU loop run on
    those items alone, up to the padded length."""
    name = "many_s33_b4_g2"
    c = gbr.CASES[name]
    r = gbr.case_reference(name, synth_sd)
    feats, _, _ = gbr.case_inputs(name)
    m = gpu_model(c["profile"])
    nb = c["nb"]
    got = m.language_model.group_beam_search(feats.to(DEV), c["L"], nb, c["G"], c["lam"], num_return_sequences=nb).cpu()
    assert m.engine().kv_format_in_use(feats.shape[0] * nb) == 0
    assert got.shape[0] == feats.shape[0] * nb
    rows = [s * nb + j for s in c["rows"] for j in range(nb)]
    _same_items(got[rows], r["seq"])


# ------------------------------------------------------------------------------------------------ 5. prompts
def test_left_padded_prompt_fp32():
    name = "prompt_s3_t4_b4_g2"
    c = gbr.CASES[name]
    r = gbr.case_reference(name, synth_sd)
    lm = gpu_model(c["profile"]).language_model
    got = lm.group_beam_search(r["feats"].to(DEV), c["L"], c["nb"], c["G"], c["lam"], num_return_sequences=c["nb"],
                               input_ids=r["ids"].to(DEV), attention_mask=r["mask"].to(DEV)).cpu()
    assert torch.equal(got[:, :c["T"]], r["ids"].repeat_interleave(c["nb"], 0))
    assert torch.equal(got, r["seq"]), (got.tolist(), r["seq"].tolist())


def test_bos_prompt_equals_unprompted():
    lm = gpu_model("ragged").language_model
    feats = torch.randn((3, 1024), generator=torch.Generator().manual_seed(86)).to(DEV)
    bos = torch.full((3, 1), EOS, dtype=torch.int64, device=DEV)
    ref = lm.group_beam_search(feats, 8, 4, 2, 0.5, num_return_sequences=4)
    got = lm.group_beam_search(feats, 8, 4, 2, 0.5, num_return_sequences=4, input_ids=bos, attention_mask=torch.ones_like(bos))
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ 6. the 16-bit plans
_FP32_GROUP_BEAMS = {}


@pytest.mark.parametrize("dtype,S", [(torch.float16, 10), (torch.bfloat16, 20), (torch.float16, 20)])
def test_16bit_plans(dtype, S):
    """10 items under fp16: 40 rows, the fused plan; 20 items under bf16 / fp16: 80 rows, the 16-bit cache.  Against the fp32 group
    beams of the same inputs, over the generated columns: the thresholds of tests/test_gpu_parity_gaps.py (16-bit beams against fp32
    beams)."""
    L, nb, G, lam = 11, 4, 2, 0.5
    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(197)).to(DEV)
    m = gpu_model("ragged")
    lm = m.language_model
    if S not in _FP32_GROUP_BEAMS:
        _FP32_GROUP_BEAMS[S] = lm.group_beam_search(feats, L, nb, G, lam).cpu()
    a = _FP32_GROUP_BEAMS[S]
    with torch.autocast("cuda", dtype=dtype):
        b = lm.group_beam_search(feats, L, nb, G, lam).cpu()
        again = lm.group_beam_search(feats, L, nb, G, lam).cpu()
        assert m.engine().fused_row_limit() == 64
        assert m.engine().kv_format_in_use(S * nb) == (0 if S * nb <= 64 else (2 if dtype == torch.float16 else 1))
    assert torch.equal(b, again)
    assert b.dtype == torch.int64 and b.shape[0] == S
    Lc = min(a.shape[1], b.shape[1])
    same = a[:, 1:Lc] == b[:, 1:Lc]
    tok, seq = same.float().mean().item(), same.all(1).float().mean().item()
    print(f"GROUPBEAM16 dtype={dtype} rows={S * nb} tokens equal to the fp32 group beams {tok:.4f} sequences {seq:.4f}")
    assert tok >= 0.85 and seq >= 0.75, (tok, seq)


# ------------------------------------------------------------------------------------------------ 7. model level, refusals on the GPU
def test_generate_diverse():
    m = gpu_model("ragged")
    images = synth.make_images(2, 77).to(DEV)
    out = m.generate_diverse(images, 8, 4, 2, 0.5, early_stopping=True, num_return_sequences=2)
    assert isinstance(out, tuple) and len(out) == 4
    seqs, sel, det, cd = out
    ref = m.generate(images, max_length=8)
    assert torch.equal(sel, ref[1]) and torch.equal(cd, ref[3]) and all(torch.equal(det[k], ref[2][k]) for k in ref[2])
    _, _, top_feats, cd2 = m.object_detector(images)
    _, feats = m.binary_classifier_region_selection(top_feats, cd2, return_loss=False)
    S = feats.shape[0]
    assert S > 0
    direct = m.language_model.group_beam_search(feats, 8, 4, 2, 0.5, early_stopping=True, num_return_sequences=2)
    assert seqs.shape[0] == 2 * S and torch.equal(seqs, direct)
    with pytest.raises(NotImplementedError):
        m.language_model.generate(feats, 8, num_beams=4, num_beam_groups=2)


def test_e4m3_cache_takes_no_prompt():
    lm = gpu_model("ragged").language_model
    S = 20
    feats = torch.randn((S, 1024), generator=torch.Generator().manual_seed(88)).to(DEV)
    ids = torch.randint(0, 50000, (S, 3), generator=torch.Generator().manual_seed(89)).to(DEV)
    lm.set_kv_cache_dtype("fp8_e4m3")
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with pytest.raises(_hip.RgrgHipError, match="e4m3"):
                lm.group_beam_search(feats, 8, 4, 2, 0.5, input_ids=ids, attention_mask=torch.ones_like(ids))   # 80 rows
    finally:
        lm.set_kv_cache_dtype(None)
    got = lm.group_beam_search(feats[:2], 8, 4, 2, 0.5, input_ids=ids[:2], attention_mask=torch.ones_like(ids[:2]))
    assert got.shape[0] == 2 and torch.equal(got[:, :3], ids[:2])
