"""The reference of tests/det16_reference.py and the bounds of tests/test_gpu_det16_layers.py, checked without a GPU:
  * with rounding switched off, the float64 chain equals oracle.tv013.resnet50_trunk and rpn_head on the synthetic weights to fp32
    accuracy (the oracle runs in fp32);
  * SENSITIVITY: on the inputs the GPU test uses, every named mutation of the reference, stored as a kernel would store it (fp32 and
    16-bit) and pushed through the same judge with the same bounds, leaves the bound in EVERY case it applies to: the small forced-tile
    cases, every one of the detector's 54 convolutions on the teacher-forced inputs, the RoIAlign inputs, fc6;
  * the unmutated float32 evaluation - the noise run - passes its own bound in every case, and no RoIAlign input has a sample so close
    to the out-of-bounds edge that the two evaluations disagree about it (the noise would then be the size of a feature value);
  * rgrg_debug_bf16_tile_choice loads and answers without a GPU: the tiles the issue lists for the detector at batch 32 and batch 2.
"""
import pytest
import torch

import det16_reference as R
from conftest import synth_sd
from oracle import tv013
from rgrg_amd import _hip, synth

F64, F32 = torch.float64, torch.float32
CONV_MUTATIONS = tuple(m for m in R.MUTATIONS if m != "roi_average_from_rounded")


def _image():
    return synth.make_images(1, 1234)


# ------------------------------------------------------------------------------------------------ reference against the oracle
def test_unrounded_float64_chain_is_the_oracles_trunk_and_rpn_head():
    sd = synth_sd("bench")
    img = _image()
    feat, head = R.trunk16_free(sd, img, None, F64)
    want = tv013.resnet50_trunk(sd, R.BB, img)
    obj, reg = tv013.rpn_head(sd, R.RPN, want)
    # the oracle is fp32 through 53 layers: 1e-5 of the range is its own accuracy (test_gpu_kernels holds the fp32 HIP trunk to 1e-4)
    assert float((feat - want).abs().max()) <= 1e-5 * float(want.abs().max())
    want_head = torch.cat([obj, reg], 1)
    assert float((head - want_head).abs().max()) <= 1e-5 * float(want_head.abs().max())
    assert feat.shape == (1, 2048, 16, 16) and head.shape == (1, 800, 16, 16)
    # a channel permutation is the same mathematics
    feat_p, head_p = R.trunk16_free(sd, img, None, F64, perm=1)
    assert float((feat_p - feat).abs().max()) <= 1e-12 * float(feat.abs().max())
    assert float((head_p - head).abs().max()) <= 1e-12 * float(head.abs().max())


def test_chain_has_the_engines_54_convolutions():
    layers = R.chain_layers(synth_sd("bench"))
    assert len(layers) == 54 and [L["name"] for L in layers[-2:]] == ["rpn_conv", "rpn_head"]
    assert sum(1 for L in layers if L.get("role") == "ds") == 4 and sum(1 for L in layers if L["w"].shape[2] == 3) == 17
    assert layers[-1]["w"].shape == (800, 2048, 1, 1) and layers[-1].get("out_f32")


def test_layout_helpers_round_trip():
    x = R.rnd16(torch.randn(2, 64, 3, 5, generator=torch.Generator().manual_seed(1)), True)
    bits = R.nhwc_bits(x, True)
    assert bits.shape == (2, 3, 5, 64) and bits.dtype == torch.int16 and torch.equal(R.nchw_values(bits, True), x)
    w = R.rnd16(torch.randn(4, 64, 3, 3, generator=torch.Generator().manual_seed(2)), False)
    wb = R.weight_bits(w, False)
    assert wb.shape == (4, 3, 3, 64) and float(R.from_bits(wb, False)[1, 2, 0, 7]) == float(w[1, 7, 2, 0])


# ------------------------------------------------------------------------------------------------ sensitivity and self-check
def _verdict_conv(name, applies, evaluate, r64, r32, fp16, kinds):
    """The noise run passes, every applicable mutation fails, for every way the output is stored.  Returns the mutations seen."""
    seen = []
    for out_f32 in kinds:
        own = R.judge(R.stored(r32, fp16, out_f32), r64, r32, fp16, out_f32)
        assert own["ok"], (name, out_f32, own)
    for m in CONV_MUTATIONS:
        if not applies(m):
            continue
        v = evaluate(m)
        for out_f32 in kinds:
            res = R.judge(R.stored(v, fp16, out_f32), r64, r32, fp16, out_f32)
            assert not res["ok"], f"{m} stays inside the bound at {name}, out_f32={out_f32}: {res}"
        seen.append(m)
    return seen


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
def test_small_case_mutations_are_rejected_and_the_noise_run_passes(fp16):
    seen = set()
    for i in range(len(R.SMALL_GEOMS)):
        c = R.small_case(i, fp16)
        r64, r32 = R.case_eval(c, F64), R.case_eval(c, F32)
        seen.update(_verdict_conv(c["name"], lambda m: R.conv_applies(m, c), lambda m: R.case_eval(c, F64, m), r64, r32, fp16, (True, False)))
    assert seen == set(CONV_MUTATIONS), set(CONV_MUTATIONS) - seen


def test_small_cases_cover_what_the_issue_lists():
    G = R.SMALL_GEOMS
    M = [g["B"] * R.out_size(g["H"], g["k"], g["stride"], g["pad"]) * R.out_size(g["W"], g["k"], g["stride"], g["pad"]) for g in G]
    assert any(m % 64 and m % 128 and m > 128 for m in M)
    assert any(R.conv_applies("straddle_reads_next_image", g) for g in G)
    assert any(g["H"] != g["W"] for g in G)
    assert {(g["k"], g["stride"], g["pad"]) for g in G} >= {(3, 1, 1), (3, 2, 1), (1, 1, 0), (1, 2, 0)}
    assert {g["H"] % 2 for g in G if g["k"] == 3 and g["stride"] == 2} == {0, 1}
    assert {g["Cin"] for g in G} == {64, 128, 192} and {g["Cout"] for g in G} == {64, 160, 192}
    assert any(g["k"] ** 2 * g["Cin"] // 64 < 2 for g in G) and any(g["k"] ** 2 * g["Cin"] // 64 == 2 for g in G)   # < stages - 1 tiles
    assert {g["res"] for g in G} == {True, False} and {g["act"] for g in G} == {R.ACT_NONE, R.ACT_RELU}
    assert len(R.TILES) == 12 and len(set(R.TILES)) == 12


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
def test_detector_layer_mutations_are_rejected_and_the_noise_run_passes(fp16):
    """Every one of the 54 convolutions, stored as the detector stores it (16 bit; rpn_head fp32)."""
    sd = synth_sd("bench")
    seen, n = set(), 0
    for rec in R.trunk16_walk(sd, _image(), fp16):
        g = dict(rec, res=rec["r16"] is not None)

        def evaluate(m, rec=rec):
            return R.conv16(rec["x16"], rec["w"], rec["scale"], rec["shift"], rec["r16"], rec["stride"], rec["pad"], rec["act"], fp16, F64, m)
        seen.update(_verdict_conv(rec["name"], lambda m: R.conv_applies(m, g), evaluate, rec["v64"], rec["v32"], fp16, (rec["out_f32"],)))
        n += 1
    assert n == 54
    assert seen == set(CONV_MUTATIONS) - {"h_w_swapped_in_offset", "straddle_reads_next_image"}   # square maps, one image


@pytest.mark.parametrize("name", R.ROI_CASES)
def test_roi_align_mutation_is_rejected_and_no_sample_sits_on_the_edge(name):
    feat, plist = R.roi_case(name)
    rois = R.rois_of(plist)
    r64, r32 = R.roi_align16(feat, rois, 1.0 / 32, None, F64), R.roi_align16(feat, rois, 1.0 / 32, None, F32)   # the same for both types
    for fp16 in (False, True):
        own = R.judge_roi(R.rnd16(r32["maps"].float(), fp16), r32["pooled"].float(), r64, r32, fp16)
        assert all(v["ok"] for v in own.values()), (name, own)
        # interpolation in float32 against float64: a few ulp of a feature value.  A sample the two evaluations disagree about
        # (dead in one, alive in the other) would show as a whole feature value.
        assert own["maps"]["noise"] <= 1e-5 * own["maps"]["max"], (name, own["maps"])
        mut = R.roi_outputs(r64["bins"], fp16, "roi_average_from_rounded")
        res = R.judge_roi(R.rnd16(mut["maps"].float(), fp16), mut["pooled"].float(), r64, r32, fp16)
        assert res["maps"]["ok"] and not res["pooled"]["ok"], (name, fp16, res)


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
def test_fc6_mutation_is_rejected_and_the_noise_run_passes(fp16):
    M = R.FC6_ROWS[0]
    r64, r32 = R.fc6_eval(fp16, M, F64), R.fc6_eval(fp16, M, F32)
    assert R.compare(r32, r64, r32)["ok"]
    res = R.compare(R.fc6_eval(fp16, M, F64, "last_k_tile_dropped").float(), r64, r32)
    assert not res["ok"], res
    assert R.MARGIN == 8.0


# ------------------------------------------------------------------------------------------------ the launcher's tile query
def test_tile_query_answers_without_a_gpu():
    sd = synth_sd("bench")
    lib = _hip.load()
    q = lib.rgrg_debug_bf16_tile_choice
    assert q(0, 64, 64) < 0                                  # RGRG_EINVAL
    assert q(100, 64, 576) == 3 + 16 * 2                     # N <= 64: 128 x 64, 2 stages
    assert q(100, 64, 64) == 3 + 16 * 2
    assert q(512, 1024, 131072) == 2 + 16 * 4 and q(130, 320, 131072) == 2 + 16 * 4
    assert q(6650, 1024, 131072) == 1 + 16 * 2               # fc6 at 8 images
    assert q(162, 160, 64) == 2 + 16 * 2                     # 64 x 64 with 4 stages asked, K = one tile: 2 stages
    b32 = [q(*mnk[1:]) for mnk in R.chain_mnk(sd, 32)]
    b2 = [(mnk[0], q(*mnk[1:])) for mnk in R.chain_mnk(sd, 2)]
    assert len(b32) == 54 and b32.count(1 + 16 * 2) == 42    # batch 32: 128 x 128 with 2 stages for 42 of the 54
    big2 = [n for n, t in b2 if t == 1 + 16 * 2]
    by_name = {L["name"]: L for L in R.chain_layers(sd)}
    assert len(big2) == 4 and all(by_name[n]["w"].shape[2] == 1 and by_name[n]["stride"] == 1 for n in big2)   # batch 2: 4, all 1 x 1, stride 1
    seen = {q(*mnk[1:]) for B in (1, 2, 4, 8, 16, 32) for mnk in R.chain_mnk(sd, B)}
    assert seen <= set(R.TILES) and {1 + 16 * 2, 3 + 16 * 3, 2 + 16 * 3, 2 + 16 * 4, 3 + 16 * 2} <= seen
