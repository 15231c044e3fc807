"""LanguageModel.sample / ReportGenerationModel.sample on the GPU (synthetic weights): greedy equivalence at top_k = 1, every
last-step draw against the reference sampler on the decoder's own logits, log-prob consistency with the teacher-forced pass,
determinism, and the 16-bit step plans."""
import numpy as np
import pytest
import torch

import sample_reference as sr
from conftest import gpu_model
from rgrg_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 50256


def _feats(S, seed=21):
    return torch.randn((S, 1024), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _accept_last_step(m, ids, lp, seed, T=1.0, k=0, p=1.0):
    """copy_last_logits -> the reference sampler with (seed, row, last step): every unfinished row's last token and log-prob."""
    S, L = ids.shape
    logits = m.engine().last_logits(S).cpu().numpy()
    ids, lp = ids.cpu().numpy(), lp.cpu().numpy()
    checked = 0
    for s in range(S):
        if (ids[s, 1:L - 1] == PAD).any():
            continue   # finished before the last step: PAD, log-prob 0
        row = sr.Row(logits[s], T, k, p)
        if row.is_coin_flip():
            continue
        ok, why = row.accept(seed, s, L - 2, ids[s, L - 1], lp[s, L - 1])
        assert ok, (s, why)
        checked += 1
    return checked


@pytest.mark.parametrize("S", [29, 140])
def test_top_k_1_equals_greedy_fp32(S):
    """29 rows: the fused plan; 140 rows: the many-sequence plan."""
    lm = gpu_model("ragged").language_model
    feats = _feats(S)
    ref = lm.generate(feats, max_length=24)
    ids, lp = lm.sample(feats, max_length=24, top_k=1, seed=5, return_logprobs=True)
    assert torch.equal(ids, ref)                       # same tokens, same PAD, same L' (out_len)
    fin = torch.cat([torch.zeros_like(ids[:, :2], dtype=torch.bool), (ids[:, 1:-1] == PAD).cumsum(1) > 0], 1)
    assert (lp[:, 0] == 0).all() and (lp[fin] == 0).all() and (ids[fin] == PAD).all()   # finished rows: PAD with log-prob 0
    assert (lp <= 0).all()


@pytest.mark.parametrize("S,T,k,p", [(29, 1.0, 0, 1.0), (29, 0.7, 50, 0.9), (140, 1.3, 40, 0.8)])
def test_last_step_draws_are_accepted_and_calls_are_deterministic(S, T, k, p):
    m = gpu_model("bench")
    lm = m.language_model
    feats = _feats(S, 3)
    ids, lp = lm.sample(feats, max_length=12, temperature=T, top_k=k, top_p=p, seed=99, return_logprobs=True)
    assert ids.shape == (S, 12) and ids.dtype == torch.int64 and (ids[:, 0] == PAD).all()
    assert _accept_last_step(m, ids, lp, 99, T, k, p) >= S // 2
    ids2, lp2 = lm.sample(feats, max_length=12, temperature=T, top_k=k, top_p=p, seed=99, return_logprobs=True)
    assert torch.equal(ids, ids2) and torch.equal(lp, lp2)
    eager, lpe = m.engine().sample_decode(feats, 12, T, k, p, 99, use_graph=False)
    assert torch.equal(ids, eager) and torch.equal(lp, lpe)            # graph and eager launches
    other = lm.sample(feats, max_length=12, temperature=T, top_k=k, top_p=p, seed=100)
    assert other.shape == ids.shape and not torch.equal(other, ids)      # another seed, other draws


def test_logprobs_match_the_teacher_forced_pass():
    """temperature 1, no filters, fp32: logprobs[s, t] = log_softmax(teacher-forced logits)[s, t - 1, ids[s, t]].  Tolerance
    2e-3: the bound the existing tests put on BOTH fp32 passes' logits against one oracle (tests/test_gpu_generate.py:34 the
    incremental step, :346 the teacher-forced pass)."""
    lm = gpu_model("ragged").language_model
    feats = _feats(5, 8)
    ids, lp = lm.sample(feats, max_length=12, seed=4, return_logprobs=True)
    am = torch.ones_like(ids, dtype=torch.float32)
    ref = torch.log_softmax(lm.teacher_forced_logits(ids, am, feats).double(), -1)
    got = ref[:, :-1].gather(2, ids[:, 1:, None])[..., 0]
    live = torch.cat([torch.ones_like(ids[:, :1], dtype=torch.bool), (ids[:, 1:-1] == PAD).cumsum(1) == 0], 1)
    err = (got - lp[:, 1:].double()).abs()[live].max().item()
    print(f"largest |log-prob - teacher-forced log-softmax|: {err:.3e}")
    assert err <= 2e-3, err


def test_num_return_sequences_row_order_and_manual_seed():
    lm = gpu_model("bench").language_model
    feats = _feats(4, 6)
    ids3 = lm.sample(feats, max_length=10, num_return_sequences=3, seed=17)
    assert ids3.shape == (12, 10)
    rep = lm.sample(feats.repeat_interleave(3, dim=0), max_length=10, seed=17)          # row s * 3 + j
    assert torch.equal(ids3, rep)
    assert len({tuple(r.tolist()) for r in ids3[:3]}) > 1                               # hypotheses of one input differ
    torch.manual_seed(123)
    a = lm.sample(feats, max_length=10)
    b = lm.sample(feats, max_length=10)
    torch.manual_seed(123)
    assert torch.equal(lm.sample(feats, max_length=10), a) and not torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("S", [40, 116, 928])
def test_autocast_step_plans(S, dtype):
    """40 rows: the fused plan on 16-bit weights; 116 and 928 rows: the many-sequence 16-bit plan.  top_k = 1 against greedy
    under the same autocast are two 16-bit evaluations of the same step: the agreement bound tests/test_gpu_fp16.py:90 uses for
    two 16-bit evaluations (>= 0.95 of the tokens under fp16, >= 0.85 under bf16), over the generated tokens (no BOS column)."""
    m = gpu_model("bench")
    lm = m.language_model
    feats = _feats(S, 12)
    with torch.autocast("cuda", dtype=dtype):
        ids, lp = lm.sample(feats, max_length=8, temperature=0.9, top_k=50, top_p=0.95, seed=31, return_logprobs=True)
        n = _accept_last_step(m, ids, lp, 31, 0.9, 50, 0.95)
        greedy = lm.generate(feats, max_length=8)
        one = lm.sample(feats, max_length=8, top_k=1, seed=31)
    assert ids.shape == (S, 8) and n >= S // 2
    assert one.shape == greedy.shape
    agree = (greedy[:, 1:] == one[:, 1:]).float().mean().item()
    print(f"top_k = 1 vs greedy under {dtype}: {agree:.4f} of the generated tokens equal")
    assert agree >= (0.95 if dtype == torch.float16 else 0.85) - 1e-6, agree


def test_report_model_sample_matches_generate_outside_the_ids():
    m = gpu_model("bench")
    images = synth.make_images(2, 77).to(DEV)
    g = m.generate(images, max_length=8)
    s = m.sample(images, max_length=8, top_k=50, seed=3, return_logprobs=True)
    assert isinstance(s, tuple) and len(s) == 4
    (ids, lp), sel, det, cd = s
    assert torch.equal(sel, g[1]) and torch.equal(cd, g[3])
    assert all(torch.equal(det[k], g[2][k]) for k in g[2])
    assert ids.shape == g[0].shape and lp.shape == ids.shape
    # nothing selected -> -1, as generate() (tests/test_gpu_generate.py::test_generate_returns_minus_one_when_nothing_selected)
    from conftest import synth_sd
    sd = dict(synth_sd("bench"))
    sd["binary_classifier_region_selection.classifier.4.bias"] = torch.tensor([-100.0])
    m.load_state_dict(sd)
    m.to(DEV)
    try:
        assert m.sample(synth.make_images(1, 77).to(DEV), max_length=8) == -1
    finally:
        m.load_state_dict(synth_sd("bench"))
        m.to(DEV)
