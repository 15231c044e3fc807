"""Different kinds of decode step at ONE row count on ONE decoder: every kind captures a step graph of its own, keyed by the step's
inputs, and replays it after every other kind has run.  A step that replayed another kind's graph, or that picked up an input another
kind had used (token source, ancestor table, per-row positions, padded slots, slot mask), would decode something else than a decoder
that has run nothing but that kind."""
import time
from types import SimpleNamespace

import pytest
import torch

from conftest import gpu_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EOS = 50256
L, T, NB = 8, 4, 4


def _inputs(rows):
    g = torch.Generator().manual_seed(271)
    feats = torch.randn((rows, 1024), generator=g)
    ids = torch.randint(0, 50000, (rows, T), generator=g)
    mask = torch.ones((rows, T), dtype=torch.int64)
    for s in range(rows):
        p = (0, 1, 3, 2)[s % 4]
        mask[s, :p] = 0
        ids[s, :p] = EOS
    return feats.to(DEV), ids.to(DEV), mask.to(DEV)


def _kinds(lm, rows, diverse_and_sampling):
    """name -> call, in the order of the test; beam kinds take rows / NB items."""
    feats, ids, mask = _inputs(rows)
    S = rows // NB
    scorer = SimpleNamespace(num_beams=NB, _beam_hyps=[None] * S, length_penalty=1.0, do_early_stopping=False, num_beam_hyps_to_keep=1,
                             num_beam_groups=1)
    exp = lambda t: t[:S].repeat_interleave(NB, dim=0)   # noqa: E731 (_expand_inputs_for_generation)
    kinds = {
        "greedy": lambda: (lm.generate(feats, max_length=L),),
        "sampling": lambda: lm.sample(feats, L, seed=7, return_logprobs=True),
        "padded greedy": lambda: (lm.greedy_search(ids, feats, L, attention_mask=mask, use_cache=True),),
        "padded sampling": lambda: lm.sample_from_prompt(ids, feats, L, attention_mask=mask, seed=7, return_logprobs=True),
        "beam": lambda: (lm.generate(feats[:S], max_length=L, num_beams=NB),),
        "diverse beam": lambda: (lm.group_beam_search(feats[:S], L, NB, 2, 0.5),),
        "padded beam": lambda: (lm.beam_search(exp(ids), feats[:S], L, scorer, attention_mask=exp(mask), use_cache=True),),
        "padded diverse beam": lambda: (lm.group_beam_search(feats[:S], L, NB, 2, 0.5, input_ids=ids[:S], attention_mask=mask[:S]),),
    }
    if not diverse_and_sampling:
        kinds = {k: v for k, v in kinds.items() if "diverse" not in k and "sampling" not in k}
    return kinds


@pytest.mark.parametrize("rows,dtype", [(12, None), (132, torch.bfloat16)])
def test_step_kinds_share_one_decoder(rows, dtype):
    """12 rows in fp32: the fused plan, all eight kinds.  132 rows under bfloat16: the 16-bit many-sequence plan - greedy (c_attn
    with the K/V-cache epilogue, q-only attention), padded greedy (padded slots per row), beam and padded beam (ancestor table).
    Reference of a kind: a decoder that has run nothing else.  Then all kinds in order and in reverse on one decoder: the second
    pass replays every graph after every other kind has run.  Bit-equal, the sampler's log-probs included.
    Every kind is bit-repeatable between two new decoders (the references and the first pass are such a pair).
    Measured on the MI355X (the body below, behind the model's creation): 0.56 s for the 12-row case, 0.43 s for the 132-row case."""
    m = gpu_model("ragged")
    lm, eng = m.language_model, m.engine()
    t0 = time.perf_counter()
    with torch.autocast("cuda", dtype=dtype, enabled=dtype is not None):
        kinds = _kinds(lm, rows, diverse_and_sampling=dtype is None)
        ref = {}
        for name, call in kinds.items():
            eng.close()   # the next call creates a new decoder: no graph, no input of another kind
            ref[name] = [t.clone() for t in call()]
        eng.close()
        for name in list(kinds) + list(reversed(kinds)):
            got = kinds[name]()
            assert len(got) == len(ref[name])
            for a, b in zip(got, ref[name]):
                assert a.dtype == b.dtype and torch.equal(a, b), (name, a.tolist(), b.tolist())
        assert eng.kv_format_in_use(rows) == (0 if dtype is None else 1)
        assert (rows <= eng.fused_row_limit()) == (dtype is None)
    torch.cuda.synchronize()
    print(f"STEPKINDS rows={rows} dtype={dtype} kinds={len(kinds)} seconds={time.perf_counter() - t0:.2f}")
