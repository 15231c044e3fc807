"""CPU references of beam search and sampling FROM A PROMPT.  TEST INFRASTRUCTURE ONLY.

``beam_search``: the loop of ``oracle.language_model.beam_generate`` (language_model.py:529-607 on the restated HF-4.19.2
``BeamSearchScorer``), started from given ids and mask instead of a BOS column: positions come from the mask
(``prepare_inputs_for_generation`` :498-520), the mask grows by a column of ones per step (:522-527), hypothesis lengths and the
``is_done`` length count the prompt, padding included.  ``tests/golden/lm_prompt_beam.pt`` pins it against the real reference.

``sample``: a sampling loop from a prompt over ``oracle.language_model.lm_forward`` and the sampler contract of
``tests/sample_reference.py``: row r draws the token of column c with the Philox counter (r, c - 1)."""
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

import sample_reference as sr
from oracle import language_model as o_lm
from oracle.beam_scorer import BeamSearchScorer
from prompt_reference import positions_from_mask

EOS = PAD = o_lm.EOS


def expand(t: torch.Tensor, num_beams: int) -> torch.Tensor:
    """``_expand_inputs_for_generation`` (:481-490): row s -> rows s * num_beams .. s * num_beams + num_beams - 1."""
    S = t.shape[0]
    return t.index_select(0, torch.arange(S).view(-1, 1).repeat(1, num_beams).view(-1))


@torch.no_grad()
def beam_search(sd, input_ids: torch.Tensor, attention_mask: torch.Tensor, image_hidden_states: torch.Tensor, max_length: int,
                num_beams: int, early_stopping: bool = False, num_return_sequences: int = 1, return_gap: bool = False,
                stop_below: float = 0.0):
    """input_ids / attention_mask [S,T]: ONE prompt per item (expanded here).  -> int64 [S * num_return_sequences, L].
    ``return_gap``: also the smallest difference between adjacent entries of the top 2 * num_beams + 1 candidate scores over every
    step and unfinished item (what a ranking swap would have to overcome); ``stop_below``: give up - (None, gap) - as soon as that
    gap falls below it (the seed walk of tests/golden/make_golden_lm_prompt_beam.py)."""
    S = input_ids.shape[0]
    scorer = BeamSearchScorer(batch_size=S, num_beams=num_beams, length_penalty=1.0, do_early_stopping=early_stopping,
                              num_beam_hyps_to_keep=num_return_sequences)
    ids = expand(input_ids.clone(), num_beams)
    attn = expand(attention_mask.clone().to(torch.int64), num_beams)
    beam_scores = torch.zeros((S, num_beams), dtype=torch.float)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    past, cur_len, gap = None, ids.shape[1], float("inf")
    while True:
        pos = positions_from_mask(attn)
        inp = ids if past is None else ids[:, -1:]
        if past is not None:
            pos = pos[:, -1:]
        logits, past = o_lm._lm_forward_beams(sd, inp, attn, image_hidden_states, past, pos, num_beams, "language_model.")
        scores = F.log_softmax(logits[:, -1, :], dim=-1) + beam_scores[:, None]
        V = scores.shape[-1]
        flat = scores.view(S, num_beams * V)
        if return_gap:
            top = torch.topk(flat, 2 * num_beams + 1, dim=1).values
            live = ~scorer._done
            if live.any():
                gap = min(gap, float((top[live, :-1] - top[live, 1:]).min()))
            if gap < stop_below:
                return None, gap
        scores, tokens = torch.topk(flat, 2 * num_beams, dim=1, largest=True, sorted=True)
        indices = torch.div(tokens, V, rounding_mode="floor")
        tokens = tokens % V
        out = scorer.process(ids, scores, tokens, indices, pad_token_id=PAD, eos_token_id=EOS)
        beam_scores, beam_tok, beam_idx = out["next_beam_scores"], out["next_beam_tokens"], out["next_beam_indices"]
        ids = torch.cat([ids[beam_idx, :], beam_tok.unsqueeze(-1)], dim=-1)
        attn = torch.cat([attn, attn.new_ones((attn.shape[0], 1))], dim=-1)
        past = [(k.index_select(0, beam_idx), v.index_select(0, beam_idx)) for k, v in past]  # _reorder_cache (:492-496)
        cur_len += 1
        if scorer.is_done or (max_length and cur_len >= max_length):
            break
    seq = scorer.finalize(ids, beam_scores, tokens, indices, pad_token_id=PAD, eos_token_id=EOS, max_length=max_length)["sequences"]
    return (seq, gap) if return_gap else seq


@torch.no_grad()
def sample(sd, input_ids: torch.Tensor, attention_mask: torch.Tensor, image_hidden_states: torch.Tensor, max_length: Optional[int],
           seed: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
    """-> (ids int64 [S, L'], log-probs float32 [S, L'], coin flips): the greedy loop of tests/prompt_reference.py with the arg-max
    replaced by ``sample_reference.Row.draw`` at the counter (row, column - 1); log-prob 0 in the prompt columns and for PAD.
    ``coin flips`` counts the draws the sampler contract calls undecidable in fp32 (Row.is_coin_flip): a caller that compares ids
    must see 0."""
    ids = input_ids.clone()
    attn = attention_mask.clone().to(torch.int64)
    S, cur_len = ids.shape
    lps = torch.zeros((S, cur_len), dtype=torch.float32)
    unfinished = torch.ones((S,), dtype=torch.int64)
    past, flips = None, 0
    while True:
        pos = positions_from_mask(attn)
        inp = ids if past is None else ids[:, -1:]
        if past is not None:
            pos = pos[:, -1:]
        logits, past = o_lm.lm_forward(sd, inp, attn, image_hidden_states, past, pos)
        nxt = torch.full((S,), PAD, dtype=torch.int64)
        lp = torch.zeros((S,), dtype=torch.float32)
        for s in range(S):
            if not unfinished[s]:
                continue
            row = sr.Row(logits[s, -1].numpy(), temperature, top_k, top_p)
            flips += int(row.is_coin_flip())
            tok, logp = row.draw(seed, s, cur_len - 1)
            nxt[s], lp[s] = int(tok), float(np.float32(logp))
        ids = torch.cat([ids, nxt[:, None]], dim=-1)
        lps = torch.cat([lps, lp[:, None]], dim=-1)
        attn = torch.cat([attn, attn.new_ones((S, 1))], dim=-1)
        cur_len += 1
        unfinished = unfinished * (nxt != EOS).long()
        if unfinished.max() == 0 or (max_length and cur_len >= max_length):
            break
    return ids, lps, flips


# ---------------------------------------------------------------------- inputs of the kernel test (ancestor table AND padded slots)
BEAM_FIRST_NKEYS = (2, 9, 17, 72, 73, 145, 146, 217)
BEAM_FIRST_S, BEAM_FIRST_H = 33, 16


def beam_first_inputs(nkeys: int, kv16=None):
    """One decode step of S = 33 beam rows (groups of 4, the last group a single row), H = 16, nkeys = step + 2 keys, with an
    ancestor table AND padded prompt slots: ``attn_reference.decode_inputs`` with a table, plus first [S] - constant inside each
    group of 4 rows, cycling over 0, 1, the chunk edges of the kernels (32: fp32 kernel with 2 keys per group; 72: the 16-bit
    kernel; 144: fp32 kernel with 9 keys per group) and nkeys - 2 (every prompt slot padded) - and the additive mask [S,slots]
    built from it.  -> (d, first int32 [S], kmask [S,slots])."""
    import attn_reference as R
    S, H, slots = BEAM_FIRST_S, BEAM_FIRST_H, nkeys + 1
    d = R.decode_inputs(S, H, nkeys, slots, 9100 * nkeys + (0 if kv16 is None else 10 + kv16), True, None, kv16, "half",
                        tile=8 if nkeys < 40 else 72)
    top = nkeys - 2
    cands = [0, 1, min(top, 72), top, min(top, 32), min(top, 144), top // 2]
    first = torch.tensor([cands[(s // 4) % len(cands)] for s in range(S)], dtype=torch.int32)
    kmask = torch.zeros((S, slots))
    for s in range(S):
        kmask[s, 1:1 + int(first[s])] = -10000.0
    return d, first, kmask


def beam_first_reference(d, kmask, dt, kv16=None, src="table"):
    """``attn_reference.decode_forward`` on those inputs (NaN slots of the cache - never read as keys - zeroed)."""
    import attn_reference as R
    K, V = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])
    return R.decode_forward(d["q"], d["kn"], d["vn"], K, V, d["step"], d["src"] if src == "table" else None, kmask, dt, kv16=kv16)
