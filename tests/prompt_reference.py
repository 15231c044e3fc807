"""CPU reference of ``LanguageModel.greedy_search`` with a prompt (language_model.py:609-652 over ``prepare_inputs_for_generation``
:498-520 and ``_update_model_kwargs_for_generation`` :522-527): a plain greedy loop over ``oracle.language_model.lm_forward``.
TEST INFRASTRUCTURE ONLY.  ``tests/golden/lm_prompt_greedy.pt`` pins it against the real reference; the GPU tests use it for the
shapes that fixture does not hold."""
from typing import Optional

import torch

from oracle import language_model as o_lm

EOS = PAD = o_lm.EOS


def positions_from_mask(attention_mask: torch.Tensor) -> torch.Tensor:
    """:506-509: cumsum(mask) - 1, and 1 where the mask is 0."""
    pos = attention_mask.long().cumsum(-1) - 1
    return pos.masked_fill(attention_mask == 0, 1)


@torch.no_grad()
def greedy_search(sd, input_ids: torch.Tensor, image_hidden_states: torch.Tensor, max_length: Optional[int],
                  attention_mask: torch.Tensor, return_prompt_pass: bool = False):
    """-> int64 [S, L'] (prompt in front; PAD behind a row's EOS).  ``return_prompt_pass``: also the logits of the last prompt
    position [S, V] and the ``presents`` of the prompt pass (24 pairs [S,16,1+T,64], the image key / value in slot 0)."""
    ids = input_ids.clone()
    attn = attention_mask.clone().to(torch.int64)
    S, cur_len = ids.shape
    unfinished = torch.ones((S,), dtype=torch.int64)
    past, first = None, None
    while True:
        pos = positions_from_mask(attn)
        inp = ids if past is None else ids[:, -1:]
        if past is not None:
            pos = pos[:, -1:]
        logits, past = o_lm.lm_forward(sd, inp, attn, image_hidden_states, past, pos)
        if first is None:
            first = (logits[:, -1].clone(), [(k.clone(), v.clone()) for k, v in past])
        nxt = torch.argmax(logits[:, -1, :], dim=-1)
        nxt = nxt * unfinished + PAD * (1 - unfinished)
        ids = torch.cat([ids, nxt[:, None]], dim=-1)
        attn = torch.cat([attn, attn.new_ones((S, 1))], dim=-1)
        cur_len += 1
        unfinished = unfinished * (nxt != EOS).long()
        if unfinished.max() == 0 or (max_length and cur_len >= max_length):
            break
    return (ids, first[0], first[1]) if return_prompt_pass else ids


def eos_boosted(sd, factor: float):
    """Weight variant that makes every row finish early: the EOS row of the (tied, aliased) token table scaled by ``factor``."""
    key = "language_model.gpt_with_lm_head.transformer.wte.weight"
    w = sd[key].clone()
    w[EOS] *= factor
    return {k: (w if (v.shape == sd[key].shape and v.data_ptr() == sd[key].data_ptr()) else v) for k, v in sd.items()}
