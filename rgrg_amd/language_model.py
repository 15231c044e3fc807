"""Host-side mirror of ``src/language_model/language_model.py`` (ttanida/rgrg).

``LanguageModel`` keeps the reference's module tree - and therefore its state-dict keys,
including the three aliased copies of every GPT-2 tensor (``gpt_with_lm_head.transformer.*``,
``gpt.*``, ``gpt2_blocks.N.{0,1,2,3}.*``) and the pseudo-attention buffers - but holds
parameters only.  ``generate`` (language_model.py:401-479) keeps the reference's mode
checks and exceptions; greedy and beam search run on the HIP decoder.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _hip
from ._owner import EngineOwner
from .constants import BOS_TOKEN_ID, EOS_TOKEN_ID, PAD_TOKEN_ID

N_LAYER, D_MODEL, VOCAB, N_POS = 24, 1024, 50257, 1024


class Conv1DWithTrainedWeights(nn.Module):
    """HF Conv1D layout: weight [in,out] (language_model.py:11-29)."""

    def __init__(self, nin: int, nout: int):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(nin, nout), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(nout), requires_grad=False)


class GPT2PseudoAttention(nn.Module):
    def __init__(self):
        super().__init__()
        self.c_attn = Conv1DWithTrainedWeights(D_MODEL, 3 * D_MODEL)
        self.c_proj = Conv1DWithTrainedWeights(D_MODEL, D_MODEL)
        self.embed_dim, self.num_heads, self.head_dim, self.split_size = D_MODEL, 16, 64, D_MODEL
        # buffers of the reference state dict (language_model.py:60-70); the decode kernels need neither:
        # a single-query causal row and the all-ones padding mask are no-ops in greedy generation
        self.register_buffer("causal_mask", torch.tril(torch.ones((N_POS, N_POS), dtype=torch.uint8)).view(1, 1, N_POS, N_POS))
        self.register_buffer("mask_out_value", torch.tensor(-1e4))
        self.uk = nn.Linear(D_MODEL, D_MODEL)
        self.uv = nn.Linear(D_MODEL, D_MODEL)


class GPT2MLP(nn.Module):
    def __init__(self):
        super().__init__()
        self.c_fc = Conv1DWithTrainedWeights(D_MODEL, 4 * D_MODEL)
        self.c_proj = Conv1DWithTrainedWeights(4 * D_MODEL, D_MODEL)


class GPT2Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.ln_1 = nn.LayerNorm(D_MODEL, eps=1e-5)
        self.attn = GPT2PseudoAttention()
        self.ln_2 = nn.LayerNorm(D_MODEL, eps=1e-5)
        self.mlp = GPT2MLP()


class GPT2Transformer(nn.Module):
    def __init__(self):
        super().__init__()
        self.wte = nn.Embedding(VOCAB, D_MODEL)
        self.wpe = nn.Embedding(N_POS, D_MODEL)
        self.drop = nn.Dropout(0.1)
        self.h = nn.ModuleList(GPT2Block() for _ in range(N_LAYER))
        self.ln_f = nn.LayerNorm(D_MODEL, eps=1e-5)


class GPT2LMHeadSkeleton(nn.Module):
    def __init__(self):
        super().__init__()
        self.transformer = GPT2Transformer()
        self.lm_head = nn.Linear(D_MODEL, VOCAB, bias=False)
        self.lm_head.weight = self.transformer.wte.weight  # tied


class _TeacherForcedLoss(torch.autograd.Function):
    """Bridges the HIP training pass into autograd: forward runs loss + gradients in one call
    (rgrg_decoder_lm_loss_grad); backward hands the gradients of the 100 trainable tensors (uk/uv of every layer,
    feature_space_transformation_nn) to autograd, scaled by the incoming gradient."""

    @staticmethod
    def forward(ctx, lm, input_ids, attention_mask, feats, position_ids, *params):
        low = _hip.autocast_mode()
        lm.dropout_seed += 1  # a fresh counter-based stream per pass
        loss, g = lm.engine().lm_loss_grad(feats, input_ids, attention_mask, bf16=low, dropout_p=float(lm.dropout_p),
                                           dropout_seed=lm.pass_dropout_seed(), position_ids=position_ids)
        D, grads = 1024, []
        for l in range(len(lm.gpt.h)):  # same order as LanguageModel.trainable_parameters()
            grads += [g["ukv_w"][(2 * l) * D:(2 * l + 1) * D], g["ukv_b"][(2 * l) * D:(2 * l + 1) * D],
                      g["ukv_w"][(2 * l + 1) * D:(2 * l + 2) * D], g["ukv_b"][(2 * l + 1) * D:(2 * l + 2) * D]]
        grads += [g["fst0_w"], g["fst0_b"], g["fst2_w"], g["fst2_b"]]
        ctx.grads = grads
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        return (None, None, None, None, None) + tuple(g * grad_out for g in ctx.grads)


def check_sample_args(temperature, top_k, top_p, num_return_sequences) -> None:
    """Argument errors of ``sample`` (LanguageModel, ReportGenerationModel): raised before any GPU work."""
    if not temperature > 0:
        raise ValueError(f"temperature has to be > 0, but is {temperature}")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k has to be a non-negative integer (0 = off), but is {top_k}")
    if not (0 < top_p <= 1):
        raise ValueError(f"top_p has to be in (0, 1], but is {top_p}")
    if int(num_return_sequences) != num_return_sequences or num_return_sequences < 1:
        raise ValueError(f"num_return_sequences has to be a positive integer, but is {num_return_sequences}")


def check_group_beam_args(max_length, num_beams, num_beam_groups, diversity_penalty, num_return_sequences) -> None:
    """Argument errors of ``group_beam_search`` (LanguageModel) / ``generate_diverse`` (ReportGenerationModel): raised before any
    GPU work."""
    if max_length is None:
        raise ValueError("max_length has to be set for beam generation.")
    if int(num_beams) != num_beams or num_beams < 2:
        raise ValueError(f"num_beams has to be an integer > 1 for beam search, but is {num_beams}")
    if int(num_beam_groups) != num_beam_groups or num_beam_groups < 1:
        raise ValueError(f"num_beam_groups has to be a positive integer, but is {num_beam_groups}")
    if num_beam_groups > num_beams:
        raise ValueError("'num_beam_groups' has to be smaller or equal to 'num_beams'")
    if num_beams % num_beam_groups != 0:
        raise ValueError("'num_beams' has to be divisible by 'num_beam_groups'")
    if num_beam_groups > 1 and (not isinstance(diversity_penalty, float) or not diversity_penalty > 0.0):
        raise ValueError("'diversity_penalty' has to be a float strictly larger than 0 when 'num_beam_groups' > 1")
    if num_beams > 16:
        raise ValueError(f"diverse beam search ranks at most 16 beams, but num_beams is {num_beams}")
    if int(num_return_sequences) != num_return_sequences or not 1 <= num_return_sequences <= num_beams:
        raise ValueError("'num_return_sequences' has to be between 1 and 'num_beams'.")


def check_beam_sample_args(max_length, num_beams, temperature, top_k, top_p, num_return_sequences) -> None:
    """Argument errors of ``beam_sample`` (LanguageModel) / ``generate_beam_sample`` (ReportGenerationModel): ``check_sample_args``
    plus the beam checks, raised before any GPU work."""
    check_sample_args(temperature, top_k, top_p, num_return_sequences)
    if max_length is None:
        raise ValueError("max_length has to be set for beam generation.")
    if int(num_beams) != num_beams or num_beams < 2:
        raise ValueError(f"num_beams has to be an integer > 1 for beam sampling, but is {num_beams}")
    if num_beams > 16:
        raise ValueError(f"beam sampling ranks at most 16 beams, but num_beams is {num_beams}")
    if num_return_sequences > num_beams:
        raise ValueError("'num_return_sequences' has to be smaller or equal to 'num_beams'.")


def check_rolling_args(max_length, rows) -> None:
    """Argument errors of ``generate_rolling`` (LanguageModel, ReportGenerationModel): raised before any GPU work."""
    if max_length is None:
        raise ValueError("max_length has to be set for rolling-batch generation (it bounds every sequence and the K/V cache).")
    if int(max_length) != max_length or max_length < 2:
        raise ValueError(f"max_length has to be an integer >= 2 (BOS and one generated token), but is {max_length}")
    if max_length > N_POS:
        raise ValueError(f"max_length {max_length} exceeds the {N_POS} positions of the model")
    if rows is not None and (int(rows) != rows or rows < 1):
        raise ValueError(f"rows has to be a positive integer (the decoder rows the sequences flow through), but is {rows}")


def check_rolling_beam_args(max_length, num_beams, rows, num_return_sequences) -> None:
    """Argument errors of ``beam_search_rolling`` (LanguageModel) / ``generate_rolling_beam`` (ReportGenerationModel):
    ``check_rolling_args`` plus the beam checks of ``generate``, raised before any GPU work."""
    check_rolling_args(max_length, rows)
    if int(num_beams) != num_beams or num_beams < 2:
        raise ValueError(f"num_beams has to be an integer > 1 for beam search, but is {num_beams}")
    if rows is not None and rows < num_beams:
        raise ValueError(f"rows has to be at least num_beams (one region slot of {num_beams} decoder rows), but is {rows}")
    if int(num_return_sequences) != num_return_sequences or num_return_sequences < 1:
        raise ValueError(f"num_return_sequences has to be a positive integer, but is {num_return_sequences}")
    if num_return_sequences > num_beams:
        raise ValueError("'num_return_sequences' has to be smaller or equal to 'num_beams'.")


class LanguageModel(EngineOwner):
    _engine_prefix = "language_model."

    def __init__(self):
        super().__init__()
        self.checkpoint = "healx/gpt-2-pubmed-medium"  # not downloaded: weights come from load_state_dict
        self.bos_token_id, self.eos_token_id, self.pad_token_id = BOS_TOKEN_ID, EOS_TOKEN_ID, PAD_TOKEN_ID
        self.gpt_with_lm_head = GPT2LMHeadSkeleton()
        for p in self.gpt_with_lm_head.parameters():
            p.requires_grad = False
        # the reference freezes GPT-2 BEFORE it swaps in GPT2PseudoAttention (language_model.py:207-213, :50-57), so
        # uk / uv (and feature_space_transformation_nn below) are the trainable decoder tensors
        for b in self.gpt_with_lm_head.transformer.h:
            for p in (b.attn.uk.weight, b.attn.uk.bias, b.attn.uv.weight, b.attn.uv.bias):
                p.requires_grad = True
        # the same aliases the reference creates (language_model.py:215-227)
        self.gpt = self.gpt_with_lm_head.transformer
        self.lm_head = self.gpt_with_lm_head.lm_head
        self.wte, self.wpe, self.drop = self.gpt.wte, self.gpt.wpe, self.gpt.drop
        self.final_layernorm = self.gpt.ln_f
        self.gpt2_blocks = nn.ModuleList(nn.ModuleList([b.ln_1, b.attn, b.ln_2, b.mlp]) for b in self.gpt.h)
        self.feature_space_transformation_nn = nn.Sequential(nn.Linear(1024, 1024), nn.ReLU(), nn.Linear(1024, 1024))
        # train-mode dropout of GPT-2 (embd / attention / residual / MLP, all 0.1 in the gpt2-medium config the reference
        # loads).  Counter-based (seed, site, element) masks: same distribution as the reference's, not the same draws.
        # Set dropout_p = 0.0 for a deterministic training pass.
        self.dropout_p = 0.1
        self.dropout_seed = 0x5EED0000

    def forward(self, input_ids: torch.LongTensor, attention_mask: torch.FloatTensor, image_hidden_states: torch.FloatTensor,
                return_loss: bool = False, past_key_values=None, position_ids: Optional[torch.LongTensor] = None,
                use_cache: Optional[bool] = False):
        """Teacher-forced pass of language_model.py:258-399 in eval mode (LM part):
        ``return_loss=True`` -> the scalar language-modelling loss (float32 tensor); ``position_ids`` ([S,T] or [1,T]; default
        arange(T)) are embedded as given - through the token table, the reference's quirk (:293-307).  Like the reference, the
        positions of ``input_ids`` whose ``attention_mask`` is 0 are overwritten with -100 IN PLACE (:371-374),
        and ``return_loss=False, use_cache=False`` returns None (:396-399).  The incremental
        ``use_cache=True`` form belongs to the reference's own generate loop; here ``generate()`` owns the cache.
        In ``train()`` mode with gradients enabled the returned loss carries a ``grad_fn`` (HIP backward pass)."""
        if past_key_values is not None or use_cache:
            return self._forward_cached(input_ids, attention_mask, image_hidden_states, return_loss, past_key_values, position_ids)
        if not return_loss:
            return None
        ids2 = input_ids.view(-1, input_ids.shape[-1])
        am2 = attention_mask.view(ids2.shape[0], -1)
        if self.training and torch.is_grad_enabled():
            # training pass: loss with a grad_fn; loss.backward() fills .grad of uk/uv/feature_space_transformation_nn
            # (what the reference trains in the decoder).  GPT-2's four dropout sites are active with self.dropout_p
            # (0.1 as in the reference; 0 = deterministic), bf16 GEMMs under torch.autocast.
            self.sync_trainable_if_stale()
            loss = _TeacherForcedLoss.apply(self, ids2, am2, image_hidden_states, position_ids, *self.trainable_parameters())
        else:
            self.sync_trainable_if_stale()
            low = _hip.autocast_mode()
            _, loss = self.engine().lm_forward(image_hidden_states, ids2, am2, want_logits=False, want_loss=True, bf16=low,
                                               position_ids=position_ids)
        ids2[~am2.to(torch.bool)] = -100  # the reference's in-place label write (labels IS input_ids)
        return loss

    @torch.no_grad()
    def _forward_cached(self, input_ids, attention_mask, image_hidden_states, return_loss, past_key_values, position_ids):
        """The incremental form (language_model.py:258-366, :396-399): ``forward(..., use_cache=True)`` returns
        ``(lm_logits [S,T,50257], presents)``; ``presents`` - 24 (key, value) pairs [S,16,1+tokens,64], the image key / value
        in slot 0 - are VIEWS of the HIP decoder's pre-allocated cache (a torch tensor), and feeding them back as
        ``past_key_values`` continues on that cache (the reference concatenates new tensors every step).  Round 4:
        ``position_ids`` may be anything the embedding table holds ([S,T] or [1,T]; default, as in the reference :293-304,
        arange(past_length, past_length + T) where past_length counts the image key when a past is given), and a FOREIGN
        ``past_key_values`` (clones, tensors of another model instance) is copied into the cache and continued from.  Still
        raised: stale views of this decoder's own cache (generate() or another call chain has rewritten it since), train mode, a
        loss.  Round 6: an ``attention_mask`` with zeros ([S, past + T], padding inside the prompt or the past) adds the
        reference's -1e4 to the scores of the masked keys (:316-334)."""
        if return_loss or self.training:
            raise NotImplementedError("forward(use_cache=True) is the generation form: eval mode, return_loss=False")
        self.sync_trainable_if_stale()
        ids2 = input_ids.view(-1, input_ids.shape[-1])
        S, T = ids2.shape
        eng = self.engine()
        adopt = None
        if past_key_values is None:
            past = 0
        else:
            past = eng.owns_cache(past_key_values)
            if past is None:
                if eng.aliases_cache(past_key_values):
                    raise NotImplementedError("past_key_values must be the presents returned by the previous forward(use_cache=True) of "
                                              "this model, or independent tensors: these are stale views of the decoder's cache (it has "
                                              "been rewritten since)")
                adopt = past_key_values
                past = int(past_key_values[0][0].shape[-2]) - 1   # slot 0 = the image key
        am = None
        if attention_mask is not None and not bool((attention_mask.reshape(S, -1) != 0).all()):
            am = attention_mask   # padding inside the prompt / the past: the reference's additive -1e4 per masked key (:316-334)
        if position_ids is None and past_key_values is not None:
            # the reference's default counts the image key: arange(past_length, past_length + T), past_length = keys in the cache
            position_ids = torch.arange(past + 1, past + 1 + T).view(1, T)
        return eng.forward_cached(image_hidden_states if (past == 0 and adopt is None) else None, ids2, past, position_ids=position_ids,
                                  adopt_past=adopt, attention_mask=am)

    def trainable_parameters(self):
        """uk/uv of every layer, then feature_space_transformation_nn: the language-model tensors the reference
        leaves trainable (language_model.py:207-213 freezes the rest)."""
        ps = []
        for b in self.gpt.h:
            ps += [b.attn.uk.weight, b.attn.uk.bias, b.attn.uv.weight, b.attn.uv.bias]
        f = self.feature_space_transformation_nn
        return ps + [f[0].weight, f[0].bias, f[2].weight, f[2].bias]

    def pass_dropout_seed(self) -> int:
        """Seed of the current training pass: the per-pass counter, offset per data-parallel rank so that replicas
        draw different masks; rank 0 / no process group = the counter itself."""
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        return int(self.dropout_seed) + (rank << 40)

    def sync_trainable_if_stale(self) -> None:
        """Push optimizer-updated parameters into the engine (cheap version check: torch bumps ``_version`` on every
        in-place update)."""
        ver = tuple(p._version for p in self.trainable_parameters())
        root = self._root()
        eng_existed = root.__dict__.get("_engine") is not None
        eng = self.engine()
        if eng_existed and root.__dict__.get("_trainable_version") != ver:
            eng.sync_trainable(root._full_state_dict())
        root.__dict__["_trainable_version"] = ver

    @torch.no_grad()
    def teacher_forced_logits(self, input_ids: torch.LongTensor, attention_mask: torch.FloatTensor,
                              image_hidden_states: torch.FloatTensor, position_ids: Optional[torch.LongTensor] = None) -> torch.FloatTensor:
        """lm_logits [S,T,50257] of the same pass (what the reference returns next to ``presents``, :398-399)."""
        logits, _ = self.engine().lm_forward(image_hidden_states, input_ids, attention_mask, want_logits=True, want_loss=False,
                                             position_ids=position_ids)
        return logits

    KV_CACHE_DTYPES = (None, "fp8_e4m3")

    def set_kv_cache_dtype(self, name: Optional[str]) -> None:
        """Storage type of the decode K/V cache of ``generate`` (greedy and beam search) and ``sample``: None (default) = the cache
        follows the precision mode; "fp8_e4m3" = plain OCP e4m3fn bytes (no scales; k / v clamped to +-448 and rounded once from
        fp32) wherever the 16-bit cache would be used, i.e. under torch.autocast with more token rows than the fused plans take
        (rgrg_decoder_row_limit(): 64).  WITHOUT autocast, or at fewer rows, the setting has NO effect - the fp32 paths and
        their bit-exactness with the reference do not depend on it.  ``forward(use_cache=True)`` and training are not affected.
        The setting lives on the outermost module (not a parameter or buffer: state dicts are untouched) and survives
        ``load_state_dict`` / ``.to()``.  Any other value raises ValueError."""
        if name not in self.KV_CACHE_DTYPES:
            raise ValueError(f"kv cache dtype must be one of {self.KV_CACHE_DTYPES}, got {name!r}")
        self._root().__dict__["_kv_cache_dtype"] = name

    def kv_cache_dtype(self) -> Optional[str]:
        return self._root().__dict__.get("_kv_cache_dtype")

    def _kv_fp8(self) -> bool:
        return self.kv_cache_dtype() == "fp8_e4m3"

    def _decode_modes(self, device=None) -> dict:
        """What every decode entry does in front of its engine call: "no CPU fallback" for ``device`` (before any engine is built),
        the weights an optimizer step changed since the engine packed them, and -> the ``bf16`` / ``kv_fp8`` arguments of that call."""
        if device is not None:
            from .engine import _require_gpu
            _require_gpu(device)
        self.sync_trainable_if_stale()
        return {"bf16": _hip.autocast_mode(), "kv_fp8": self._kv_fp8()}

    @torch.no_grad()
    def sample(self, image_hidden_states: torch.FloatTensor, max_length: Optional[int] = None, *, temperature: float = 1.0,
               top_k: int = 0, top_p: float = 1.0, num_return_sequences: int = 1, seed: Optional[int] = None,
               return_logprobs: bool = False):
        """Draws from the model's distribution instead of its arg-max (``generate`` keeps raising for ``do_sample=True``, as the
        reference does): int64 ids [S*n, L'] incl. the leading BOS, rows s*n + j for the n = num_return_sequences hypotheses
        of input row s; with ``return_logprobs`` also fp32 [S*n, L'], the log-probability of every token under the
        distribution it was drawn from (0 for BOS and for the PAD of finished rows).  temperature > 0; top_k >= 0 (0 = off)
        and 0 < top_p <= 1 (1 = off) are HF 4.19.2's warpers, top-k first, tied logits kept or dropped together
        (include/rgrg_hip.h "Sampling").  ``seed=None`` draws the seed from torch's CPU generator (``torch.manual_seed``
        governs it); the same seed gives the same ids.  torch.autocast opts into the 16-bit modes as for ``generate``."""
        check_sample_args(temperature, top_k, top_p, num_return_sequences)
        modes = self._decode_modes(image_hidden_states.device)
        if seed is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
        ids, logprobs = self.engine().sample_decode(image_hidden_states, max_length, temperature, int(top_k), top_p, int(seed),
                                                    int(num_return_sequences), **modes)
        return (ids, logprobs) if return_logprobs else ids

    @torch.no_grad()
    def generate_rolling(self, image_hidden_states: torch.FloatTensor, max_length: int, *, rows: Optional[int] = None) -> torch.LongTensor:
        """Greedy search in its serving form: the S rows of ``image_hidden_states`` flow through ``rows`` decoder rows; a row whose
        sentence has ended (EOS, or ``max_length`` tokens) takes the next pending one in the same step.  Same
        return contract as ``generate(num_beams=1)`` - int64 [S, L'], input order, PAD after EOS, L' the longest sentence - and the
        same tokens; the work follows the sum of the sentence lengths instead of S x the longest, and the K/V cache is sized by
        ``rows``, so S may exceed what one ``generate`` call can hold.  ``rows=None`` takes min(S, the rows a cache of
        ``max_length`` tokens can have on this device).  ValueError: ``max_length`` None or < 2, ``rows`` < 1; RgrgHipError: more
        ``rows`` than that cache can have, and ``set_kv_cache_dtype("fp8_e4m3")`` where it would be used (the e4m3 attention kernel
        has no per-row step).  torch.autocast opts into the 16-bit plans by ``rows``, exactly as ``generate`` does by S."""
        check_rolling_args(max_length, rows)
        modes = self._decode_modes(image_hidden_states.device)
        return self.engine().greedy_decode_rolling(image_hidden_states, int(max_length), None if rows is None else int(rows), **modes)

    @torch.no_grad()
    def sample_rolling(self, image_hidden_states: torch.FloatTensor, max_length: int, *, rows: Optional[int] = None,
                       temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, num_return_sequences: int = 1,
                       seed: Optional[int] = None, return_logprobs: bool = False):
        """``sample`` in its serving form: the S*n sentences (n = num_return_sequences per row of ``image_hidden_states``) flow
        through ``rows`` decoder rows as in ``generate_rolling``.  Same return contract as ``sample`` - int64
        [S*n, L'], row s*n + j, BOS first, PAD after EOS, L' the longest sentence; with ``return_logprobs`` also fp32 [S*n, L'].
        Sentence q draws the token of column c from the Philox counter (q, c - 1) under ``seed`` - ``sample``'s counter for its row
        q - so which decoder row decodes a sentence, and when, does not enter the draw: on one step plan (fp32: up to 128 rows, or
        above) the result is ``sample``'s, bit for bit, for every ``rows``.  Across step plans the logits differ by rounding and a
        draw may differ with them.  ``top_k=1`` gives the ids of ``generate_rolling``.  The n hypotheses of a row share its image
        key / value (one prefill row, not n); the K/V cache is sized by ``rows``, so S*n may exceed what one ``sample`` call
        holds.  ``rows=None`` takes min(S*n, the rows a cache of ``max_length`` tokens can have on this device); ``seed=None``
        draws the seed from torch's CPU generator.  Errors: those of ``sample`` and of ``generate_rolling``."""
        check_sample_args(temperature, top_k, top_p, num_return_sequences)
        check_rolling_args(max_length, rows)
        modes = self._decode_modes(image_hidden_states.device)
        if seed is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
        ids, logprobs = self.engine().sample_decode_rolling(image_hidden_states, int(max_length), None if rows is None else int(rows),
                                                            temperature, int(top_k), top_p, int(seed), int(num_return_sequences), **modes)
        return (ids, logprobs) if return_logprobs else ids

    def open_rolling(self, max_length: int, *, rows: int, capacity: Optional[int] = None, do_sample: bool = False,
                     temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, num_return_sequences: int = 1,
                     seed: Optional[int] = None, num_beams: int = 1, early_stopping: bool = False, length_penalty: float = 1.0,
                     max_prompt_length: int = 0):
        """``generate_rolling`` / ``sample_rolling`` (``do_sample``) over an OPEN list: a ``RollingSession`` on
        ``rows`` decoder rows.  ``submit(feats)`` -> the range of sentence numbers q (n = num_return_sequences per feature row, in
        submit order), at any time between steps; ``advance(steps=None)`` runs steps (None: until nothing is unfinished);
        ``collect()`` -> ``(q, ids[, logprobs])`` of every sentence that has ended since, trimmed to its length; ``close()``, or use
        it as a context manager.  Sentence q gets the tokens ``generate`` (the draws ``sample_rolling``: counter (q, c - 1)) gives
        it.  ``capacity``: the feature rows held at a time (None: 4 * rows sentences); a submit beyond it raises RgrgHipError
        until sentences in front have been collected.  Precision and step plan are those of ``rows`` under the autocast state of
        THIS call.  Argument errors (ValueError, before any device work) are those of ``generate_rolling`` / ``sample_rolling``,
        ``rows`` is required; any other decode call on the model makes the session stale (RgrgHipError "stale").
        What is given HERE holds for every submit that says nothing else: ``submit(feats, max_length=.., temperature=.., top_k=..,
        top_p=.., seed=.., stop_token_ids=..)`` decodes its sentences with parameters of their own and ``cancel(qs)`` cuts
        submitted sentences (not in a beam session).
        ``max_prompt_length`` > 0 (not in a beam session, below ``max_length``): ``submit(feats, prompt_ids=..)``
        continues prompts of up to that many tokens - int64 [m, P] or [P], one P per submit, no padding, ``max_length`` counting
        the prompt - as ``greedy_search`` continues ``input_ids`` under a mask of ones; ragged prompts are separate submits.  The
        rings that hold the prompts are allocated here (RgrgHipError naming their size when they do not fit).  0: no prompts,
        nothing allocated, the session as it was.
        ``num_beams > 1``: ``beam_search_rolling`` over an open list -> a ``RollingBeamSession`` on
        ``rows // num_beams`` slots.  ``submit(feats)`` -> the range of REGION numbers, one per feature row; ``collect()`` ->
        ``(q, ids)`` with ids int64 [num_return_sequences, L_q], the rows ``generate(num_beams=..)`` gives the region.  ``capacity``
        counts regions (None: 4 * (rows // num_beams)).  Argument errors are those of ``beam_search_rolling``; ``do_sample``
        with beams raises ValueError (beam-sampling has no session)."""
        from .rolling_session import check_max_prompt_length
        if num_beams != 1:
            if do_sample:
                raise ValueError("do_sample has to be False with num_beams > 1: beam-sampling has no rolling session")
            check_rolling_beam_args(max_length, num_beams, rows, num_return_sequences)
            check_max_prompt_length(max_prompt_length, max_length, beam=True)
            if rows is None:
                raise ValueError("rows has to be given for a rolling session (the decoder rows the regions flow through)")
            if capacity is not None and (int(capacity) != capacity or capacity < 1):
                raise ValueError(f"capacity has to be a positive integer (the regions the session holds at a time), but is {capacity}")
            modes = self._decode_modes(next(self.parameters()).device)
            beam = dict(num_beams=int(num_beams), early_stopping=bool(early_stopping), length_penalty=float(length_penalty),
                        num_return_sequences=int(num_return_sequences))
            return self.engine().open_rolling(int(max_length), int(rows), None if capacity is None else int(capacity), beam=beam, **modes)
        if do_sample:
            check_sample_args(temperature, top_k, top_p, num_return_sequences)
        elif num_return_sequences != 1:
            raise ValueError("num_return_sequences has to be 1 without do_sample (greedy search has one hypothesis per row)")
        check_rolling_args(max_length, rows)
        mp = check_max_prompt_length(max_prompt_length, max_length)
        if rows is None:
            raise ValueError("rows has to be given for a rolling session (the decoder rows the sentences flow through)")
        if capacity is not None and (int(capacity) != capacity or capacity < 1):
            raise ValueError(f"capacity has to be a positive integer (the feature rows the session holds at a time), but is {capacity}")
        modes = self._decode_modes(next(self.parameters()).device)
        sample = None
        if do_sample:
            if seed is None:
                seed = int(torch.empty((), dtype=torch.int64).random_().item())
            sample = dict(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), seed=int(seed),
                          num_return_sequences=int(num_return_sequences))
        return self.engine().open_rolling(int(max_length), int(rows), None if capacity is None else int(capacity), sample=sample,
                                          max_prompt_length=mp, **modes)

    @torch.no_grad()
    def beam_search_rolling(self, image_hidden_states: torch.FloatTensor, max_length: int, num_beams: int, *, rows: Optional[int] = None,
                            early_stopping: bool = False, length_penalty: float = 1.0, num_return_sequences: int = 1) -> torch.LongTensor:
        """Beam search in its serving form: the S regions of ``image_hidden_states`` flow through
        ``G = rows // num_beams`` slots of ``num_beams`` consecutive decoder rows (``rows`` counts decoder rows); a region whose scorer
        is done, or whose hypotheses have ``max_length`` tokens, leaves and its slot takes the next pending region in the same step.
        The return of ``generate(num_beams=..)`` - int64 [S * num_return_sequences, L], the same ids, the same padded width L, the
        same order - on one step plan (fp32: up to 128 rows, or above) bit for bit; the work follows the sum of the regions'
        iterations instead of S x the slowest region, and the K/V cache is sized by ``rows``.  ``rows=None`` takes min(S, the rows
        a cache of ``max_length`` tokens can have on this device // num_beams) slots.  ValueError: ``max_length`` None or < 2,
        ``num_beams`` < 2, ``rows`` < ``num_beams``, ``num_return_sequences`` outside 1 .. ``num_beams``; RgrgHipError: more ``rows``
        than that cache can have, and ``set_kv_cache_dtype("fp8_e4m3")`` where it would be used (the e4m3 attention kernel has no
        per-row step).  torch.autocast opts into the 16-bit plans by the rows in use, as ``generate`` does by S * num_beams."""
        check_rolling_beam_args(max_length, num_beams, rows, num_return_sequences)
        modes = self._decode_modes(image_hidden_states.device)
        return self.engine().beam_search_rolling(image_hidden_states, int(max_length), int(num_beams), None if rows is None else int(rows),
                                                 bool(early_stopping), float(length_penalty), int(num_return_sequences), **modes)

    @torch.no_grad()
    def greedy_search(self, input_ids: torch.LongTensor, image_hidden_states: torch.FloatTensor, max_length: Optional[int],
                      **model_kwargs) -> torch.LongTensor:
        """language_model.py:609-652 with a prompt: continues ``input_ids`` [S,T] greedily and returns int64 [S, L'], the prompt in
        front, PAD behind a row's EOS; ``cur_len`` starts at T, one token is always produced, the loop ends at
        ``cur_len >= max_length`` or when every row has emitted EOS among its GENERATED tokens.  ``model_kwargs`` are the
        reference's: ``attention_mask`` [S,T] (zeros = LEFT padding; positions are ``cumsum(mask) - 1`` per row as in
        ``prepare_inputs_for_generation``, :498-520, padded keys stay masked in every later step) and ``use_cache`` (anything
        but True raises ValueError: the reference's loop feeds one token per step, which needs the cache); any other keyword
        raises TypeError.  ``attention_mask`` is REQUIRED, as it is in the reference - its ``forward`` dereferences the mask
        (:281) and ``_update_model_kwargs_for_generation`` indexes it (:524), so a call without one fails there with the
        AttributeError raised here.  The prompt is run as ONE batched pass into the decode cache;
        torch.autocast opts into the 16-bit plans exactly as for ``generate``.  A BOS column with a mask of ones IS
        ``generate()``."""
        attention_mask = self._prompt_kwargs("greedy_search", model_kwargs)
        modes = self._decode_modes(image_hidden_states.device)
        return self.engine().greedy_decode_prompted(image_hidden_states, input_ids, attention_mask, max_length, **modes)

    @staticmethod
    def _prompt_kwargs(name: str, model_kwargs: dict):
        """The ``model_kwargs`` rules of ``greedy_search``, for ``name``: -> attention_mask."""
        unknown = set(model_kwargs) - {"attention_mask", "use_cache"}
        if unknown:
            raise TypeError(f"{name}() got an unexpected keyword argument {sorted(unknown)[0]!r}")
        if model_kwargs.get("use_cache", True) is not True:
            raise ValueError(f"{name} needs use_cache=True: its loop feeds one token per step on top of the cached keys / values")
        attention_mask = model_kwargs.get("attention_mask")
        if attention_mask is None:
            raise AttributeError(f"'NoneType' object has no attribute 'to' ({name} needs model_kwargs['attention_mask'], like the "
                                 "reference's forward, language_model.py:281)")
        return attention_mask

    @torch.no_grad()
    def beam_search(self, input_ids: torch.LongTensor, image_hidden_states: torch.FloatTensor, max_length: int, beam_scorer,
                    **model_kwargs) -> torch.LongTensor:
        """language_model.py:529-607 with a prompt: ``input_ids`` and ``model_kwargs['attention_mask']`` are [S*num_beams, T],
        expanded as ``_expand_inputs_for_generation`` (:481-490) leaves them (the num_beams rows of an item equal; zeros = LEFT
        padding), ``image_hidden_states`` is [S,1024].  Returns int64 [S * num_beam_hyps_to_keep, L], the prompt in front.
        ``beam_scorer`` (a transformers-4.19.2 ``BeamSearchScorer`` or anything with its attributes) is READ, not called:
        ``num_beams``, ``len(_beam_hyps)``, ``length_penalty``, ``do_early_stopping`` and ``num_beam_hyps_to_keep`` are taken
        from it and the search runs on the decoder's own restatement of the scorer - ITS STATE IS NOT UPDATED (no hypotheses are
        added to it, ``is_done`` stays what it was); ``num_beam_groups > 1`` raises ValueError.  Hypothesis lengths count the
        prompt, padding included, as the reference's do.  ``max_length >= T + 1`` is required (ValueError: the scorer's
        ``finalize`` cannot hold a longer hypothesis).  Rows of a group that differ in ids or in mask raise ValueError: the prompt
        runs ONCE per item, as S x T token rows whose keys / values every beam reaches through the ancestor table (DESIGN.md
        7.10).  ``model_kwargs`` follow ``greedy_search``: the mask is required (AttributeError), ``use_cache`` must be True, any
        other keyword raises TypeError.  torch.autocast opts into the 16-bit plans as for ``generate``."""
        attention_mask = self._prompt_kwargs("beam_search", model_kwargs)
        if getattr(beam_scorer, "num_beam_groups", 1) > 1:
            raise ValueError("beam_search takes a scorer with num_beam_groups = 1: diverse beam search is not implemented")
        batch_size = len(beam_scorer._beam_hyps)
        num_beams = int(beam_scorer.num_beams)
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [S * num_beams, T], got {tuple(input_ids.shape)}")
        batch_beam_size, T = input_ids.shape
        if num_beams * batch_size != batch_beam_size:
            raise ValueError(f"Batch dimension of 'input_ids' should be {num_beams * batch_size}, but is {batch_beam_size}.")
        if tuple(attention_mask.shape) != (batch_beam_size, T):
            raise ValueError(f"attention_mask has shape {tuple(attention_mask.shape)}, input_ids {(batch_beam_size, T)}")
        if int(max_length) < T + 1:
            raise ValueError(f"max_length has to be at least {T + 1} for a prompt of {T} tokens, but is {max_length}")
        from .engine import _require_gpu
        _require_gpu(image_hidden_states.device)   # "no CPU fallback", before any engine is built
        _require_gpu(input_ids.device)
        _require_gpu(attention_mask.device)
        ids3 = input_ids.reshape(batch_size, num_beams, T)
        am3 = attention_mask.reshape(batch_size, num_beams, T)
        # one device comparison per call: the shared prompt pass needs the rows of a group equal
        if bool(((ids3 != ids3[:, :1]).any() | (am3 != am3[:, :1]).any())):
            raise ValueError("the num_beams rows of a beam group differ in input_ids or attention_mask: beam_search runs one prompt "
                             "per item (expand the prompts with _expand_inputs_for_generation)")
        return self._beam_search_prompts(ids3[:, 0], am3[:, 0], image_hidden_states, int(max_length), num_beams,
                                         bool(beam_scorer.do_early_stopping), float(beam_scorer.length_penalty),
                                         int(beam_scorer.num_beam_hyps_to_keep))

    def _beam_search_prompts(self, prompts, mask, image_hidden_states, max_length, num_beams, early_stopping, length_penalty, keep):
        """``beam_search`` on unexpanded prompts [S,T] (one per item)."""
        modes = self._decode_modes()
        return self.engine().beam_search_prompted(image_hidden_states, prompts, mask, max_length, num_beams, early_stopping,
                                                  length_penalty, num_return_sequences=keep, **modes)

    @torch.no_grad()
    def group_beam_search(self, image_hidden_states: torch.FloatTensor, max_length: int, num_beams: int, num_beam_groups: int,
                          diversity_penalty: float, *, early_stopping: bool = False, num_return_sequences: int = 1,
                          length_penalty: float = 1.0, input_ids: Optional[torch.LongTensor] = None,
                          attention_mask: Optional[torch.Tensor] = None) -> torch.LongTensor:
        """Diverse beam search (transformers 4.19.2 ``group_beam_search`` with ``HammingDiversityLogitsProcessor``; ``generate`` keeps
        raising for ``num_beam_groups > 1``, as the reference does): the ``num_beams`` beams of an item form ``num_beam_groups``
        groups that are ranked in order within every step, each group's candidates lowered by ``diversity_penalty`` times the number
        of beams of the earlier groups that took the same token in that step (arithmetic contract in
        include/rgrg_hip.h).  Returns int64 [S * num_return_sequences, L]: the best hypotheses of the item's heap overall (best
        first), NOT one per group.  ``input_ids`` / ``attention_mask`` [S,T] hold ONE prompt per item, unexpanded (zeros = LEFT
        padding, the rules of ``greedy_search``); both or neither; without them the search starts from BOS.  The prompt runs once
        per item, as in ``beam_search``.  ``num_beam_groups = 1`` applies no penalty and IS plain beam search.  ValueError:
        ``num_beams`` not divisible by ``num_beam_groups`` or smaller than it; ``num_beam_groups > 1`` with a ``diversity_penalty``
        that is not a float > 0 (HF's rule); ``num_beams > 16`` (the K-round "wide" ranking kernels of more than 16 beams are not
        extended to groups); ``num_return_sequences`` outside 1 .. ``num_beams``; ``max_length`` None.  torch.autocast opts into
        the 16-bit plans as for ``generate``."""
        check_group_beam_args(max_length, num_beams, num_beam_groups, diversity_penalty, num_return_sequences)
        if (input_ids is None) != (attention_mask is None):
            raise ValueError("input_ids and attention_mask have to be given together (one prompt per item), or neither")
        if input_ids is not None and int(max_length) < input_ids.shape[-1] + 1:
            raise ValueError(f"max_length has to be at least {input_ids.shape[-1] + 1} for a prompt of {input_ids.shape[-1]} tokens, "
                             f"but is {max_length}")
        modes = self._decode_modes(image_hidden_states.device)
        if input_ids is None:
            return self.engine().group_beam_search(image_hidden_states, int(max_length), int(num_beams), int(num_beam_groups),
                                                   float(diversity_penalty), bool(early_stopping), float(length_penalty),
                                                   num_return_sequences=int(num_return_sequences), **modes)
        return self.engine().group_beam_search_prompted(image_hidden_states, input_ids, attention_mask, int(max_length), int(num_beams),
                                                        int(num_beam_groups), float(diversity_penalty), bool(early_stopping),
                                                        float(length_penalty), num_return_sequences=int(num_return_sequences), **modes)

    @torch.no_grad()
    def beam_sample(self, image_hidden_states: torch.FloatTensor, max_length: int, num_beams: int, *, temperature: float = 1.0,
                    top_k: int = 0, top_p: float = 1.0, seed: Optional[int] = None, early_stopping: bool = False,
                    num_return_sequences: int = 1, length_penalty: float = 1.0, input_ids: Optional[torch.LongTensor] = None,
                    attention_mask: Optional[torch.Tensor] = None) -> torch.LongTensor:
        """Beam-search sampling (transformers' ``beam_sample``; ``generate`` keeps raising for ``do_sample=True`` with
        ``num_beams > 1``, as the reference does): beam search whose every step DRAWS the item's 2 * ``num_beams`` candidates
        without replacement from the joint distribution over its ``num_beams`` x vocabulary continuations - log-probabilities
        warped by ``temperature`` / ``top_k`` / ``top_p`` (at least two tokens per row are kept), then the beam score added
        (contract in include/rgrg_hip.h).  Scorer, early stopping, length penalty and ``num_return_sequences``
        are beam search's.  Returns int64 [S * num_return_sequences, L], best hypothesis first.  ``seed=None`` draws the seed from
        torch's CPU generator (``torch.manual_seed`` governs it); the same seed gives the same ids.  ``input_ids`` /
        ``attention_mask`` [S,T] hold ONE prompt per item, unexpanded, as in ``group_beam_search``; both or neither.
        ValueError: the errors of ``sample``; ``num_beams`` outside 2 .. 16; ``num_return_sequences > num_beams``; ``max_length``
        None or smaller than T + 1.  torch.autocast and ``set_kv_cache_dtype`` act as for ``generate``."""
        check_beam_sample_args(max_length, num_beams, temperature, top_k, top_p, num_return_sequences)
        if (input_ids is None) != (attention_mask is None):
            raise ValueError("input_ids and attention_mask have to be given together (one prompt per item), or neither")
        if input_ids is not None and int(max_length) < input_ids.shape[-1] + 1:
            raise ValueError(f"max_length has to be at least {input_ids.shape[-1] + 1} for a prompt of {input_ids.shape[-1]} tokens, "
                             f"but is {max_length}")
        modes = self._decode_modes(image_hidden_states.device)
        if seed is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
        args = (int(max_length), int(num_beams), float(temperature), int(top_k), float(top_p), int(seed), bool(early_stopping),
                float(length_penalty))
        if input_ids is None:
            return self.engine().beam_sample(image_hidden_states, *args, num_return_sequences=int(num_return_sequences), **modes)
        return self.engine().beam_sample_prompted(image_hidden_states, input_ids, attention_mask, *args,
                                                  num_return_sequences=int(num_return_sequences), **modes)

    @torch.no_grad()
    def sample_from_prompt(self, input_ids: torch.LongTensor, image_hidden_states: torch.FloatTensor, max_length: Optional[int] = None,
                           *, attention_mask: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                           num_return_sequences: int = 1, seed: Optional[int] = None, return_logprobs: bool = False):
        """``sample`` that continues ``input_ids`` [S,T] (``attention_mask`` [S,T], zeros = LEFT padding, with the rules of
        ``greedy_search``): int64 ids [S*n, L'] with the prompt in front, rows s*n + j for the n = num_return_sequences hypotheses
        of row s; with ``return_logprobs`` also fp32 [S*n, L'], 0 in the prompt columns and for the PAD of finished rows.  One
        token is always produced; ``max_length`` is ``greedy_search``'s.  Row r draws the token of column c from the Philox
        counter (r, c - 1) under ``seed``, so a BOS column with a mask of ones IS ``sample()``."""
        check_sample_args(temperature, top_k, top_p, num_return_sequences)
        if attention_mask is None:
            raise AttributeError("'NoneType' object has no attribute 'to' (sample_from_prompt needs attention_mask, like the "
                                 "reference's forward, language_model.py:281)")
        modes = self._decode_modes(image_hidden_states.device)
        if seed is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
        ids, logprobs = self.engine().sample_decode_prompted(image_hidden_states, input_ids, attention_mask, max_length, temperature,
                                                             int(top_k), top_p, int(seed), int(num_return_sequences), **modes)
        return (ids, logprobs) if return_logprobs else ids

    @torch.no_grad()
    def generate(self, image_hidden_states: torch.FloatTensor, max_length: Optional[int] = None, num_beams: int = 1,
                 num_beam_groups: int = 1, do_sample: bool = False, num_return_sequences: int = 1,
                 early_stopping: bool = False) -> torch.LongTensor:
        """Same contract as language_model.py:401-479: int64 [S, L'] incl. the leading BOS."""
        # same mode table, exceptions and messages as the reference's generate() (language_model.py:422-479)
        if image_hidden_states.is_cuda:
            self.sync_trainable_if_stale()  # weights changed by an optimizer step since the engine packed them
        single_group = num_beam_groups == 1
        if num_beam_groups > num_beams:
            raise ValueError("'num_beam_groups' has to be smaller or equal to 'num_beams'")
        if num_beams > 1 and not single_group and do_sample is True:
            raise ValueError("Diverse beam search cannot be used in sampling mode. Make sure that 'do_sample' is set to 'False'.")
        if num_beams == 1 and single_group:
            if do_sample is True:
                raise NotImplementedError("Multinomial sampling is not implemented.")
            if num_return_sequences > 1:
                raise ValueError(f"num_return_sequences has to be 1, but is {num_return_sequences} when doing greedy search.")
            # like the reference's scripts, callers may wrap generate() in torch.autocast: a reduced-precision
            # autocast dtype opts the many-sequence decode GEMMs into the bf16 MFMA path
            low = _hip.autocast_mode()
            return self.engine().greedy_decode(image_hidden_states, max_length, bf16=low, kv_fp8=self._kv_fp8())
        if num_beams > 1 and single_group:
            if do_sample is True:
                raise NotImplementedError("Beam-search multinomial sampling is not implemented.")
            if num_return_sequences > num_beams:
                raise ValueError("'num_return_sequences' has to be smaller or equal to 'num_beams'.")
            if max_length is None:
                raise ValueError("max_length has to be set for beam generation.")
            # length_penalty = 1.0 as in the reference (language_model.py:461)
            low = _hip.autocast_mode()
            return self.engine().beam_search(image_hidden_states, max_length, num_beams, early_stopping, 1.0, bf16=low,
                                             num_return_sequences=num_return_sequences, kv_fp8=self._kv_fp8())
        raise NotImplementedError("Diverse beam-search decoding is not implemented.")
