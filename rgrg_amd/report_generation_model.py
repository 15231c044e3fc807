"""Host-side mirror of ``src/full_model/report_generation_model.py`` (ttanida/rgrg).

Drop-in for the inference hot path: same constructor, sub-module attribute names,
``load_state_dict(checkpoint["model"])`` keys and ``generate()`` signature / return
tuple / ``-1`` sentinel (report_generation_model.py:12-33, :212-276).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from . import _hip
from ._owner import EngineOwner
from .binary_classifier import BinaryClassifierRegionAbnormal, BinaryClassifierRegionSelection
from .language_model import (LanguageModel, check_beam_sample_args, check_group_beam_args, check_rolling_args, check_rolling_beam_args,
                             check_sample_args)
from .object_detector import ObjectDetector

_LM = "language_model."
_G = _LM + "gpt_with_lm_head.transformer."
_BLOCK_SUB = {"ln_1": "0", "attn": "1", "ln_2": "2", "mlp": "3"}


def expand_alias_keys(sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """The reference state dict holds every GPT-2 tensor under three aliased key families
    (SURVEY.md 8(b)).  Accept a dict that carries only one family (canonical
    ``gpt_with_lm_head.transformer.*``, ``gpt.*`` or ``gpt2_blocks.*`` + ``wte/wpe/...``)
    by filling in the others; also accept the pre-0.13 ``rpn.head.conv.{weight,bias}``
    names (generate_reports_for_images.py:156-159)."""
    out = dict(sd)
    for old, new in (("object_detector.rpn.head.conv.weight", "object_detector.rpn.head.conv.0.0.weight"),
                     ("object_detector.rpn.head.conv.bias", "object_detector.rpn.head.conv.0.0.bias")):
        if old in out and new not in out:
            out[new] = out.pop(old)
    # gpt.* / gpt2_blocks.* / top-level -> canonical
    for k in list(out):
        if k.startswith(_LM + "gpt."):
            out.setdefault(_G + k[len(_LM + "gpt."):], out[k])
        elif k.startswith(_LM + "gpt2_blocks."):
            n, sub, *rest = k[len(_LM + "gpt2_blocks."):].split(".")
            name = {v: kk for kk, v in _BLOCK_SUB.items()}[sub]
            out.setdefault(f"{_G}h.{n}.{name}." + ".".join(rest), out[k])
    for top, canon in ((_LM + "wte.weight", _G + "wte.weight"), (_LM + "wpe.weight", _G + "wpe.weight"),
                       (_LM + "final_layernorm.weight", _G + "ln_f.weight"), (_LM + "final_layernorm.bias", _G + "ln_f.bias"),
                       (_LM + "lm_head.weight", _LM + "gpt_with_lm_head.lm_head.weight")):
        if top in out:
            out.setdefault(canon, out[top])
    if _G + "wte.weight" in out:
        out.setdefault(_LM + "gpt_with_lm_head.lm_head.weight", out[_G + "wte.weight"])
    # canonical -> aliases
    for k in [k for k in out if k.startswith(_G)]:
        rest = k[len(_G):]
        out.setdefault(_LM + "gpt." + rest, out[k])
        parts = rest.split(".")
        if parts[0] == "h":
            out.setdefault(f"{_LM}gpt2_blocks.{parts[1]}.{_BLOCK_SUB[parts[2]]}." + ".".join(parts[3:]), out[k])
        elif parts[0] in ("wte", "wpe"):
            out.setdefault(f"{_LM}{parts[0]}.weight", out[k])
        elif parts[0] == "ln_f":
            out.setdefault(_LM + "final_layernorm." + parts[1], out[k])
    if _LM + "gpt_with_lm_head.lm_head.weight" in out:
        out.setdefault(_LM + "lm_head.weight", out[_LM + "gpt_with_lm_head.lm_head.weight"])
    return out


class ReportGenerationModel(EngineOwner):
    """Object detector encoder -> region-selection classifier -> language-model decoder."""

    def __init__(self, pretrain_without_lm_model: bool = False):
        super().__init__()
        self.pretrain_without_lm_model = pretrain_without_lm_model
        self.object_detector = ObjectDetector(return_feature_vectors=True)
        self.binary_classifier_region_selection = BinaryClassifierRegionSelection()
        self.binary_classifier_region_abnormal = BinaryClassifierRegionAbnormal()
        self.language_model = LanguageModel()
        for child in (self.object_detector, self.binary_classifier_region_selection, self.binary_classifier_region_abnormal,
                      self.language_model):
            self._adopt(child)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Loads a reference ``checkpoint["model"]`` unchanged.  Missing alias families and the
        persistent buffers the kernels do not need (``causal_mask``, ``mask_out_value``,
        ``num_batches_tracked``, ``pos_weight``) are filled from the module; anything else that
        is missing or unexpected is reported (raised when ``strict``), never silently dropped."""
        sd = expand_alias_keys(state_dict)
        own = self.state_dict()
        optional = ("causal_mask", "mask_out_value", "num_batches_tracked", "loss_fn.pos_weight")
        for k, v in own.items():
            if k not in sd and k.endswith(optional):
                sd[k] = v
        return super().load_state_dict(sd, strict=strict, **kw)

    def forward(self, images: torch.FloatTensor, image_targets, input_ids: torch.LongTensor,
                attention_mask: torch.FloatTensor, region_has_sentence: torch.BoolTensor,
                region_is_abnormal: torch.BoolTensor, return_loss: bool = True, past_key_values=None,
                position_ids: Optional[torch.LongTensor] = None, use_cache: Optional[bool] = False):
        """Eval-mode branch of report_generation_model.py:35-168:
        detector -> both region classifiers with their losses -> decoder inputs of the SELECTED regions
        (get_valid_decoder_input_for_evaluation, :196-210) -> teacher-forced language-model loss.  Returns
        ``(obj_detector_loss_dict, classifier_loss_region_selection, classifier_loss_region_abnormal,
        language_model_loss, detections, class_detected, selected_regions, predicted_abnormal_regions)``, the
        7-tuple without the LM loss when ``pretrain_without_lm_model``, or ``-1`` when no region is selected (:136).

        ``image_targets`` (list of {"boxes", "labels"} per image, as evaluate_model.py:413 passes them): the detector
        returns its four validation losses and - as in the reference - runs its RoI heads on the randomly SAMPLED
        training proposals (custom_roi_heads.py:225-226), so the detections / region features of this call depend on the
        sampler's draws.  ``image_targets=None``: ``obj_detector_loss_dict`` is ``{}`` (object_detector.py:195-197).
        In ``train()`` mode see ``_forward_train`` (frozen detector)."""
        if self.training:
            return self._forward_train(images, input_ids, attention_mask, region_has_sentence, region_is_abnormal, return_loss,
                                       past_key_values, position_ids, use_cache)
        obj_detector_loss_dict, detections, top_region_features, class_detected = self.object_detector(images, image_targets)
        del images
        classifier_loss_region_selection, selected_regions, selected_region_features = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=True, region_has_sentence=region_has_sentence)
        classifier_loss_region_abnormal, predicted_abnormal_regions = self.binary_classifier_region_abnormal(
            top_region_features, class_detected, region_is_abnormal)
        if self.pretrain_without_lm_model:
            return (obj_detector_loss_dict, classifier_loss_region_selection, classifier_loss_region_abnormal, detections,
                    class_detected, selected_regions, predicted_abnormal_regions)
        valid_input_ids, valid_attention_mask = self.get_valid_decoder_input_for_evaluation(selected_regions, input_ids,
                                                                                            attention_mask)
        if valid_input_ids.shape[0] == 0:
            return -1
        language_model_loss = self.language_model(valid_input_ids, valid_attention_mask, selected_region_features, return_loss,
                                                  past_key_values, position_ids, use_cache)
        return (obj_detector_loss_dict, classifier_loss_region_selection, classifier_loss_region_abnormal, language_model_loss,
                detections, class_detected, selected_regions, predicted_abnormal_regions)

    def _forward_train(self, images, input_ids, attention_mask, region_has_sentence, region_is_abnormal, return_loss,
                       past_key_values, position_ids, use_cache):
        """Training branch (report_generation_model.py:52-84,136-157) with the object detector FROZEN (BASELINE
        configs[4]; the reference also fine-tunes it): the detector runs its inference branch, ``image_targets`` are
        not used and ``obj_detector_loss_dict`` is ``{}``.  Returns ``(obj_detector_loss_dict,
        classifier_loss_region_selection, classifier_loss_region_abnormal[, language_model_loss])`` - losses with a
        ``grad_fn`` for the classifiers and for uk/uv/feature_space_transformation_nn - or ``-1`` (:136)."""
        low = _hip.autocast_mode()
        with torch.no_grad():
            _detections, top_region_features, class_detected = self.engine().detect(images, bf16=low)
        del images
        classifier_loss_region_selection = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=True, region_has_sentence=region_has_sentence)
        classifier_loss_region_abnormal = self.binary_classifier_region_abnormal(top_region_features, class_detected,
                                                                                 region_is_abnormal)
        if self.pretrain_without_lm_model:
            return {}, classifier_loss_region_selection, classifier_loss_region_abnormal
        valid_input_ids, valid_attention_mask, valid_region_features = self.get_valid_decoder_input_for_training(
            class_detected, region_has_sentence, input_ids, attention_mask, top_region_features)
        if valid_input_ids.shape[0] == 0:
            return -1
        language_model_loss = self.language_model(valid_input_ids, valid_attention_mask, valid_region_features, return_loss,
                                                  past_key_values, position_ids, use_cache)
        return {}, classifier_loss_region_selection, classifier_loss_region_abnormal, language_model_loss

    def get_valid_decoder_input_for_training(self, class_detected, region_has_sentence, input_ids, attention_mask, region_features):
        """report_generation_model.py:170-194: regions that were detected AND have a ground-truth sentence."""
        valid = torch.logical_and(class_detected, region_has_sentence)
        flat = valid.reshape(-1)
        return input_ids[flat], attention_mask[flat], region_features[valid]

    def trainable_parameters(self):
        """What a frozen-detector training run optimises: both region classifiers and the decoder's uk/uv/fst-nn
        (53.66 M values)."""
        return (list(self.binary_classifier_region_selection.classifier.parameters()) +
                list(self.binary_classifier_region_abnormal.classifier.parameters()) +
                self.language_model.trainable_parameters())

    def get_valid_decoder_input_for_evaluation(self, selected_regions, input_ids, attention_mask):
        """report_generation_model.py:196-210: rows of the (batch*29) sentences whose region was selected."""
        selected_regions = selected_regions.reshape(-1)
        return input_ids[selected_regions], attention_mask[selected_regions]

    @torch.no_grad()
    def generate(self, images: torch.FloatTensor, max_length: int = None, num_beams: int = 1, num_beam_groups: int = 1,
                 do_sample: bool = False, num_return_sequences: int = 1, early_stopping: bool = False):
        """images [B,1,512,512] -> (output_ids int64 [S,L'], selected_regions bool [B,29],
        detections {top_region_boxes [B,29,4], top_scores [B,29]}, class_detected bool [B,29]) or ``-1``
        when no region is both detected and selected (report_generation_model.py:260-261)."""
        _, detections, top_region_features, class_detected = self.object_detector(images)
        del images
        selected_regions, selected_region_features = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=False)
        del top_region_features
        if selected_region_features.shape[0] == 0:
            return -1
        output_ids = self.language_model.generate(selected_region_features, max_length, num_beams, num_beam_groups,
                                                  do_sample, num_return_sequences, early_stopping)
        del selected_region_features
        return output_ids, selected_regions, detections, class_detected

    @torch.no_grad()
    def generate_rolling(self, images: torch.FloatTensor, max_length: int, *, rows: Optional[int] = None):
        """``generate`` (greedy) with the sentences of the selected regions decoded by ``LanguageModel.generate_rolling``: the
        regions flow through ``rows`` decoder rows instead of all being decoded in lock step.  The 4-tuple of ``generate``, with the
        same output_ids, or ``-1`` when no region is selected.  Argument errors are ``generate_rolling``'s, raised before the
        detector runs."""
        check_rolling_args(max_length, rows)
        _, detections, top_region_features, class_detected = self.object_detector(images)
        del images
        selected_regions, selected_region_features = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=False)
        del top_region_features
        if selected_region_features.shape[0] == 0:
            return -1
        output_ids = self.language_model.generate_rolling(selected_region_features, max_length, rows=rows)
        del selected_region_features
        return output_ids, selected_regions, detections, class_detected

    def open_rolling(self, max_length: int, *, rows: int, capacity: Optional[int] = None, do_sample: bool = False,
                     temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, num_return_sequences: int = 1,
                     seed: Optional[int] = None, num_beams: int = 1, early_stopping: bool = False, length_penalty: float = 1.0,
                     max_prompt_length: int = 0):
        """``LanguageModel.open_rolling`` behind the detector (same arguments and errors): ``submit(images)`` runs the detector and
        the region selection as ``generate_rolling`` does, enqueues the selected regions' feature rows and returns a ticket;
        ``advance``; ``collect()`` -> ``(ticket, result)`` for every ticket whose sentences have all ended, ``result`` being the
        4-tuple ``generate_rolling(images)`` returns for that submit, or ``-1`` when no region was selected (such a ticket
        completes at once).  With ``num_beams > 1`` the regions are decoded by a ``RollingBeamSession`` and ``result`` is the 4-tuple
        ``generate(images, num_beams=.., early_stopping=.., num_return_sequences=..)`` returns for that submit.
        ``submit(images, max_length=.., temperature=.., top_k=.., top_p=.., seed=.., stop_token_ids=..)`` decodes that submit's
        sentences with parameters of their own and ``cancel(ticket)`` cuts them (``RollingSession``).
        With ``max_prompt_length`` > 0, ``submit(images, region_prompts=..)`` takes int64 [B, 29, P]: the selected regions' sentences
        continue their prompts and the ticket's ids start with them."""
        from .rolling_session import ReportRollingSession
        return ReportRollingSession(self, self.language_model.open_rolling(
            max_length, rows=rows, capacity=capacity, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
            num_return_sequences=num_return_sequences, seed=seed, num_beams=num_beams, early_stopping=early_stopping,
            length_penalty=length_penalty, max_prompt_length=max_prompt_length))

    @torch.no_grad()
    def generate_rolling_beam(self, images: torch.FloatTensor, max_length: int, num_beams: int, *, rows: Optional[int] = None,
                              early_stopping: bool = False, length_penalty: float = 1.0, num_return_sequences: int = 1):
        """``generate(num_beams=..)`` with the sentences of the selected regions decoded by ``LanguageModel.beam_search_rolling``: the
        regions flow through ``rows // num_beams`` slots of beam rows instead of all being decoded in lock step.  The 4-tuple of
        ``generate`` with the same output_ids, or ``-1`` when no region is selected.  Argument errors are
        ``beam_search_rolling``'s, raised before the detector runs."""
        check_rolling_beam_args(max_length, num_beams, rows, num_return_sequences)
        _, detections, top_region_features, class_detected = self.object_detector(images)
        del images
        selected_regions, selected_region_features = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=False)
        del top_region_features
        if selected_region_features.shape[0] == 0:
            return -1
        output_ids = self.language_model.beam_search_rolling(selected_region_features, max_length, num_beams, rows=rows,
                                                             early_stopping=early_stopping, length_penalty=length_penalty,
                                                             num_return_sequences=num_return_sequences)
        del selected_region_features
        return output_ids, selected_regions, detections, class_detected

    @torch.no_grad()
    def sample_rolling(self, images: torch.FloatTensor, max_length: int, *, rows: Optional[int] = None, temperature: float = 1.0,
                       top_k: int = 0, top_p: float = 1.0, num_return_sequences: int = 1, seed: Optional[int] = None,
                       return_logprobs: bool = False):
        """``sample`` with the sentences of the selected regions drawn by ``LanguageModel.sample_rolling``: the same 4-tuple
        (``output_ids`` replaced by the sampler's return: ids, or (ids, logprobs) with ``return_logprobs``) or ``-1`` when no region
        is selected.  Argument errors are ``sample``'s and ``generate_rolling``'s, raised before the detector runs."""
        check_sample_args(temperature, top_k, top_p, num_return_sequences)
        check_rolling_args(max_length, rows)
        _, detections, top_region_features, class_detected = self.object_detector(images)
        del images
        selected_regions, selected_region_features = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=False)
        del top_region_features
        if selected_region_features.shape[0] == 0:
            return -1
        output = self.language_model.sample_rolling(selected_region_features, max_length, rows=rows, temperature=temperature,
                                                    top_k=top_k, top_p=top_p, num_return_sequences=num_return_sequences, seed=seed,
                                                    return_logprobs=return_logprobs)
        del selected_region_features
        return output, selected_regions, detections, class_detected

    @torch.no_grad()
    def generate_diverse(self, images: torch.FloatTensor, max_length: int, num_beams: int, num_beam_groups: int,
                         diversity_penalty: float, early_stopping: bool = False, num_return_sequences: int = 1):
        """``generate`` with the sentences of the selected regions decoded by ``LanguageModel.group_beam_search`` (diverse beam
        search, length penalty 1.0): the 4-tuple of ``generate`` (output_ids [S * num_return_sequences, L]) or ``-1`` when no
        region is selected.  Argument errors are ``group_beam_search``'s, raised before the detector runs."""
        check_group_beam_args(max_length, num_beams, num_beam_groups, diversity_penalty, num_return_sequences)
        _, detections, top_region_features, class_detected = self.object_detector(images)
        del images
        selected_regions, selected_region_features = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=False)
        del top_region_features
        if selected_region_features.shape[0] == 0:
            return -1
        output_ids = self.language_model.group_beam_search(selected_region_features, max_length, num_beams, num_beam_groups,
                                                           diversity_penalty, early_stopping=early_stopping,
                                                           num_return_sequences=num_return_sequences)
        del selected_region_features
        return output_ids, selected_regions, detections, class_detected

    @torch.no_grad()
    def generate_beam_sample(self, images: torch.FloatTensor, max_length: int, num_beams: int, *, temperature: float = 1.0,
                             top_k: int = 0, top_p: float = 1.0, seed: Optional[int] = None, early_stopping: bool = False,
                             num_return_sequences: int = 1):
        """``generate`` with the sentences of the selected regions decoded by ``LanguageModel.beam_sample`` (beam-search sampling,
        length penalty 1.0): the 4-tuple of ``generate`` (output_ids [S * num_return_sequences, L]) or ``-1`` when no region is
        selected.  Argument errors are ``beam_sample``'s, raised before the detector runs."""
        check_beam_sample_args(max_length, num_beams, temperature, top_k, top_p, num_return_sequences)
        _, detections, top_region_features, class_detected = self.object_detector(images)
        del images
        selected_regions, selected_region_features = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=False)
        del top_region_features
        if selected_region_features.shape[0] == 0:
            return -1
        output_ids = self.language_model.beam_sample(selected_region_features, max_length, num_beams, temperature=temperature,
                                                     top_k=top_k, top_p=top_p, seed=seed, early_stopping=early_stopping,
                                                     num_return_sequences=num_return_sequences)
        del selected_region_features
        return output_ids, selected_regions, detections, class_detected

    @torch.no_grad()
    def generate_from_prompts(self, images: torch.FloatTensor, region_prompts: torch.LongTensor, region_prompt_mask: torch.Tensor,
                              max_length: int = None):
        """``generate`` with every region's sentence started from a prefix: region_prompts int64 [B,29,T] and region_prompt_mask
        [B,29,T] (zeros = left padding) hold one prompt per region; the prompts of the SELECTED regions are continued by
        ``LanguageModel.greedy_search``.  Returns the 4-tuple of ``generate`` (output_ids [S,L'] with the prompts in front) or
        ``-1`` when no region is selected."""
        sel = self._selected_prompts(images, region_prompts, region_prompt_mask)
        if sel is None:
            return -1
        prompts, mask, feats, selected_regions, detections, class_detected = sel
        output_ids = self.language_model.greedy_search(prompts, feats, max_length, attention_mask=mask, use_cache=True)
        return output_ids, selected_regions, detections, class_detected

    def _selected_prompts(self, images, region_prompts, region_prompt_mask):
        """Detector and region selection of ``generate`` plus the prompts of the selected regions -> None when nothing is selected,
        else (prompts [S,T], mask [S,T], features [S,1024], selected_regions, detections, class_detected)."""
        B = images.shape[0]
        if region_prompts.dim() != 3 or tuple(region_prompts.shape[:2]) != (B, 29):
            raise ValueError(f"region_prompts must be [B, 29, T] with B = {B}, got {tuple(region_prompts.shape)}")
        if tuple(region_prompt_mask.shape) != tuple(region_prompts.shape):
            raise ValueError(f"region_prompt_mask has shape {tuple(region_prompt_mask.shape)}, region_prompts {tuple(region_prompts.shape)}")
        _, detections, top_region_features, class_detected = self.object_detector(images)
        selected_regions, selected_region_features = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=False)
        if selected_region_features.shape[0] == 0:
            return None
        prompts, mask = self.get_valid_decoder_input_for_evaluation(selected_regions, region_prompts.reshape(B * 29, -1),
                                                                    region_prompt_mask.reshape(B * 29, -1))
        return prompts, mask, selected_region_features, selected_regions, detections, class_detected

    @torch.no_grad()
    def beam_search_from_prompts(self, images: torch.FloatTensor, region_prompts: torch.LongTensor, region_prompt_mask: torch.Tensor,
                                 max_length: int, num_beams: int, early_stopping: bool = False, num_return_sequences: int = 1):
        """``generate_from_prompts`` with beam search: the prompts of the SELECTED regions (one per region, unexpanded) are continued
        by ``LanguageModel.beam_search`` with ``num_beams`` beams and length penalty 1.0, each prompt run once for all its beams.
        Returns the 4-tuple of ``generate`` (output_ids [S * num_return_sequences, L]) or ``-1`` when no region is selected."""
        if int(num_beams) != num_beams or num_beams < 2:
            raise ValueError(f"num_beams has to be an integer > 1 for beam search, but is {num_beams}")
        if not 1 <= num_return_sequences <= num_beams:
            raise ValueError("'num_return_sequences' has to be between 1 and 'num_beams'.")
        if max_length is None:
            raise ValueError("max_length has to be set for beam generation.")
        T = region_prompts.shape[-1]
        if int(max_length) < T + 1:
            raise ValueError(f"max_length has to be at least {T + 1} for prompts of {T} tokens, but is {max_length}")
        sel = self._selected_prompts(images, region_prompts, region_prompt_mask)
        if sel is None:
            return -1
        prompts, mask, feats, selected_regions, detections, class_detected = sel
        output_ids = self.language_model._beam_search_prompts(prompts, mask, feats, int(max_length), int(num_beams), bool(early_stopping),
                                                              1.0, int(num_return_sequences))
        return output_ids, selected_regions, detections, class_detected

    @torch.no_grad()
    def sample_from_prompts(self, images: torch.FloatTensor, region_prompts: torch.LongTensor, region_prompt_mask: torch.Tensor,
                            max_length: int = None, *, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                            num_return_sequences: int = 1, seed: Optional[int] = None, return_logprobs: bool = False):
        """``generate_from_prompts`` with the continuations drawn by ``LanguageModel.sample_from_prompt``: the same 4-tuple
        (``output_ids`` replaced by the sampler's return: ids, or (ids, logprobs) with ``return_logprobs``) or ``-1``."""
        check_sample_args(temperature, top_k, top_p, num_return_sequences)
        sel = self._selected_prompts(images, region_prompts, region_prompt_mask)
        if sel is None:
            return -1
        prompts, mask, feats, selected_regions, detections, class_detected = sel
        output = self.language_model.sample_from_prompt(prompts, feats, max_length, attention_mask=mask, temperature=temperature,
                                                        top_k=top_k, top_p=top_p, num_return_sequences=num_return_sequences, seed=seed,
                                                        return_logprobs=return_logprobs)
        return output, selected_regions, detections, class_detected

    def set_kv_cache_dtype(self, name: Optional[str]) -> None:
        """``LanguageModel.set_kv_cache_dtype``: None, or "fp8_e4m3" for an e4m3 decode K/V cache under torch.autocast with more than
        64 token rows (no effect otherwise)."""
        self.language_model.set_kv_cache_dtype(name)

    @torch.no_grad()
    def sample(self, images: torch.FloatTensor, max_length: int = None, *, temperature: float = 1.0, top_k: int = 0,
               top_p: float = 1.0, num_return_sequences: int = 1, seed: Optional[int] = None, return_logprobs: bool = False):
        """``generate`` with the sentences drawn by ``LanguageModel.sample``: the same 4-tuple (``output_ids`` replaced by the
        sampler's return: ids, or (ids, logprobs) with ``return_logprobs``) and the same ``-1`` when no region is selected."""
        check_sample_args(temperature, top_k, top_p, num_return_sequences)
        _, detections, top_region_features, class_detected = self.object_detector(images)
        del images
        selected_regions, selected_region_features = self.binary_classifier_region_selection(
            top_region_features, class_detected, return_loss=False)
        del top_region_features
        if selected_region_features.shape[0] == 0:
            return -1
        output = self.language_model.sample(selected_region_features, max_length, temperature=temperature, top_k=top_k, top_p=top_p,
                                            num_return_sequences=num_return_sequences, seed=seed, return_logprobs=return_logprobs)
        del selected_region_features
        return output, selected_regions, detections, class_detected
