"""Rolling sessions (per-submit parameters and cancel: 7.18): rolling-batch greedy decoding and sampling over an open
list.  ``RollingSession`` is what ``HipEngine.open_rolling`` / ``LanguageModel.open_rolling`` return - feature rows in, numbered sequences out -,
``ReportRollingSession`` what ``ReportGenerationModel.open_rolling`` returns - images in, one ``generate_rolling`` result per
submit out.  Every FLOP runs in ``librgrg_hip.so`` (rgrg_decoder_roll_*)."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Union

import torch

from . import _hip
from .constants import PAD_TOKEN_ID


def check_max_prompt_length(max_prompt_length, max_length: int, beam: bool = False) -> int:
    """``open_rolling(max_prompt_length=..)`` -> the int, or ValueError: 0 (no prompts) .. max_length - 1, and 0 in a beam session."""
    mp = max_prompt_length
    if isinstance(mp, bool) or int(mp) != mp or mp < 0:
        raise ValueError(f"max_prompt_length has to be a non-negative integer, but is {mp}")
    if mp and beam:
        raise ValueError("max_prompt_length: a rolling beam session takes no prompts (its scheduler lives on the host); open it with "
                         "max_prompt_length=0")
    if mp >= max_length:
        raise ValueError(f"max_prompt_length has to be below max_length {max_length} (which counts the prompt, and one token is always "
                         f"generated), but is {mp}")
    return int(mp)


class RollingSession:
    """R decoder rows through which the sequences of any number of ``submit`` calls flow.  Sequences are numbered q = 0, 1, ... in
    submit order, n per feature row.  The session holds ``capacity`` feature rows at a time: a submit that does not fit until
    finished sequences have been collected raises ``RgrgHipError`` and leaves the session as it was.  Any other decode call on the
    engine makes the session stale: its next call raises ``RgrgHipError`` ("stale"), ``close`` still works."""

    def __init__(self, engine, dec, rows: int, capacity: int, n: int, max_length: int, sample: bool, max_prompt_length: int = 0):
        self._eng, self._dec = engine, dec
        self.rows, self.capacity, self.n, self.max_length, self.sampled = rows, capacity, n, max_length, sample
        self.max_prompt_length = max_prompt_length   # 0: the session takes no prompts
        self.submitted = 0          # sequences numbered so far
        self.watermark = 0          # the lowest sequence number not yet released
        self.unfinished = 0         # sequences pending or in a row, as of the last advance plus what was submitted since
        self.steps = 0              # the device's count of steps that had a sequence in a row
        self._collected = set()     # delivered sequences at or above the watermark
        self.cancelled = set()      # sequences that ``cancel`` has cut, as their delivery by ``collect`` told
        self._known_stale = False
        self._hold = []

    _abi = "rgrg_decoder_roll_"   # the C entries behind submit / advance / close (RollingBeamSession: rgrg_decoder_beam_roll_)

    # ------------------------------------------------------------------ helpers
    def _fn(self, name: str):
        return getattr(self._eng.lib, self._abi + name)

    def _check(self, rc: int, name: str) -> None:
        try:
            _hip.check(rc, name)
        except _hip.RgrgHipError as e:
            if "stale" in str(e):
                self._known_stale = True
            raise

    def _live(self):
        if self._dec is None:
            raise _hip.RgrgHipError("the rolling session is closed")
        if self._eng._decoder is not self._dec:   # the engine has replaced its decoder (a larger call): the rows are gone
            self._known_stale = True
            raise _hip.RgrgHipError("the rolling session is stale: the engine's decoder has been replaced since it was opened")
        return self._eng.lib, self._dec

    @property
    def closed(self) -> bool:
        return self._dec is None

    # ------------------------------------------------------------------ the calls
    def _request(self, max_length=None, temperature=None, top_k=None, top_p=None, seed=None, stop_token_ids=None):
        """The keywords of ``submit`` -> the arguments of rgrg_decoder_roll_submit_req behind m, or None when no keyword is given
        (ValueError before anything is enqueued)."""
        from .language_model import check_sample_args
        sampling = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
        given = [k for k, v in sampling.items() if v is not None]
        if max_length is None and not given and stop_token_ids is None:
            return None
        if max_length is not None and (int(max_length) != max_length or not 2 <= max_length <= self.max_length):
            raise ValueError(f"max_length of a submit has to be in 2 .. {self.max_length} (the session's), but is {max_length}")
        if given and not self.sampled:
            raise ValueError(f"{', '.join(given)}: sampling parameters of a submit need a sampling session, this is a greedy session")
        check_sample_args(1.0 if temperature is None else temperature, 0 if top_k is None else top_k, 1.0 if top_p is None else top_p, 1)
        if seed is not None and int(seed) != seed:
            raise ValueError(f"seed has to be an integer, but is {seed}")
        stops = [] if stop_token_ids is None else list(stop_token_ids)
        if len(stops) > 4:
            raise ValueError(f"stop_token_ids holds {len(stops)} token ids, up to 4 are possible")
        for t in stops:
            if int(t) != t or not 0 <= t < 65535:
                raise ValueError(f"stop_token_ids has to hold token ids in 0 .. 65534, but holds {t}")
        return (0 if max_length is None else int(max_length), 0.0 if temperature is None else float(temperature),
                -1 if top_k is None else int(top_k), 0.0 if top_p is None else float(top_p), 0 if seed is None else 1,
                0 if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF, (C.c_int * max(len(stops), 1))(*[int(t) for t in stops]), len(stops))

    def _prompt(self, prompt_ids, m: int, max_length: Optional[int]) -> Optional[torch.Tensor]:
        """``submit(prompt_ids=..)`` -> int64 [m, P] on the host, contiguous (None without a prompt); ValueError before anything is
        enqueued.  (A device tensor is copied to the host here, which waits for its stream: callers that must not wait pass host ids.)"""
        if prompt_ids is None:
            return None
        if not self.max_prompt_length:
            raise ValueError("prompt_ids: the session was opened without max_prompt_length (open_rolling(.., max_prompt_length=P_max) "
                             "allocates the prompt rings)")
        if not isinstance(prompt_ids, torch.Tensor) or prompt_ids.dtype != torch.int64:
            raise ValueError(f"prompt_ids has to be an int64 tensor [m, P] or [P], but is "
                             f"{prompt_ids.dtype if isinstance(prompt_ids, torch.Tensor) else type(prompt_ids).__name__}")
        if prompt_ids.dim() == 1:
            prompt_ids = prompt_ids.unsqueeze(0).expand(m, -1)
        if prompt_ids.dim() != 2 or prompt_ids.shape[0] != m:
            raise ValueError(f"prompt_ids has to be [m = {m}, P] (one prompt length per submit) or [P], but is {tuple(prompt_ids.shape)}")
        P, limit = prompt_ids.shape[1], self.max_length if max_length is None else max_length
        if not 1 <= P <= self.max_prompt_length or P + 1 > limit:
            raise ValueError(f"prompt_ids holds {P} tokens per prompt: 1 .. {min(self.max_prompt_length, limit - 1)} are possible "
                             f"(max_prompt_length {self.max_prompt_length}; max_length {limit} counts the prompt and one token is always "
                             f"generated)")
        ids = prompt_ids.detach().to("cpu").contiguous()
        vocab = self._eng.vocab
        if int(ids.min()) < 0 or int(ids.max()) >= vocab:
            raise ValueError(f"prompt_ids has to hold token ids in 0 .. {vocab - 1}, but holds {int(ids.min())} .. {int(ids.max())}")
        return ids

    def submit(self, feats: torch.Tensor, *, prompt_ids: Optional[torch.Tensor] = None, max_length: Optional[int] = None,
               temperature: Optional[float] = None, top_k: Optional[int] = None, top_p: Optional[float] = None,
               seed: Optional[int] = None, stop_token_ids: Optional[Iterable[int]] = None) -> range:
        """feats [m, 1024] on the engine's device -> the sequence numbers of its m * n sentences.  Enqueued behind the steps already
        launched; an idle row starts a new sentence in the very next step.  Does not wait for the device.
        The keywords hold for all m * n sentences of this submit, None being the session's value: ``max_length`` in
        2 .. the session's; ``temperature`` / ``top_k`` / ``top_p`` / ``seed`` in a sampling session only, validated as ``sample``
        does (``top_k=1``: a greedy sentence); with ``seed`` the sentences draw what ``sample_rolling(feats, .., seed=seed)`` draws for
        these rows alone; ``stop_token_ids``: up to 4 token ids that end a sentence as EOS does, the stop token being its last.
        ``prompt_ids`` (a session opened with ``max_prompt_length``): int64 [m, P], or [P] for all m rows - the
        sentences continue it as ``greedy_search`` continues ``input_ids`` under a mask of ones.  One P per submit, 1 ..
        ``max_prompt_length``, and P + 1 <= the submit's ``max_length``, which counts the prompt; no padding and no mask.  Any ids
        of the vocabulary: an EOS or a stop token inside the prompt ends nothing.  The n hypotheses of a row share its prompt;
        ``collect`` delivers the prompt in front, its log-probs 0.  A BOS column is the submit without a prompt.  Pass a HOST
        tensor: the ids are checked and handed over on the host, so a tensor on the device is copied back first, and that copy
        waits for the device - the one case in which ``submit`` does.
        ValueError, the session as it was, for a value out of range."""
        lib, dec = self._live()
        if feats.dim() != 2 or feats.shape[0] < 1 or feats.shape[1] != 1024:
            raise ValueError(f"submit takes feature rows [m >= 1, 1024], got {tuple(feats.shape)}")
        req = self._request(max_length=max_length, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, stop_token_ids=stop_token_ids)
        prompt = self._prompt(prompt_ids, feats.shape[0], max_length)
        with torch.cuda.device(self._eng.device):
            f = feats.to(device=self._eng.device, dtype=torch.float32).contiguous()
            first = C.c_longlong(0)
            if prompt is not None:
                if req is None:
                    req = (0, 0.0, -1, 0.0, 0, 0, (C.c_int * 1)(), 0)   # the session's values
                self._check(lib.rgrg_decoder_roll_submit_prompt(dec, _hip.ptr(f), f.shape[0], prompt.data_ptr(), prompt.shape[1], *req,
                                                                C.byref(first), self._eng._s()), "rgrg_decoder_roll_submit_prompt")
            elif req is None:
                self._check(self._fn("submit")(dec, _hip.ptr(f), f.shape[0], C.byref(first), self._eng._s()), self._abi + "submit")
            else:
                self._check(lib.rgrg_decoder_roll_submit_req(dec, _hip.ptr(f), f.shape[0], *req, C.byref(first), self._eng._s()),
                            "rgrg_decoder_roll_submit_req")
            self._hold.append(f)   # the GEMMs read it on the decoder's stream: kept until an advance has synchronised
        count = f.shape[0] * self.n
        self.submitted = first.value + count
        self.unfinished += count
        return range(first.value, first.value + count)

    def cancel(self, qs: Union[int, Iterable[int]]) -> None:
        """Cancels sequences - a number or an iterable of numbers at or above the watermark and below ``submitted`` (ValueError
        otherwise, nothing cancelled).  Enqueued on the decoder's stream: the next step launched cuts a sequence that is running
        (that step's token is not appended, its row takes the next pending sequence in the same step); a pending one is cut in the
        first step of the row it takes, as BOS - or its prompt - alone; one that has ended is left as it is.  ``collect`` delivers a cut sequence with
        the tokens it had, and ``cancelled`` then holds its number."""
        lib, dec = self._live()
        qs = [qs] if isinstance(qs, int) else list(qs)
        for q in qs:
            if int(q) != q or not self.watermark <= q < self.submitted:
                raise ValueError(f"cancel: sequence {q}, {self.watermark} .. {self.submitted - 1} can be cancelled (collected and "
                                 f"released ones, and ones not submitted yet, cannot)")
        qs = sorted(set(int(q) for q in qs))
        with torch.cuda.device(self._eng.device):
            i = 0
            while i < len(qs):   # whole runs of consecutive numbers
                j = i
                while j + 1 < len(qs) and qs[j + 1] == qs[j] + 1:
                    j += 1
                self._check(lib.rgrg_decoder_roll_cancel(dec, qs[i], j - i + 1), "rgrg_decoder_roll_cancel")
                i = j + 1

    def advance(self, steps: Optional[int] = None) -> int:
        """Runs up to ``steps`` decode steps (None: until nothing is unfinished) and waits for them -> the steps launched; 0 at once
        when nothing is unfinished."""
        lib, dec = self._live()
        if steps is not None and (int(steps) != steps or steps < 0):
            raise ValueError(f"steps has to be None or a non-negative integer, but is {steps}")
        launched, unfinished, dsteps = C.c_int(0), C.c_int(0), C.c_int(0)
        with torch.cuda.device(self._eng.device):
            self._check(self._fn("advance")(dec, -1 if steps is None else int(steps), C.byref(launched), C.byref(unfinished),
                                            C.byref(dsteps)), self._abi + "advance")
        self.unfinished, self.steps = unfinished.value, dsteps.value
        self._hold = []
        return launched.value

    def collect(self) -> List[tuple]:
        """Every finished sequence not delivered yet, in ascending q: ``(q, ids)`` - int64 [len], BOS first, the EOS included - and for
        a sampling session ``(q, ids, logprobs)``.  Sequences finish out of order and are delivered so; the ring is released over
        the delivered PREFIX only, so one long sentence in front keeps the room of those behind it.  A sequence that ``cancel`` has
        cut is delivered likewise, with the tokens it had and no EOS added, and joins ``cancelled``."""
        lib, dec = self._live()
        first, count = self.watermark, self.submitted - self.watermark
        if count == 0:
            return []
        lens = (C.c_int * count)()
        with torch.cuda.device(self._eng.device):
            self._check(lib.rgrg_decoder_roll_collect(dec, first, count, None, None, lens, self._eng._s()), "rgrg_decoder_roll_collect")
            new = [i for i in range(count) if lens[i] != 0 and first + i not in self._collected]   # (< 0: cut by cancel)
            if not new:
                return []
            lo, span = new[0], new[-1] - new[0] + 1
            ids = torch.empty((span, self.max_length), dtype=torch.int64, device=self._eng.device)
            lp = torch.empty((span, self.max_length), dtype=torch.float32, device=self._eng.device) if self.sampled else None
            lens2 = (C.c_int * span)()
            self._check(lib.rgrg_decoder_roll_collect(dec, first + lo, span, _hip.ptr(ids), _hip.ptr(lp), lens2, self._eng._s()),
                        "rgrg_decoder_roll_collect")
            out = []
            for i in new:
                row = (first + i, ids[i - lo, :abs(lens[i])])   # (views of this call's own copy of the ring rows)
                out.append(row + (lp[i - lo, :abs(lens[i])],) if self.sampled else row)
                self._collected.add(first + i)
                if lens[i] < 0:
                    self.cancelled.add(first + i)
            wm = self.watermark
            while wm in self._collected:
                self._collected.discard(wm)
                wm += 1
            if wm != self.watermark:
                self._check(lib.rgrg_decoder_roll_release(dec, wm), "rgrg_decoder_roll_release")
                self.watermark = wm
        return out

    def close(self) -> None:
        """Ends the session (also a stale one); the engine can open another."""
        if self._dec is None:
            return
        dec, self._dec = self._dec, None
        if self._eng._session is self:
            self._eng._session = None
        if self._eng._decoder is dec:   # otherwise the decoder went away, and the session's rings with it
            with torch.cuda.device(self._eng.device):
                _hip.check(self._fn("close")(dec), self._abi + "close")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class RollingBeamSession(RollingSession):
    """Rolling beam search over an open list (rgrg_decoder_beam_roll_*): ``rows // num_beams`` slots of ``num_beams``
    decoder rows through which the regions of any number of ``submit`` calls flow.  The surface of ``RollingSession`` with regions
    in place of sentences: one region per feature row, numbered q = 0, 1, ... in submit order; ``capacity`` counts regions."""

    _abi = "rgrg_decoder_beam_roll_"

    def __init__(self, engine, dec, rows: int, capacity: int, max_length: int, num_beams: int, num_return_sequences: int):
        super().__init__(engine, dec, rows, capacity, 1, max_length, False)
        self.num_beams, self.num_return_sequences, self.slots = num_beams, num_return_sequences, rows // num_beams

    def _request(self, **params):
        if any(v is not None for v in params.values()):
            raise ValueError(f"{', '.join(k for k, v in params.items() if v is not None)}: a rolling beam session takes no parameters "
                             f"per submit (its scheduler lives on the host)")
        return None

    def submit(self, feats: torch.Tensor, *, prompt_ids=None, **params) -> range:
        if prompt_ids is not None:
            raise ValueError("prompt_ids: a rolling beam session takes no prompts (its scheduler lives on the host)")
        self._request(**params)
        return super().submit(feats)

    def cancel(self, qs) -> None:
        raise ValueError("cancel: a rolling beam session cannot cancel a region (its scheduler lives on the host)")

    def collect(self) -> List[tuple]:
        """Every finished region not delivered yet, in ascending q: ``(q, ids)`` with ids int64 [num_return_sequences, L_q] - the rows
        ``generate(num_beams=..)`` returns for the region, at the padded width L_q of that region alone.  Regions finish out of
        order and are delivered so; the delivered PREFIX is released."""
        lib, dec = self._live()
        first, count = self.watermark, self.submitted - self.watermark
        if count == 0:
            return []
        fin = (C.c_int * count)()
        out = []
        with torch.cuda.device(self._eng.device):
            self._check(lib.rgrg_decoder_beam_roll_collect(dec, first, count, None, 0, None, fin, self._eng._s()), "rgrg_decoder_beam_roll_collect")
            for i in range(count):
                q = first + i
                if not fin[i] or q in self._collected:
                    continue
                ids = torch.empty((self.num_return_sequences, self.max_length), dtype=torch.int64, device=self._eng.device)
                width = C.c_int(0)
                self._check(lib.rgrg_decoder_beam_roll_collect(dec, q, 1, _hip.ptr(ids), self.max_length, C.byref(width), None, self._eng._s()),
                            "rgrg_decoder_beam_roll_collect")
                out.append((q, ids[:, :width.value].contiguous()))
                self._collected.add(q)
            wm = self.watermark
            while wm in self._collected:
                self._collected.discard(wm)
                wm += 1
            if wm != self.watermark:
                self._check(lib.rgrg_decoder_beam_roll_release(dec, wm), "rgrg_decoder_beam_roll_release")
                self.watermark = wm
        return out


class ReportRollingSession:
    """``ReportGenerationModel.open_rolling``: every ``submit(images)`` is a ticket; ``collect`` returns ``(ticket, result)`` for the
    tickets whose sentences have all ended, ``result`` being what ``generate_rolling(images)`` returns for that submit (``-1`` when
    no region was selected - such a ticket completes at once).  Over a ``RollingBeamSession`` a region delivers its
    num_return_sequences hypotheses and ``result`` is what ``generate(images, num_beams=..)`` returns."""

    def __init__(self, model, session: RollingSession):
        self._model, self.session = model, session
        self._tickets = {}      # ticket -> [range of sequences, rest of the 4-tuple, {q: ids}]
        self._done = []         # (ticket, -1) of submits without a selected region
        self._cancelled = set()
        self._next = 0

    @torch.no_grad()
    def submit(self, images: torch.Tensor, *, region_prompts: Optional[torch.Tensor] = None, **params) -> int:
        """``params``: the keywords of ``RollingSession.submit`` for the sentences of these images.  ``region_prompts``: int64
        [B, 29, P], a prompt for every region of every image (``generate_from_prompts``' layout, without a mask); the prompts of the
        selected regions go with their feature rows and the ticket's ids start with them.  An argument error leaves the session as
        it was and takes no ticket."""
        m = self._model
        if self.session.closed:
            raise _hip.RgrgHipError("the rolling session is closed")
        if region_prompts is not None and (not isinstance(region_prompts, torch.Tensor) or region_prompts.dim() != 3
                                           or region_prompts.shape[:2] != (images.shape[0], 29)):
            raise ValueError(f"region_prompts has to be an int64 tensor [B = {images.shape[0]}, 29, P], but is "
                             f"{tuple(region_prompts.shape) if isinstance(region_prompts, torch.Tensor) else type(region_prompts).__name__}")
        _, detections, top_region_features, class_detected = m.object_detector(images)
        selected_regions, feats = m.binary_classifier_region_selection(top_region_features, class_detected, return_loss=False)
        if region_prompts is not None:
            flat = region_prompts.reshape(-1, region_prompts.shape[2])
            # the argument errors are those of a submit that has sentences, whatever was selected
            params["prompt_ids"] = flat[selected_regions.reshape(-1).to(flat.device)] if feats.shape[0] else flat[:1]
        if feats.shape[0] == 0:
            self.session._request(**{k: v for k, v in params.items() if k != "prompt_ids"})   # (the argument errors of a submit that has sentences)
            if region_prompts is not None:
                self.session._prompt(params["prompt_ids"], 1, params.get("max_length"))
            rng = None
        else:
            rng = self.session.submit(feats, **params)
        ticket, self._next = self._next, self._next + 1
        if rng is None:
            self._done.append((ticket, -1))
        else:
            self._tickets[ticket] = [rng, (selected_regions, detections, class_detected), {}]
        return ticket

    def cancel(self, ticket: int) -> None:
        """Cancels the sentences of a ticket that have not ended (``RollingSession.cancel``); the ticket completes with the cut
        sentences and is in ``cancelled`` then if at least one was cut.  A ticket that has been delivered: ValueError."""
        if ticket not in self._tickets:
            if any(t == ticket for t, _ in self._done):
                return   # (no region was selected: nothing runs)
            raise ValueError(f"cancel: ticket {ticket} is not open (never given, or delivered already)")
        rng, _, got = self._tickets[ticket]
        qs = [q for q in rng if q not in got]
        if qs:
            self.session.cancel(qs)

    @property
    def cancelled(self) -> set:
        """Tickets of which ``cancel`` has cut at least one sentence, as their sentences' delivery told."""
        return self._cancelled

    def advance(self, steps: Optional[int] = None) -> int:
        return self.session.advance(steps)

    @property
    def unfinished(self) -> int:
        return self.session.unfinished

    def collect(self) -> List[tuple]:
        out, self._done = self._done, []
        if self._tickets:
            for item in self.session.collect():
                for rng, _, got in self._tickets.values():
                    if item[0] in rng:
                        got[item[0]] = item[1]
                        break
            for ticket, (rng, _, _) in self._tickets.items():
                if any(q in self.session.cancelled for q in rng):
                    self._cancelled.add(ticket)
        for ticket in sorted(self._tickets):
            rng, rest, got = self._tickets[ticket]
            if len(got) == len(rng):
                # a sentence [len] or a region's hypotheses [n, L_q], PAD up to the widest of the ticket: the width generate() computes
                rows = [got[q].reshape(-1, got[q].shape[-1]) for q in rng]
                width = max(r.shape[1] for r in rows)
                ids = torch.full((sum(r.shape[0] for r in rows), width), PAD_TOKEN_ID, dtype=torch.int64, device=rows[0].device)
                at = 0
                for r in rows:
                    ids[at:at + r.shape[0], :r.shape[1]] = r
                    at += r.shape[0]
                out.append((ticket, (ids,) + rest))
                del self._tickets[ticket]
        return sorted(out, key=lambda t: t[0])

    def close(self) -> None:
        self.session.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
