"""Numpy model of prompts in a rolling session (rgrg_amd/csrc/decoder_roll.hip), and the greedy oracle loop the GPU
tests hold prompted sessions to.  No GPU.

A session opened with max_prompt_length = MP keeps, per FEATURE row f = (q / n) % Cf of the ring (Cf = C / n feature rows, C sequences):
  ptok [Cf][MP]   the prompt's tokens           plen [Cf]   its length P, 1 .. MP (1, BOS: a submit without a prompt)
  pkv  [layers][2][Cf][H][MP][64]               the keys / values of prompt rows 0 .. P - 2 in slots 1 .. P - 1 (slot 0 is not used)
Device side, on plain arrays (what rgrg_debug_roll_prompt_step runs; ``prompt_step`` is its model):
  submit_init     the id row of a new sequence q (ring row q % C) holds its feature row's P prompt tokens, then PAD; log-probs 0, length 0
  pass_           the retire pass of rolling_request_reference with ONE change, the seating: a row that takes sequence q gets
                  len = P, tok = prompt[P - 1], pos = step = P - 1.  Everything else follows from len starting at P: the limit
                  (the request's max_length, or the session's) counts the prompt, stop tokens and EOS are looked at in GENERATED
                  tokens only, and a sequence cut before its first step has the length word -P.
  prompt_refill   for every (row, sequence) seated: ring slots 1 .. P - 1 -> cache slots 1 .. P - 1 of the row, every layer, plane, head.
``play`` drives whole sequences through R rows with a token function and returns what ``collect`` would deliver.

MUTATIONS are wrong rules an implementation could have; tests/test_rolling_prompt_reference.py shows that the cases the GPU tests run
reject each of them.

``oracle_greedy`` is greedy_search of the restated reference (oracle.language_model.lm_forward) for prompts without padding, grouped by
prompt length, with the smallest top-2 logit gap over the generated positions of unfinished rows."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import rolling_request_reference as Q

BOS = EOS = PAD = Q.BOS
NEXT, UNFINISHED, REFILLS, STEPS = Q.NEXT, Q.UNFINISHED, Q.REFILLS, Q.STEPS
NO_STOP, CANCEL = Q.NO_STOP, Q.CANCEL
MUTATIONS = ("seat_step_P", "position_zero", "ring_row_q", "no_wrap", "copy_P_slots", "limit_generated_only", "stop_in_prompt",
             "cancel_bos_alone")


def new_state(R: int) -> Dict[str, np.ndarray]:
    """Every row idle, nothing pending (roll_begin_kernel with S = 0)."""
    st = {k: np.zeros(R, dtype=np.int32) for k in ("seq", "len", "tok", "pos", "step")}
    st["seq"][:], st["tok"][:] = -1, BOS
    st["shared"] = np.zeros(4, dtype=np.int32)
    return st


def feature_row(q: int, n: int, Cf: int, mut: Optional[str] = None) -> int:
    """The ring row of sequence q's prompt (and of its image key / value)."""
    f = q if mut == "ring_row_q" else q // n
    return min(f, Cf - 1) if mut == "no_wrap" else f % Cf      # (no wrap: a real kernel would read past the ring; the model stays inside)


def submit_init(st, ids, lens, lp, C: int, n: int, S_before: int, count: int, max_length: int, ptok, plen, mut=None) -> int:
    """The ring rows of sequences S_before .. S_before + count - 1 IN PLACE -> the new S."""
    Cf = C // n
    for q in range(S_before, S_before + count):
        f = feature_row(q, n, Cf, mut)
        P = int(plen[f])
        ids[q % C, :max_length] = PAD
        ids[q % C, :P] = ptok[f, :P]
        lens[q % C] = 0
        if lp is not None:
            lp[q % C, :max_length] = 0.0
    st["shared"][UNFINISHED] += count
    return S_before + count


def pass_(st, arg, ids, lens, C: int, n: int, S_: int, max_length: int, ptok, plen, req=None, handout_only: bool = False,
          mut: Optional[str] = None) -> List[Tuple[int, int, int, int]]:
    """One retire pass (handout_only: rows that hold a sequence are not touched, no step is counted) IN PLACE -> the seatings
    [(row, sequence, ring row, P)] in ascending row order."""
    assert mut is None or mut in MUTATIONS, mut
    R, Cf = st["seq"].shape[0], C // n
    nxt = int(st["shared"][NEXT])
    free, any_active = [], False
    for r in range(R):
        seq = int(st["seq"][r])
        if seq < 0:
            free.append(r)
            continue
        if handout_only:
            continue
        any_active = True
        slot = seq % C
        tok, ln = int(arg[r]), int(st["len"][r])
        P = int(plen[feature_row(seq, n, Cf)])
        limit, stops, cut = max_length, [], False
        if req is not None:
            e = req[slot]
            limit = min(int(e["max_length"]), max_length)
            stops = [int(t) for t in e["stop"] if int(t) != NO_STOP]
            cut = bool(int(e["flags"]) & CANCEL)
        if cut:
            lens[slot] = -1 if (mut == "cancel_bos_alone" and ln == P) else -ln
            free.append(r)
            continue
        ids[slot, ln] = tok
        ln += 1
        hit = tok == EOS or tok in stops
        if mut == "stop_in_prompt":      # (a rule that scans the whole row: a stop token or EOS in the prompt ends the sequence)
            hit = hit or any(int(t) == EOS or int(t) in stops for t in ptok[feature_row(seq, n, Cf), 1:P])
        done = (ln - P + 1 >= limit) if mut == "limit_generated_only" else ln >= limit
        if hit or done:
            lens[slot] = ln
            free.append(r)
        else:
            st["len"][r], st["tok"][r], st["pos"][r], st["step"][r] = ln, tok, ln - 1, ln - 1
    given = min(len(free), S_ - nxt)
    seated = []
    for k, r in enumerate(free):
        if k >= given:
            st["seq"][r], st["len"][r], st["tok"][r], st["pos"][r], st["step"][r] = -1, 0, BOS, 0, 0
            continue
        seq = nxt + k
        f = feature_row(seq, n, Cf, mut)
        P = int(plen[f])
        st["seq"][r], st["len"][r], st["tok"][r] = seq, P, int(ptok[f, P - 1])
        st["pos"][r] = 0 if mut == "position_zero" else P - 1
        st["step"][r] = P if mut == "seat_step_P" else P - 1
        seated.append((r, seq, f, P))
    nxt += given
    st["shared"][NEXT] = nxt
    st["shared"][REFILLS] = given
    st["shared"][UNFINISHED] = (S_ - nxt) + int((st["seq"] >= 0).sum())
    st["shared"][STEPS] += 1 if any_active else 0
    return seated


def prompt_refill(cache: np.ndarray, ring: np.ndarray, seated, mut: Optional[str] = None) -> None:
    """cache [layers][2][R][H][T][64], ring [layers][2][Cf][H][MP][64] (any dtype: these are bytes) IN PLACE."""
    for r, _, f, P in seated:
        hi = min(P + 1 if mut == "copy_P_slots" else P, ring.shape[4])
        cache[:, :, r, :, 1:hi] = ring[:, :, f, :, 1:hi]


def prompt_step(st, arg, ids, lens, lp, C, n, S_before, submit, handout, retire, max_length, ptok, plen, req=None, mut=None):
    """rgrg_debug_roll_prompt_step IN PLACE -> the seatings of the hand-out pass and of the retire pass."""
    S_ = submit_init(st, ids, lens, lp, C, n, S_before, submit, max_length, ptok, plen, mut) if submit else S_before
    a = pass_(st, arg, ids, lens, C, n, S_, max_length, ptok, plen, req, True, mut) if handout else []
    b = pass_(st, arg, ids, lens, C, n, S_, max_length, ptok, plen, req, False, mut) if retire else []
    return a, b


# ------------------------------------------------------------------------------------------------ whole sequences
def model_token(q: int, pos: int, step: int, tok_in: int, keys_ok: bool) -> int:
    """The stand-in for the decoder: the next token of sequence q as a function of EVERYTHING the step is fed - the input token, its
    embedding position, the key count (step + 2) and whether the cache slots 1 .. step hold the sequence's own keys - so that a wrong
    seating shows in the tokens.  Never EOS, never below 1000."""
    return 1000 + (31 * q + 7 * pos + 13 * step + 3 * (tok_in % 97) + (0 if keys_ok else 5000)) % 40000


def play(subs: Sequence[dict], R: int, Cf: int, n: int, L: int, MP: int, mut: Optional[str] = None, natural: Optional[Dict[int, int]] = None,
         cancel: Sequence[int] = ()):
    """Submits ``subs`` - dicts(m, prompt [m][P] or None, max_length, stop) - one after the other, each as soon as the ring has room,
    and steps until everything has ended -> {q: (ids list, length word)}.  ``natural[q]``: the length at which sequence q emits EOS.
    ``cancel``: sequences flagged right after their submit.  The cache is modelled by a tag per (row, slot): which sequence's
    prompt / history the slot holds."""
    C = Cf * n
    st = new_state(R)
    ids, lens = np.full((C, L + MP), -7, dtype=np.int64), np.zeros(C, dtype=np.int32)      # (wider than L: a mutated limit overruns it)
    ptok, plen = np.full((Cf, MP), BOS, dtype=np.int64), np.ones(Cf, dtype=np.int32)
    ring_tag = np.full((1, 1, Cf, 1, MP, 1), -1, dtype=np.int64)          # slot j of ring row f holds the keys of (sequence group, j)
    cache_tag = np.full((1, 1, R, 1, L + MP + 2, 1), -2, dtype=np.int64)
    req = Q.new_ring(C, L)
    out, S_, watermark, pending = {}, 0, 0, list(subs)
    natural = natural or {}

    def deliver():
        nonlocal watermark
        while watermark < S_ and lens[watermark % C] != 0:
            ln = int(lens[watermark % C])
            out[watermark] = (ids[watermark % C, :abs(ln)].tolist(), ln)
            watermark += 1

    def seat(seated):
        prompt_refill(cache_tag, ring_tag, seated, mut)
        for r, q, _, _ in seated:
            cache_tag[0, 0, r, 0, 0, 0] = (q // n) * 1000       # the image slot (roll_refill_kernel, unchanged)

    for _ in range(100000):
        while pending and S_ + pending[0]["m"] * n <= watermark + C:
            sub = pending.pop(0)
            m, prompt = sub["m"], sub.get("prompt")
            for i in range(m):
                f = (S_ // n + i) % Cf
                row = [BOS] if prompt is None else list(prompt[i])
                plen[f], ptok[f, :len(row)] = len(row), row
                ring_tag[0, 0, f, 0, :, 0] = -1
                ring_tag[0, 0, f, 0, 1:len(row), 0] = [(S_ // n + i) * 1000 + j for j in range(1, len(row))]
            for q in range(S_, S_ + m * n):
                Q.set_request(req, q, max_length=sub.get("max_length") or L, stop=sub.get("stop", ()), cancel=q in cancel)
            S_ = submit_init(st, ids, lens, None, C, n, S_, m * n, L, ptok, plen, mut)
            seat(pass_(st, None, ids, lens, C, n, S_, L, ptok, plen, req, True, mut))
        if not pending and int(st["shared"][UNFINISHED]) == 0:
            break
        arg = np.zeros(R, dtype=np.int32)
        for r in range(R):
            q, ln, step = int(st["seq"][r]), int(st["len"][r]), int(st["step"][r])
            if q < 0:
                continue
            cache_tag[0, 0, r, 0, step + 1, 0] = (q // n) * 1000 + step + 1      # the step writes its own key into slot step + 1
            want = [(q // n) * 1000 + j for j in range(0, step + 2)]
            keys_ok = cache_tag[0, 0, r, 0, :step + 2, 0].tolist() == want
            # (histories of the n hypotheses of a feature row differ behind the prompt; the tag only follows the prompt and the slot count)
            arg[r] = EOS if ln + 1 == natural.get(q, -1) else model_token(q, int(st["pos"][r]), step, int(st["tok"][r]), keys_ok)
        seat(pass_(st, arg, ids, lens, C, n, S_, L, ptok, plen, req, False, mut))
        deliver()
    else:
        raise AssertionError("the model session never drained")
    deliver()
    return out


def expected(subs: Sequence[dict], n: int, L: int, natural: Optional[Dict[int, int]] = None, cancel: Sequence[int] = ()):
    """What ``play`` has to deliver, written down from the issue's semantics without any row, ring or pass: sequence q continues its
    prompt with the tokens of model_token at (position = step = len - 1, own keys), until EOS at its natural length, a stop token, or
    its limit - which counts the prompt; a sequence cancelled before its first step is its prompt alone with the length word -P."""
    natural = natural or {}
    out, q = {}, 0
    for sub in subs:
        for i in range(sub["m"]):
            row0 = [BOS] if sub.get("prompt") is None else [int(t) for t in sub["prompt"][i]]
            for _ in range(n):
                row, limit = list(row0), sub.get("max_length") or L
                if q in cancel:
                    out[q] = (row, -len(row))
                else:
                    while True:
                        ln = len(row)
                        tok = EOS if ln + 1 == natural.get(q, -1) else model_token(q, ln - 1, ln - 1, row[-1], True)
                        row.append(tok)
                        if tok == EOS or tok in sub.get("stop", ()) or len(row) >= limit:
                            break
                    out[q] = (row, len(row))
                q += 1
    return out


# ------------------------------------------------------------------------------------------------ what the GPU tests run
# The kernel test (tests/test_gpu_roll_prompt_kernels.py): n = 2, Cf = 3, C = 6, max_prompt_length 6, L = 9.  The ring holds sequences
# 8 .. 13: feature rows 4, 5, 6 in ring rows 1, 2, 0 (the prompt and ukv rings wrap inside the submit of 10 .. 13) and id rows 2, 3, 4,
# 5, 0, 1 (the output ring wraps there too).  Prompt lengths: ring row 1 -> 2, ring row 2 -> 6 (= max_prompt_length), ring row 0 -> 1.
# The five rows under test are F .. F + 4, F = 0 at R = 5 and F = 253 at R = 300 - rows 253 .. 255 end the first 256-row pass of the
# workgroup, 256 and 257 start the second; every other row holds sequence 10 at 6 tokens and goes on (the same id cell, the same token).
HOOK_N, HOOK_CF, HOOK_MP, HOOK_L = 2, 3, 6, 9
HOOK_PLEN = (1, 2, 6)
T_GO = 777


def hook_rings(seed: int = 5):
    rng = np.random.default_rng(seed)
    ptok = rng.integers(0, 50257, size=(HOOK_CF, HOOK_MP)).astype(np.int32)
    ptok[2, 2], ptok[2, 4] = EOS, 4242          # an EOS and a stop token INSIDE the prompt of sequences 10 and 11
    return ptok, np.array(HOOK_PLEN, dtype=np.int32)


def hook_cases(R: int):
    """(name, S_before, submit, handout, retire, state, arg, request ring) at R rows, C = 6, n = 2."""
    assert R in (5, 300)
    F, C, L = (0 if R == 5 else 253), HOOK_CF * HOOK_N, HOOK_L

    def state(rows, nxt, unfinished):
        st = new_state(R)
        st["seq"][:], st["len"][:], st["tok"][:], st["pos"][:], st["step"][:] = 10, 6, 1234, 5, 5
        for i, (q, ln) in enumerate(rows):
            r = F + i
            st["seq"][r], st["len"][r] = q, ln
            st["tok"][r], st["pos"][r], st["step"][r] = (BOS, 0, 0) if q < 0 else (2000 + r, ln - 1, ln - 1)
        st["shared"][:] = (nxt, unfinished, 0, 3)
        return st

    arg = np.full(R, T_GO, dtype=np.int32)
    out = []
    # 1. a submit of 10 .. 13 and the hand-out pass: rows F + 1, F + 3, F + 4 are idle and take 10 (P = 6), 11 (P = 6), 12 (P = 1); 13 stays
    #    pending; rows F and F + 2 hold 8 and 9 and are not touched
    out.append(("submit_handout", 10, 4, 1, 0, state([(8, 3), (-1, 0), (9, 4), (-1, 0), (-1, 0)], 10, 2), arg.copy(), Q.new_ring(C, L)))
    # 2. a retire pass on what 1 leaves: 8 ends (EOS) and 13 (P = 1) takes its row; 10 - EOS and the stop token 4242 inside its prompt -
    #    goes on; 9 is cancelled at 4 tokens; 11 has max_length 7 = P + 1 and ends with its first token; 12 gets its stop token
    ring = Q.new_ring(C, L)
    Q.set_request(ring, 10, stop=[4242])
    Q.set_request(ring, 9, cancel=True)
    Q.set_request(ring, 11, max_length=7, stop=[4242])
    Q.set_request(ring, 12, stop=[31])
    a2 = arg.copy()
    a2[F:F + 5] = (EOS, T_GO, T_GO, T_GO, 31)
    out.append(("retire_and_seat", 14, 0, 0, 1, state([(8, 3), (10, 6), (9, 4), (11, 6), (12, 1)], 13, 6), a2, ring))
    # 3. a prompted sequence cancelled before its first step: 11 sits in its row at len = P = 6 and is cut to the prompt alone (-6);
    #    nothing is pending, so the row idles
    ring = Q.new_ring(C, L)
    Q.set_request(ring, 11, cancel=True)
    out.append(("cancel_before_first_step", 14, 0, 0, 1, state([(13, 2), (10, 6), (-1, 0), (11, 6), (12, 3)], 14, 5), arg.copy(), ring))
    # 4. a step without refills: every row goes on
    out.append(("no_refills", 14, 0, 0, 1, state([(13, 2), (10, 6), (-1, 0), (11, 6), (12, 3)], 14, 5), arg.copy(), Q.new_ring(C, L)))
    return out


# ------------------------------------------------------------------------------------------------ the greedy oracle
def oracle_greedy(sd, prompts, feats, max_length):
    """greedy_search of the restated reference for prompts WITHOUT padding: ``prompts`` a list of S 1-D int64 tensors (ragged),
    ``feats`` [S, 1024], ``max_length`` an int or one per sequence, counting the prompt.  Sequences of equal (P, limit) run as one
    batch with a mask of ones.  -> (ids: list of S 1-D tensors, each ending with its EOS or at its limit; the smallest top-2 logit gap
    over the generated positions of rows that had not finished)."""
    import torch
    from oracle import language_model as o_lm

    S = len(prompts)
    limits = [int(max_length)] * S if isinstance(max_length, int) else [int(v) for v in max_length]
    out: List = [None] * S
    gap = float("inf")
    groups: Dict[Tuple[int, int], List[int]] = {}
    for s in range(S):
        groups.setdefault((int(prompts[s].shape[0]), limits[s]), []).append(s)
    with torch.no_grad():
        for (P, limit), rows in sorted(groups.items()):
            assert 1 <= P < limit
            ids = torch.stack([prompts[s].to(torch.int64) for s in rows])
            f = feats[rows].to(torch.float32)
            done = torch.zeros(len(rows), dtype=torch.bool)
            past = None
            while ids.shape[1] < limit and not bool(done.all()):
                T = ids.shape[1]
                attn = torch.ones((len(rows), T), dtype=torch.int64)
                pos = torch.arange(T)[None, :].expand(len(rows), T)
                logits, past = o_lm.lm_forward(sd, ids if past is None else ids[:, -1:], attn, f, past, pos if past is None else pos[:, -1:])
                top2 = torch.topk(logits[:, -1, :].double(), 2, dim=-1).values
                live = ~done
                gap = min(gap, float((top2[live, 0] - top2[live, 1]).min()))
                nxt = torch.argmax(logits[:, -1, :], dim=-1)
                nxt = torch.where(done, torch.full_like(nxt, PAD), nxt)
                ids = torch.cat([ids, nxt[:, None]], dim=-1)
                done = done | (nxt == EOS)
            for i, s in enumerate(rows):
                row = ids[i].tolist()
                end = next((j + 1 for j in range(P, len(row)) if row[j] == EOS), len(row))
                out[s] = ids[i, :end].clone()
    return out, gap
