"""CPU references of DIVERSE (grouped) beam search.  TEST INFRASTRUCTURE ONLY.

``group_beam_search``: transformers 4.19.2 ``group_beam_search`` with its ``HammingDiversityLogitsProcessor``, restated over
``oracle.language_model._lm_forward_beams`` and ``oracle.beam_scorer.BeamSearchScorer(num_beam_groups=G)`` (transformers 4.19.2 is
not installed: PARITY UNPINNED against a real install, like the scorer itself).  Prompt, mask and positions are handled as in
``prompt_beam_reference.beam_search``; without a prompt the search starts from a BOS column.

``merge_reference``: the arithmetic contract of ``beam_group_merge_kernel`` (include/rgrg_hip.h "Diverse beam search") in numpy
float32, operation by operation, on the row candidate lists that ``beam_row_topk_kernel`` leaves.

``brute_force_merge``: the same ranking over FULL penalised rows - what shows that the row lists are enough.

``merge_inputs``: the inputs of the kernel test (tests/test_gpu_group_beam.py) and of its CPU twin."""
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import language_model as o_lm
from oracle.beam_scorer import BeamSearchScorer
from prompt_beam_reference import expand
from prompt_reference import positions_from_mask

EOS = PAD = BOS = o_lm.EOS
V_MODEL = o_lm.VOCAB
BEAM_K = 32          # width of a candidate row in the decoder (rgrg_amd/csrc/decoder_internal.h)
MIN_GAP = 2e-3       # the project's bound on what an fp32 ranking may be asked to separate (tests/golden/make_golden_lm_prompt_beam.py)


@torch.no_grad()
def group_beam_search(sd, image_hidden_states: torch.Tensor, max_length: int, num_beams: int, num_beam_groups: int,
                      diversity_penalty: float, early_stopping: bool = False, num_return_sequences: int = 1,
                      input_ids: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None, return_gap: bool = False,
                      stop_below: float = 0.0, return_trace: bool = False):
    """-> int64 [S * num_return_sequences, L].  input_ids / attention_mask [S,T]: ONE prompt per item (expanded here), or None = a
    BOS column.  ``return_gap``: also the smallest difference between adjacent entries of the top 2 * group_size + 1 PENALISED
    candidate scores over every step, group and (at that group) unfinished item; ``stop_below``: give up - (None, gap) - as soon as
    that gap falls below it.  ``return_trace``: also, per step, the ``done`` flags seen by every group [G][S]."""
    S = image_hidden_states.shape[0]
    nb, G = int(num_beams), int(num_beam_groups)
    gs = nb // G
    if input_ids is None:
        input_ids = torch.full((S, 1), BOS, dtype=torch.int64)
        attention_mask = torch.ones((S, 1), dtype=torch.int64)
    scorer = BeamSearchScorer(batch_size=S, num_beams=nb, length_penalty=1.0, do_early_stopping=early_stopping,
                              num_beam_hyps_to_keep=num_return_sequences, num_beam_groups=G)
    ids = expand(input_ids.clone(), nb)
    attn = expand(attention_mask.clone().to(torch.int64), nb)
    beam_scores = torch.full((S, nb), -1e9, dtype=torch.float)
    beam_scores[:, ::gs] = 0
    beam_scores = beam_scores.view(-1)
    lam = torch.tensor(float(diversity_penalty), dtype=torch.float32)
    past, cur_len, gap, trace = None, ids.shape[1], float("inf"), []
    while True:
        pos = positions_from_mask(attn)
        inp = ids if past is None else ids[:, -1:]
        if past is not None:
            pos = pos[:, -1:]
        logits, past = o_lm._lm_forward_beams(sd, inp, attn, image_hidden_states, past, pos, nb, "language_model.")
        logits = logits[:, -1, :]
        V = logits.shape[-1]
        current_tokens = torch.zeros((S * nb,), dtype=torch.int64)
        reordering_indices = torch.zeros((S * nb,), dtype=torch.int64)
        seen_done = []
        for g in range(G):
            start = g * gs
            rows = torch.tensor([b * nb + i for b in range(S) for i in range(start, start + gs)])
            group_ids = ids[rows]
            logp = F.log_softmax(logits[rows], dim=-1)
            if g > 0:   # HammingDiversityLogitsProcessor: the tokens the earlier groups of the item took in THIS step
                for b in range(S):
                    freq = torch.bincount(current_tokens[b * nb:b * nb + start], minlength=V)
                    logp[b * gs:(b + 1) * gs] -= lam * freq.to(torch.float32)
            flat = (logp + beam_scores[rows][:, None]).view(S, gs * V)
            seen_done.append(scorer._done.clone())
            if return_gap:
                top = torch.topk(flat, 2 * gs + 1, dim=1).values
                live = ~scorer._done
                if live.any():
                    gap = min(gap, float((top[live, :-1] - top[live, 1:]).min()))
                if gap < stop_below:
                    return None, gap
            scores, tokens = torch.topk(flat, 2 * gs, dim=1, largest=True, sorted=True)
            indices = torch.div(tokens, V, rounding_mode="floor")
            tokens = tokens % V
            out = scorer.process(group_ids, scores, tokens, indices, pad_token_id=PAD, eos_token_id=EOS)
            beam_scores[rows] = out["next_beam_scores"]
            beam_tok, beam_idx = out["next_beam_tokens"], out["next_beam_indices"]
            ids[rows] = group_ids[beam_idx]
            current_tokens[rows] = beam_tok
            reordering_indices[rows] = nb * torch.div(beam_idx, gs, rounding_mode="floor") + start + (beam_idx % gs)
        trace.append(torch.stack(seen_done))
        ids = torch.cat([ids, current_tokens[:, None]], dim=-1)
        attn = torch.cat([attn, attn.new_ones((attn.shape[0], 1))], dim=-1)
        past = [(k.index_select(0, reordering_indices), v.index_select(0, reordering_indices)) for k, v in past]
        cur_len += 1
        if scorer.is_done or cur_len >= max_length:
            break
    seq = scorer.finalize(ids, beam_scores, tokens, indices, pad_token_id=PAD, eos_token_id=EOS, max_length=max_length)["sequences"]
    ret = (seq,)
    if return_gap:
        ret += (gap,)
    if return_trace:
        ret += (trace,)
    return ret if len(ret) > 1 else seq


# ---------------------------------------------------------------------------------------------- the kernel's contract
f32 = np.float32


def _rank(scores, flats, count):
    """Indices of the first ``count`` candidates in the order (score descending, flat index ascending)."""
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), int(flats[i])))
    return order[:count]


def merge_reference(row_max, row_logsum, top_val, top_tok, beam_scores, S, nb, G, penalty, V, eos=EOS, info=None, fused=False):
    """-> (score f32 [S, 2 nb], token i32 [S, 2 nb], beam i32 [S, 2 nb]): group g of item s in columns g * 2 gs .. (g + 1) * 2 gs - 1,
    ``beam`` = the row within the item.  Per candidate, fp32, every operation rounded once:
    ``((v - row_max) - row_logsum) - round(penalty * float(freq)) + beam_score``.  ``info`` (a dict) collects what the inputs
    exercised: the largest freq applied to a ranked candidate, ranks of EOS, listed candidates that a penalty pushed out.
    ``fused``: NOT the contract - the penalty as one fused multiply-subtract, ``fma(-penalty, freq, logp)`` with an exact product and
    one rounding, what a compiler that contracts the two operations computes; tests use it to show that their inputs tell the two
    apart."""
    gs, K = nb // G, 2 * nb
    lam = f32(penalty)
    out_s = np.zeros((S, K), f32)
    out_t = np.zeros((S, K), np.int32)
    out_b = np.zeros((S, K), np.int32)
    for s in range(S):
        chosen = []
        for g in range(G):
            sc, fl, tk, bm, plain, fr = [], [], [], [], [], []
            for bi in range(gs):
                row = s * nb + g * gs + bi
                for k in range(K):
                    tok = int(top_tok[row, k])
                    logp = f32(f32(f32(top_val[row, k]) - f32(row_max[row])) - f32(row_logsum[row]))
                    freq = chosen.count(tok)
                    if fused:
                        lowered = f32(np.float64(logp) - np.float64(lam) * freq)   # (24 x 5 bits: the product is exact in float64)
                    else:
                        lowered = f32(logp - f32(lam * f32(freq)))
                    sc.append(f32(lowered + f32(beam_scores[row])))
                    fr.append(freq)
                    plain.append(f32(logp + f32(beam_scores[row])))
                    fl.append(bi * V + tok)
                    tk.append(tok)
                    bm.append(g * gs + bi)
            order = _rank(sc, fl, 2 * gs)
            picked = 0
            for r, i in enumerate(order):
                c = g * 2 * gs + r
                out_s[s, c], out_t[s, c], out_b[s, c] = sc[i], tk[i], bm[i]
                if tk[i] != eos and picked < gs:
                    chosen.append(tk[i])
                    picked += 1
            if info is not None:
                info["max_freq"] = max(info.get("max_freq", 0), max(fr[i] for i in order))   # freq as APPLIED to a ranked candidate
                info.setdefault("eos_ranks", set()).update(("lt" if r < gs else "ge") for r, i in enumerate(order) if tk[i] == eos)
                unpen = set(_rank(plain, fl, 2 * gs))
                info["pushed_out"] = info.get("pushed_out", 0) + len(unpen - set(order))
                info["row_ties"] = info.get("row_ties", 0) + sum(
                    1 for a, b in zip(order[:-1], order[1:]) if sc[a] == sc[b] and bm[a] != bm[b])
                info["minus_1e9"] = info.get("minus_1e9", 0) + int(any(float(beam_scores[s * nb + g * gs + bi]) == -1e9 for bi in range(gs)))
    return out_s, out_t, out_b


def row_lists(logits, K, width=BEAM_K):
    """What beam_row_topk_kernel leaves for logits f32 [R, V]: row_max, row_logsum (any fixed fp32 evaluation serves: both rankings
    below read THESE values), and the top K (value descending, token ascending) of every row in rows ``width`` wide."""
    R, V = logits.shape
    row_max = logits.max(1).astype(f32)
    row_logsum = np.log(np.exp(logits - row_max[:, None], dtype=f32).sum(1, dtype=f32)).astype(f32)
    top_val = np.zeros((R, width), f32)
    top_tok = np.zeros((R, width), np.int32)
    for r in range(R):
        order = sorted(range(V), key=lambda t: (-float(logits[r, t]), t))[:K]
        top_val[r, :K] = logits[r, order]
        top_tok[r, :K] = order
    return row_max, row_logsum, top_val, top_tok


def brute_force_merge(logits, row_max, row_logsum, beam_scores, S, nb, G, penalty, eos):
    """``merge_reference``'s result computed over the FULL rows: every one of the gs * V penalised candidates of a group is ranked."""
    R, V = logits.shape
    gs, K = nb // G, 2 * nb
    lam = f32(penalty)
    out_s = np.zeros((S, K), f32)
    out_t = np.zeros((S, K), np.int32)
    out_b = np.zeros((S, K), np.int32)
    for s in range(S):
        freq = np.zeros(V, np.int64)
        for g in range(G):
            rows = [s * nb + g * gs + bi for bi in range(gs)]
            pen = (lam * freq.astype(f32)).astype(f32)
            sc = np.concatenate([((((logits[r] - row_max[r]).astype(f32) - row_logsum[r]).astype(f32) - pen).astype(f32)
                                  + f32(beam_scores[r])).astype(f32) for r in rows])
            order = _rank(sc, np.arange(gs * V), 2 * gs)
            picked = []
            for r, i in enumerate(order):
                c = g * 2 * gs + r
                out_s[s, c], out_t[s, c], out_b[s, c] = sc[i], i % V, g * gs + i // V
                if i % V != eos and len(picked) < gs:
                    picked.append(i % V)
            for t in picked:
                freq[t] += 1
    return out_s, out_t, out_b


MERGE_CASES = ((2, 2), (4, 2), (4, 4), (6, 3), (16, 2), (16, 16), (16, 1), (3, 1))
MERGE_S = 3


def merge_inputs(nb, G, seed=0, V=V_MODEL, eos=EOS):
    """Candidate rows of S = 3 items as the decoder holds them (rows BEAM_K wide, the first 2 nb entries sorted value descending,
    token ascending), built to reach every branch of the ranking:
      item 0  the start of a search: beam score 0 on the first row of every group, -1e9 elsewhere, the first rows EQUAL - every
              later group meets the tokens of the earlier ones (freq up to the number of earlier beams), penalised candidates
              leave the top 2 gs;
      item 1  values, log-sums and beam scores on a grid of 1/8 with copied rows inside a group: equal scores in different rows,
              which only the flat index beam * V + token separates; tokens from a small pool that holds EOS, so EOS appears at
              every rank and tokens repeat between groups;
      item 2  unquantised values and beam scores: every operation of the contract rounds.  With one row per group and at least 6
              groups, every row holds the same tokens with one dominant token, so group after group takes that token and its
              ranked candidates carry freq 5, 7, 9 .. - the counts at which round(0.3f * freq) is inexact (0.3f * freq is exact
              for freq 1, 2, 3, 4, 6 and 0.5f * freq always), where a fused multiply-subtract rounds differently.
    -> dict of numpy arrays row_max, row_logsum [R], top_val f32 / top_tok i32 [R, BEAM_K], beam_scores [R]."""
    rng = np.random.RandomState(1000 * nb + 10 * G + seed)
    S, gs, K = MERGE_S, nb // G, 2 * nb
    R = S * nb
    top_val = np.full((R, BEAM_K), -np.inf, f32)
    top_tok = np.full((R, BEAM_K), 0x7fffffff, np.int32)
    row_max = np.zeros(R, f32)
    row_logsum = np.zeros(R, f32)
    beam_scores = np.zeros(R, f32)
    pool = np.concatenate([rng.choice(V - 1, size=K + nb, replace=False), [eos]]).astype(np.int64)

    def fill(row, vals, toks):
        order = sorted(range(K), key=lambda i: (-float(vals[i]), int(toks[i])))
        top_val[row, :K] = np.asarray(vals, f32)[order]
        top_tok[row, :K] = np.asarray(toks)[order]
        row_max[row] = top_val[row, 0]

    # item 0
    vals0 = (rng.randint(0, 6 * K, size=K) / f32(8)).astype(f32)
    toks0 = rng.choice(pool, size=K, replace=False)
    for b in range(nb):
        r = b
        if b % gs == 0:
            fill(r, vals0, toks0)
            row_logsum[r] = f32(1.25)
            beam_scores[r] = 0.0
        else:
            fill(r, (rng.randint(0, 6 * K, size=K) / f32(8)).astype(f32), rng.choice(pool, size=K, replace=False))
            row_logsum[r] = f32(rng.randint(4, 24) / 8)
            beam_scores[r] = -1e9
    # item 1
    for b in range(nb):
        r = nb + b
        if b % gs == 1:   # a copy of the group's first row: equal scores in two rows
            top_val[r], top_tok[r], row_max[r], row_logsum[r], beam_scores[r] = top_val[r - 1], top_tok[r - 1], row_max[r - 1], row_logsum[r - 1], beam_scores[r - 1]
            continue
        fill(r, (rng.randint(0, 3 * K, size=K) / f32(8)).astype(f32), rng.choice(pool, size=K, replace=False))
        row_logsum[r] = f32(rng.randint(4, 24) / 8)
        beam_scores[r] = f32(-rng.randint(0, 6) / 8)
    # item 2
    dominant = gs == 1 and nb >= 6
    toks2 = rng.choice(pool[:-1], size=K, replace=False)
    for b in range(nb):
        r = 2 * nb + b
        vals = (rng.standard_normal(K) * 2 + 6).astype(f32)
        if dominant:
            vals[0] = f32(vals.max() + 0.3 * nb + 1 + rng.random_sample())   # stays in the top 2 under every group's penalty
        fill(r, vals, toks2 if dominant else rng.choice(pool, size=K, replace=False))
        row_max[r] = f32(top_val[r, 0] + abs(rng.standard_normal()))
        row_logsum[r] = f32(1 + rng.random_sample() * 3)
        beam_scores[r] = f32(-rng.random_sample() * 4)
    return dict(row_max=row_max, row_logsum=row_logsum, top_val=top_val, top_tok=top_tok, beam_scores=beam_scores)


# ---------------------------------------------------------------------------------------------- recorded end-to-end cases
def feats_of(seed, S=1):
    return torch.randn((S, 1024), generator=torch.Generator().manual_seed(seed))


def item_feats(seeds):
    """One feature row per seed: items are independent, so every item's seed was walked on its own."""
    return torch.cat([feats_of(s) for s in seeds], 0)


# Seeds walked per item on the CPU (items are independent): feature row = torch.randn((1, 1024), generator=manual_seed(seed)), and,
# for a prompted case, the item's prompt drawn from the same generator BEFORE the features.  ``batch_seed``: the rows of the whole
# batch from one generator instead.  ``gap``: what ``group_beam_search(return_gap=True)`` measured when the case was recorded -
# tests/test_group_beam_reference.py recomputes it and holds it to MIN_GAP.
CASES = {
    # contains hypotheses that finish in the first steps
    "ragged_s2_b4_g2": dict(profile="ragged", batch_seed=(301, 2), nb=4, G=2, lam=0.5, L=7, early=False, gap=0.0024),
    "bench_s1_b6_g3": dict(profile="bench", batch_seed=(305, 1), nb=6, G=3, lam=0.3, L=6, early=False, gap=0.0021),
    "early_s2_b4_g2": dict(profile="ragged", seeds=(313, 310), nb=4, G=2, lam=0.5, L=7, early=True, gap=0.0034),
    # EOS-boosted weights: item 0 becomes `done` in group 0 of a step while group 1 of that step is still to be processed
    "done_flip_s2_b4_g2": dict(profile="ragged", eos_boost=1.05, seeds=(333, 330), nb=4, G=2, lam=0.5, L=7, early=True, gap=0.0042,
                               flips=True),
    # 33 items x 4 beams = 132 rows; the items compared are [0, 1, 32]
    "many_s33_b4_g2": dict(profile="ragged", seeds=(433, 446) + tuple(range(1002, 1032)) + (451,), rows=(0, 1, 32), nb=4, G=2, lam=0.5,
                           L=7, early=False, gap=0.0020),
    # left-padded ragged prompt, T = 4
    "prompt_s3_t4_b4_g2": dict(profile="ragged", seeds=(500, 541, 580), T=4, pads=(0, 1, 3), nb=4, G=2, lam=0.5, L=8, early=False,
                               gap=0.0027),
}


def case_inputs(name):
    """-> (feats [S,1024], input_ids [S,T] or None, attention_mask [S,T] or None) of a recorded case, all items."""
    c = CASES[name]
    if "batch_seed" in c:
        seed, S = c["batch_seed"]
        return feats_of(seed, S), None, None
    feats, ids, masks = [], [], []
    for i, seed in enumerate(c["seeds"]):
        g = torch.Generator().manual_seed(seed)
        if "T" in c:
            T, pad = c["T"], c["pads"][i]
            row = torch.randint(0, 50000, (1, T), generator=g)
            m = torch.ones((1, T), dtype=torch.int64)
            m[0, :pad] = 0
            row[0, :pad] = EOS
            ids.append(row)
            masks.append(m)
        feats.append(torch.randn((1, 1024), generator=g))
    return torch.cat(feats, 0), (torch.cat(ids, 0) if ids else None), (torch.cat(masks, 0) if masks else None)


def case_weights(name, synth_sd):
    c = CASES[name]
    sd = synth_sd(c["profile"])
    if "eos_boost" in c:
        from prompt_reference import eos_boosted
        sd = eos_boosted(sd, c["eos_boost"])
    return sd


_CASE_REF = {}


def case_reference(name, synth_sd):
    """The CPU loop on a recorded case (the compared items only), num_return_sequences = num_beams: computed once per session.
    -> dict(seq, gap, trace, feats, ids, mask) with feats / ids / mask of the compared items."""
    if name not in _CASE_REF:
        c = CASES[name]
        feats, ids, mask = case_inputs(name)
        rows = list(c.get("rows", range(feats.shape[0])))
        f, i, m = feats[rows], (None if ids is None else ids[rows]), (None if mask is None else mask[rows])
        seq, gap, trace = group_beam_search(case_weights(name, synth_sd), f, c["L"], c["nb"], c["G"], c["lam"], c["early"], c["nb"], i, m,
                                            return_gap=True, return_trace=True)
        _CASE_REF[name] = dict(seq=seq, gap=gap, trace=trace, feats=f, ids=i, mask=m)
    return _CASE_REF[name]
