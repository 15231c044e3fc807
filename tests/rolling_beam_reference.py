"""Model of rolling-batch beam search (rgrg_decoder_beam_search_rolling) for the tests: the host schedule - seat,
process, leave, finalize, padded width - fed with the per-region candidate traces of ``oracle.language_model.beam_generate(...,
return_trace=True)``, and the numpy rule of the turn kernel.

Regions are independent, so the candidates region s ranks at ITS k-th iteration are ``trace[k][..][s]`` whichever step and slot
runs that iteration; the lock-step trace of a region is valid up to the iteration at which the region leaves, and the model never
reads past it.  The heap is the oracle's ``BeamHypotheses`` (one copy of the HF semantics on the test side as well).

``schedule(..., mutate=NAME)`` applies one named defect; tests/test_rolling_beam_reference.py shows that every one of them is
rejected by the equality with ``beam_generate`` or by ``check_log``."""
import numpy as np
import torch

from oracle.beam_scorer import BeamHypotheses

BOS = EOS = PAD = 50256
FRESH, IDLE = -1, -2
MUTATIONS = ("late_refill", "stale_heap", "stale_cur_len", "scores_not_reset", "out_of_order", "skip_finalize")


def turn_rule(src_old, src_new, parent, step, nb):
    """beam_roll_turn_kernel on numpy int32 arrays src_old / src_new [R][T], parent / step [R] -> (src_new, step) after the launch."""
    new, st = src_new.copy(), step.copy()
    for r in range(len(parent)):
        p = int(parent[r])
        if p == IDLE:
            st[r] = 0
        elif p == FRESH:
            new[r, 0] = r // nb * nb
            st[r] = 0
        else:
            t = int(step[p])          # all rows of a slot share t
            new[r, :t + 1] = src_old[p, :t + 1]
            new[r, t + 1] = p
            st[r] = t + 1
    return new, st


def bound(S, G, max_length):
    return (-(-S // G) + 1) * (max_length - 1)


def schedule(trace, S, nb, G, max_length, early, keep=1, lp=1.0, mutate=None):
    """-> {"seq": int64 [S * keep, L], "steps", "leave": iteration count of every region (0 = never seated), "log"}.  log: one entry
    per step, a list over the slots of None (idle) or (region, k, tokens, scores, turns) - what the host writes for the slot's nb
    rows in front of the step: k = the region's iteration, turns relative to the slot's first row (FRESH at k = 0)."""
    hyps = [BeamHypotheses(nb, lp, early) for _ in range(S)]
    region, cur_len, done = [-1] * G, [1] * G, [False] * G
    ids = [[None] * nb for _ in range(G)]
    scores = [[0.0] * nb for _ in range(G)]
    toks = [[BOS] * nb for _ in range(G)]
    turns = [[IDLE] * nb for _ in range(G)]
    pending = list(range(S))
    if mutate == "out_of_order":
        pending.reverse()
    leave = [0] * S
    fresh_scores = np.array([0.0] + [-1e9] * (nb - 1), dtype=np.float32)

    def seat(g):
        given, prev = bool(pending), region[g]
        region[g] = pending.pop(0) if given else -1
        if mutate != "stale_cur_len" or prev < 0:
            cur_len[g] = 1
        done[g] = False
        ids[g] = [torch.tensor([BOS]) for _ in range(nb)]
        toks[g] = [BOS] * nb
        if mutate != "scores_not_reset" or prev < 0:
            scores[g] = [float(x) for x in fresh_scores] if given else [0.0] * nb
        turns[g] = [FRESH if given else IDLE] * nb
        if given and prev >= 0 and mutate == "stale_heap":
            hyps[region[g]].beams, hyps[region[g]].worst_score = list(hyps[prev].beams), hyps[prev].worst_score

    for g in range(G):
        seat(g)
    steps, finished, log = 0, 0, []
    while finished < S:
        assert steps < 10 * bound(S, min(G, S), max_length), "the schedule does not end"
        log.append([None if region[g] < 0 else (region[g], leave[region[g]], tuple(toks[g]), tuple(scores[g]), tuple(turns[g]))
                    for g in range(G)])
        steps += 1
        for g in range(G):
            s = region[g]
            if s < 0:
                continue
            k = leave[s]                                   # the region's iteration
            sc, tk, ix = (t[s] for t in trace[k])
            nscore, ntok, nidx = [], [], []
            for rank in range(2 * nb):
                if int(tk[rank]) == EOS:
                    if rank >= nb:
                        continue
                    hyps[s].add(ids[g][int(ix[rank])].clone(), sc[rank].item())
                else:
                    nscore.append(float(sc[rank])); ntok.append(int(tk[rank])); nidx.append(int(ix[rank]))
                if len(ntok) == nb:
                    break
            assert len(ntok) == nb
            done[g] = done[g] or hyps[s].is_done(sc.max().item(), cur_len[g])
            ids[g] = [torch.cat([ids[g][nidx[j]], torch.tensor([ntok[j]])]) for j in range(nb)]
            scores[g], toks[g], turns[g] = nscore, ntok, nidx
            cur_len[g] += 1
            leave[s] += 1
        for g in range(G):
            s = region[g]
            if s >= 0:
                if not done[g] and cur_len[g] < max_length:
                    continue
                if not done[g] and mutate != "skip_finalize":   # BeamSearchScorer.finalize: the open beams of an undone region
                    for j in range(nb):
                        hyps[s].add(ids[g][j], scores[g][j])
                finished += 1
                if mutate == "late_refill":   # the slot idles for one step before it takes the next region
                    region[g], turns[g], toks[g], scores[g] = -1, [IDLE] * nb, [BOS] * nb, [0.0] * nb
                    continue
            seat(g)
    best = []
    for h in hyps:
        ranked = sorted(h.beams, key=lambda x: x[0])
        assert len(ranked) >= keep, "a region has fewer finished hypotheses than requested"
        for _ in range(keep):
            best.append(ranked.pop()[1])
    L = min(max(len(b) for b in best) + 1, max_length)
    seq = torch.full((S * keep, L), PAD, dtype=torch.int64)
    for i, b in enumerate(best):
        seq[i, :len(b)] = b
        if len(b) < max_length:
            seq[i, len(b)] = EOS
    return {"seq": seq, "steps": steps, "leave": leave, "log": log}


def lockstep_inputs(trace, S, nb, max_length, early):
    """What the rows of region s must be fed in front of its iteration k, derived with the ORACLE's scorer run in lock step over the
    trace: {(s, k): (tokens, scores, turns)}, k = 0 the fresh state, for every iteration the region runs before it leaves, and
    -> also the iteration count of every region."""
    from oracle.beam_scorer import BeamSearchScorer
    scorer = BeamSearchScorer(batch_size=S, num_beams=nb, length_penalty=1.0, do_early_stopping=early)
    ids = torch.full((S * nb, 1), BOS, dtype=torch.int64)
    want, iters = {}, [0] * S
    for s in range(S):
        want[(s, 0)] = ((BOS,) * nb, (0.0,) + (float(np.float32(-1e9)),) * (nb - 1), (FRESH,) * nb)
    cur_len = 1
    for k, (sc, tk, ix) in enumerate(trace):
        was_done = scorer._done.clone()
        out = scorer.process(ids, sc, tk, ix, pad_token_id=PAD, eos_token_id=EOS)
        ids = torch.cat([ids[out["next_beam_indices"], :], out["next_beam_tokens"].unsqueeze(-1)], dim=-1)
        cur_len += 1
        for s in range(S):
            if was_done[s]:
                continue
            iters[s] = k + 1
            if not scorer._done[s] and cur_len < max_length:
                r = slice(s * nb, (s + 1) * nb)
                want[(s, k + 1)] = (tuple(out["next_beam_tokens"][r].tolist()), tuple(float(x) for x in out["next_beam_scores"][r]),
                                    tuple((out["next_beam_indices"][r] - s * nb).tolist()))
        if scorer.is_done or cur_len >= max_length:
            break
    return want, iters


def check_log(res, S, G, want, iters):
    """The schedule properties the equality of the sequences does not see: every region runs its iterations 0 .. n - 1 in ONE slot
    on consecutive steps, fed what lock step feeds it; regions are seated in ascending order, free slots taken in ascending slot
    order; no slot idles while a region is pending."""
    log = res["log"]
    seen, where, last_seated = {}, {}, -1
    for t, slots in enumerate(log):
        seated_now = [e[0] for e in slots if e is not None and e[1] == 0]
        assert seated_now == sorted(seated_now), f"step {t}: regions {seated_now} are not in ascending slot order"
        for s in seated_now:
            assert s == last_seated + 1, f"step {t}: region {s} seated after region {last_seated}"
            last_seated = s
        if any(e is None for e in slots):
            assert last_seated == S - 1, f"step {t}: a slot idles while region {last_seated + 1} is pending"
        for g, e in enumerate(slots):
            if e is None:
                continue
            s, k, tk, sc, tu = e
            assert seen.get(s, 0) == k, f"step {t}: region {s} at iteration {k}, expected {seen.get(s, 0)}"
            assert k == 0 or where[s] == (g, t - 1), f"step {t}: region {s} moved or paused"
            assert (s, k) in want, f"step {t}: region {s} runs iteration {k} after it should have left"
            assert (tk, sc, tu) == want[(s, k)], f"step {t}: region {s} iteration {k} is fed {(tk, sc, tu)}, lock step feeds {want[(s, k)]}"
            seen[s], where[s] = k + 1, (g, t)
    assert [seen.get(s, 0) for s in range(S)] == list(iters), "iterations per region differ from lock step"
