"""The numpy model of prompts in a rolling session (tests/rolling_prompt_reference.py) against the semantics written down without
rows, rings or passes (``expected``), the seating rule spelled out on the kernel test's cases, and the named mutations: every wrong
rule is rejected by a case the GPU tests run (the hook cases of tests/test_gpu_roll_prompt_kernels.py, or a schedule of the kind
tests/test_gpu_roll_prompts.py drives).  No GPU."""
import numpy as np
import pytest

import rolling_prompt_reference as P

EOS = P.EOS
L, MP = 12, 6


def _prompts(count, lens, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        p = rng.integers(0, 50000, size=lens[i % len(lens)]).tolist()
        out.append(p)
    return out


def _schedule(seed=3):
    """Ragged prompts as separate submits (one P per submit), a submit without a prompt, one with a limit of its own, one with a stop
    token that also sits INSIDE its prompt, and an EOS inside a prompt."""
    pr = _prompts(6, (1, 3, 2, 5, 4, 6), seed)
    pr[3][2] = EOS                       # an EOS inside the prompt ends nothing
    stop = P.model_token(5, 6, 6, 0, True)      # never hit by accident; the hit is placed in the prompt
    pr[5][1] = 4242
    return [dict(m=1, prompt=[pr[0]]), dict(m=2, prompt=[pr[1], pr[1][::-1]]), dict(m=1, prompt=None), dict(m=1, prompt=[pr[3]], max_length=7),
            dict(m=1, prompt=[pr[4]], max_length=5), dict(m=1, prompt=[pr[5]], stop=[4242, stop]), dict(m=2, prompt=[pr[2], pr[2]])]


NATURAL = {1: 6, 3: 2, 7: 4}


@pytest.mark.parametrize("R,Cf,n", [(4, 3, 1), (3, 4, 1), (4, 3, 2), (7, 2, 3)])
def test_the_model_delivers_the_semantics(R, Cf, n):
    subs = _schedule()
    natural = {q * n: v for q, v in NATURAL.items()}
    got = P.play(subs, R, Cf, n, L, MP, natural=natural)
    want = P.expected(subs, n, L, natural=natural)
    assert got == want
    lens = [v[1] for v in got.values()]
    assert min(lens) >= 2 and max(lens) == L         # at least one token is always generated; the limit counts the prompt
    q5 = 5 * n                                        # dict(max_length=5) with a prompt of 4 tokens: exactly one generated token
    assert got[q5][1] == 5


def test_cancel_before_the_first_step_delivers_the_prompt_alone():
    subs = _schedule()
    # R = 2: sequences 5 .. are pending while 0 .. run; 6 (a prompt of 6 tokens) is cancelled at once and cut in its row's first pass
    got = P.play(subs, 2, 8, 1, L, MP, cancel=(6, 2))
    want = P.expected(subs, 1, L, cancel=(6, 2))
    assert got == want and got[6][1] == -6 and got[6][0] == subs[5]["prompt"][0] and got[2][1] == -3


def test_the_seating_rule_spelled_out():
    """The kernel test's first case by hand: 10 and 11 (ring row 2, P = 6) and 12 (ring row 0, P = 1) take the idle rows."""
    ptok, plen = P.hook_rings()
    for R in (5, 300):
        name, S_before, submit, handout, retire, st, arg, req = P.hook_cases(R)[0]
        F = 0 if R == 5 else 253
        ids, lens = np.full((6, P.HOOK_L + 1), -1, dtype=np.int64), np.full(6, -99, dtype=np.int32)
        a, b = P.prompt_step(st, arg, ids, lens, None, 6, 2, S_before, submit, handout, retire, P.HOOK_L, ptok, plen, req)
        assert a == [(F + 1, 10, 2, 6), (F + 3, 11, 2, 6), (F + 4, 12, 0, 1)] and b == []
        for r, q, f, p in a:
            assert (st["seq"][r], st["len"][r], st["tok"][r], st["pos"][r], st["step"][r]) == (q, p, ptok[f, p - 1], p - 1, p - 1)
        assert st["tok"][F + 4] == ptok[0, 0] and st["shared"].tolist()[:3] == [13, 1 + R, 3]
        # the id rows: prompt, then PAD; row 10 % 6 = 4 and 11 % 6 = 5 share ring row 2, 12 and 13 (rows 0 and 1) ring row 0
        for q in (10, 11, 12, 13):
            p = int(plen[(q // 2) % 3])
            assert ids[q % 6, :p].tolist() == ptok[(q // 2) % 3, :p].tolist() and (ids[q % 6, p:P.HOOK_L] == EOS).all() and lens[q % 6] == 0
        assert (ids[2:4] == -1).all() and lens[2] == lens[3] == -99        # 8 and 9 are not touched


def test_the_retire_case_spelled_out():
    ptok, plen = P.hook_rings()
    name, S_before, submit, handout, retire, st, arg, req = P.hook_cases(5)[1]
    ids, lens = np.full((6, P.HOOK_L + 1), -1, dtype=np.int64), np.zeros(6, dtype=np.int32)
    _, b = P.prompt_step(st, arg, ids, lens, None, 6, 2, S_before, submit, handout, retire, P.HOOK_L, ptok, plen, req)
    # 8 ended (4 tokens), 9 cut at 4, 10 goes on at 7 although EOS and its stop token are in its prompt, 11 ended at 7 = its limit,
    # 12 ended with its stop token; 13 (P = 1) took row 0, the other freed rows idle
    assert lens.tolist() == [2, 0, 4, -4, 0, 7]
    assert b == [(0, 13, 0, 1)] and st["seq"].tolist() == [13, 10, -1, -1, -1] and st["len"].tolist() == [1, 7, 0, 0, 0]


def _hook_outputs(mut):
    out = []
    ptok, plen = P.hook_rings()
    for R in (5, 300):
        for name, S_before, submit, handout, retire, st0, arg, req in P.hook_cases(R):
            st = {k: v.copy() for k, v in st0.items()}
            ids, lens = np.full((6, P.HOOK_L + 1), -1, dtype=np.int64), np.full(6, -99, dtype=np.int32)
            a, b = P.prompt_step(st, arg, ids, lens, None, 6, 2, S_before, submit, handout, retire, P.HOOK_L, ptok, plen, req, mut)
            cache = np.zeros((2, 2, R, 2, 12, 64), dtype=np.int32)
            ring = np.arange(2 * 2 * 3 * 2 * 6 * 64, dtype=np.int32).reshape(2, 2, 3, 2, 6, 64) + 1
            P.prompt_refill(cache, ring, a + b, mut)
            out.append((name, R, {k: v.tolist() for k, v in st.items()}, ids.tolist(), lens.tolist(), cache.tobytes()))
    return out


def _schedule_outputs(mut):
    subs = _schedule()
    return [P.play(subs, 4, 3, 2, L, MP, mut, natural={2: 6}), P.play(subs, 3, 4, 1, L, MP, mut, natural={1: 6}),
            P.play(subs, 2, 8, 1, L, MP, mut, cancel=(6,))]


@pytest.mark.parametrize("mut", P.MUTATIONS)
def test_mutations_are_rejected(mut):
    """Every wrong rule changes what the kernel test compares (state, id ring, length words, cache bytes) on its own cases; all but
    the one that only shows in the cache bytes also change what a session delivers."""
    hook = _hook_outputs(mut) != _hook_outputs(None)
    sched = _schedule_outputs(mut) != _schedule_outputs(None)
    assert hook, mut
    if mut != "copy_P_slots":         # (the step that follows overwrites slot P: only the byte comparison of the kernel test sees it)
        assert sched, mut


def test_the_issue_names_these_mutations():
    assert {"seat_step_P", "position_zero", "ring_row_q", "no_wrap", "copy_P_slots", "limit_generated_only"} <= set(P.MUTATIONS)


def test_oracle_greedy_on_a_tiny_case():
    """The oracle loop against tests/prompt_reference.py's greedy_search with a mask of ones (equal prompt lengths), and its ragged
    form against the rows run alone."""
    import torch

    import prompt_reference as pr
    from conftest import synth_sd
    sd = synth_sd("ragged")
    g = torch.Generator().manual_seed(97)
    prompts = [torch.randint(0, 50000, (p,), generator=g) for p in (3, 3, 1)]
    feats = torch.randn((3, 1024), generator=g)
    got, gap = P.oracle_greedy(sd, prompts, feats, 6)
    ref = pr.greedy_search(sd, torch.stack(prompts[:2]), feats[:2], 6, torch.ones((2, 3), dtype=torch.int64))
    for s in range(2):
        row = ref[s].tolist()
        end = next((j + 1 for j in range(3, len(row)) if row[j] == EOS), len(row))
        assert got[s].tolist() == row[:end]
    alone, gap1 = P.oracle_greedy(sd, prompts[2:], feats[2:], 6)
    assert got[2].tolist() == alone[0].tolist() and got[2][0] == prompts[2][0] and 0 < gap <= gap1
