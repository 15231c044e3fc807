"""CPU checks of tests/kv8_reference.py: the e4m3 conversion's known answers, the oracle patch, and the POWER of the per-kernel
comparison of tests/test_gpu_kv8_kernel.py - on that test's shapes, attn_reference.compare() with the bound derived from the
reference alone rejects an evaluation that leaves the new token's k / v unrounded, one that rounds them through bf16 first, and
the applicable mutations of attn_reference.MUTATIONS, in every output type."""
import pytest
import torch

import attn_reference as R
import kv8_reference as K8
from conftest import synth_sd
from oracle import language_model as o_lm

F64, F32 = torch.float64, torch.float32


def test_rnd8_known_answers():
    x = torch.tensor([1.0625, 1.1875, 17.0, 19.0, 448.0, 449.0, 1e9, -500.0, 464.0, 480.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9,
                      2.0 ** -10 * 1.001, 0.0, 272.5])
    want = torch.tensor([1.0, 1.25, 16.0, 20.0, 448.0, 448.0, 448.0, -448.0, 448.0, 448.0, 2.0 ** -9, 0.0, 2.0 ** -8, 2.0 ** -9, 0.0, 288.0])
    assert torch.equal(K8.rnd8(x), want)
    assert torch.isfinite(K8.rnd8(torch.tensor([3.0e38, -3.0e38]))).all()
    z = K8.rnd8(torch.tensor([-0.0, -(2.0 ** -11)]))
    assert torch.equal(z, torch.zeros(2)) and torch.signbit(z).all()                      # -0 stays -0, a tiny negative becomes -0
    assert K8.to_bytes(torch.tensor([-0.0, 448.0, -448.0, 2.0 ** -9, 1.0])).tolist() == [0x80, 0x7E, 0xFE, 0x01, 0x38]
    assert K8.rnd8_via16(torch.tensor([272.5]), 0).item() == 256.0                         # the double rounding differs
    b = torch.arange(256, dtype=torch.uint8)
    v = K8.from_bytes(b)
    ok = torch.isfinite(v)
    assert int((~ok).sum()) == 2 and torch.equal(K8.to_bytes(v[ok]), b[ok])               # every finite byte survives the round trip
    assert torch.equal(K8.rnd8(x.double()), want.double())


def test_patched_oracle_is_the_oracle_again_after_the_context():
    sd = synth_sd("bench")
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(2, 1024, generator=g)
    ids = torch.cat((torch.full((2, 1), 50256), torch.randint(0, 50257, (2, 5), generator=g)), dim=1)
    keep = o_lm.pseudo_attention
    a = o_lm.teacher_forced_trace(sd, ids, feats, bf16=True)
    with K8.e4m3_cache_oracle():
        assert o_lm.pseudo_attention is not keep
        b = o_lm.teacher_forced_trace(sd, ids, feats, bf16=True)
    assert o_lm.pseudo_attention is keep
    c = o_lm.teacher_forced_trace(sd, ids, feats, bf16=True)
    for k in a:
        assert torch.equal(a[k], c[k]), k
    assert not torch.equal(a["last_logits"], b["last_logits"])                             # ... and inside it computes something else
    with pytest.raises(RuntimeError):
        with K8.e4m3_cache_oracle():
            raise RuntimeError("x")
    assert o_lm.pseudo_attention is keep


def _case(nkeys, S, with_src, target, seed=21):
    d = K8.decode_inputs_kv8(S, 16, nkeys, nkeys + 2, seed, with_src, "half", K8.KV8_STEP, desig_all=target)
    Kc, Vc = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])
    return d, (lambda dt, o16, **kw: K8.decode_forward_kv8(d["q"], d["kn"], d["vn"], Kc, Vc, d["step"], d["src"], dt, out16=o16, **kw)[0])


POWER_NKEYS = (2, 17, 65, 129, 145, 146, 177, 225, 273, 289)
OUT_TYPES = (None, 0, 1)


@pytest.mark.parametrize("nkeys", POWER_NKEYS)
@pytest.mark.parametrize("new_kv", ("raw", "via_bf16"))
def test_compare_rejects_a_wrong_rounding_of_the_new_token(nkeys, new_kv):
    """The designated key is the new token's: half of the softmax sits on the key and the value whose rounding is wrong."""
    for with_src in (False, True):
        d, f = _case(nkeys, 5, with_src, nkeys - 1)
        for o16 in OUT_TYPES:
            r64, r32 = f(F64, o16), f(F32, o16)
            assert R.compare(r32, r64, r32, o16)["ok"]
            bad = R.compare(f(F64, o16, new_kv=new_kv), r64, r32, o16)
            assert not bad["ok"], (nkeys, new_kv, with_src, o16, bad)


def _target(mut, nkeys):
    tile = K8.KV8_CHUNK
    if mut == "drop_last_key":
        return nkeys - 1
    if mut == "drop_first_of_last_chunk":
        return ((nkeys - 1) // tile) * tile
    if nkeys < 4:
        return 0                         # two keys: the only cached key is the image key (of the ancestor's row, with a table)
    return max(1, min(nkeys - 3, 77))   # a cached key with a cached neighbour


def _mutation_cases():
    """Every mutation on every key count where it can act.  read_next_slot at two keys is left out: the only cached key is the
    image key and its next slot is the new token's own, which the kernel test fills with NaN.  With half of the softmax on ONE key
    the other scores of a short row are nearly equal, so the score scale shows in every output type only from 65 keys on;
    test_compare_rejects_a_wrong_score_scale_on_plain_scores covers every key count on the plain variant of the kernel test."""
    for mut in ("drop_last_key", "drop_first_of_last_chunk", "read_next_slot", "ignore_ancestor", "scale_sqrt65"):
        for nkeys in POWER_NKEYS:
            if nkeys < 4 and mut == "read_next_slot":
                continue
            if nkeys < 65 and mut == "scale_sqrt65":
                continue
            yield mut, nkeys


@pytest.mark.parametrize("nkeys", POWER_NKEYS)
def test_compare_rejects_a_wrong_score_scale_on_plain_scores(nkeys):
    """The inputs of the kernel test's plain variant themselves (fp32 output): unequal scores, so 1 / sqrt(65) in place of 1 / 8
    moves the softmax at every key count, two keys included."""
    d = K8.kv8_case(nkeys, K8.KV8_PLAIN)
    Kc, Vc = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])
    f = lambda dt, **kw: K8.decode_forward_kv8(d["q"], d["kn"], d["vn"], Kc, Vc, d["step"], d["src"], dt, **kw)[0]  # noqa: E731
    r64, r32 = f(F64), f(F32)
    assert R.compare(r32, r64, r32)["ok"]
    bad = R.compare(f(F64, mut="scale_sqrt65"), r64, r32)
    assert not bad["ok"], (nkeys, bad)


@pytest.mark.parametrize("mut,nkeys", list(_mutation_cases()))
def test_compare_rejects_the_mutations(nkeys, mut):
    target = _target(mut, nkeys)
    d, f = _case(nkeys, 6, mut == "ignore_ancestor", target)
    for o16 in OUT_TYPES:
        r64, r32 = f(F64, o16), f(F32, o16)
        assert R.compare(r32, r64, r32, o16)["ok"]
        bad = R.compare(f(F64, o16, mut=mut, mut_col=target), r64, r32, o16)
        assert not bad["ok"], (nkeys, mut, o16, bad)
