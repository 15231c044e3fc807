"""The float64 attention reference of tests/attn_reference.py and the bounds derived from it, checked without a GPU:
  * its forward equals the repository's oracle (oracle.language_model.pseudo_attention, pinned to the real reference by the
    committed fixtures) on random c_attn outputs - without and with `past`, with a padding mask, with a dropout mask;
  * its backward (autograd, and the closed form the 16-bit kernels are held to) equals finite differences;
  * SENSITIVITY: for every kernel family of tests/test_gpu_attention_kernels.py, each applicable mutation of the reference,
    pushed through the same compare() with the same derived bound, is rejected - the edge-weighted inputs and the bounds can
    see a subtly wrong kernel.
"""
import pytest
import torch

import attn_reference as R
from oracle import language_model as O

F64, F32 = torch.float64, torch.float32


def _sd(g):
    D = O.D_MODEL
    p = "a."
    return {p + "c_attn.weight": torch.randn(D, 3 * D, generator=g) * 0.03, p + "c_attn.bias": torch.randn(3 * D, generator=g) * 0.1,
            p + "c_proj.weight": torch.eye(D), p + "c_proj.bias": torch.zeros(D),
            p + "uk.weight": torch.randn(D, D, generator=g) * 0.03, p + "uk.bias": torch.randn(D, generator=g) * 0.1,
            p + "uv.weight": torch.randn(D, D, generator=g) * 0.03, p + "uv.bias": torch.randn(D, generator=g) * 0.1}


@pytest.mark.parametrize("am_kind,p", [(None, 0.0), ("right", 0.0), ("left", 0.25), ("all", 0.25)])
def test_forward_equals_the_oracle_without_past(am_kind, p):
    g = torch.Generator().manual_seed(3)
    S, T, H = 3, 37, O.N_HEAD
    sd = _sd(g)
    x, img = torch.randn(S, T, O.D_MODEL, generator=g), torch.randn(S, O.D_MODEL, generator=g)
    am = R.make_am(am_kind, S, T, g)
    drop = R.philox_mask(11, 5, p, (S, H, T, T + 1), T + 1) if p > 0 else None
    add = R.pad_add(am, F32) if am is not None else torch.zeros(S, 1, 1, T + 1)
    want, (Ko, Vo) = O.pseudo_attention(sd, "a.", x, img, add, None, drop_probs=drop)
    qkv = O.conv1d(sd, "a.c_attn.", x).view(S, T, 3, H, 64)                      # the oracle's own c_attn output
    ukv = torch.stack((torch.nn.functional.linear(img, sd["a.uk.weight"], sd["a.uk.bias"]),
                       torch.nn.functional.linear(img, sd["a.uv.weight"], sd["a.uv.bias"])), dim=1).view(S, 2, H, 64)
    o64, _, _ = R.tf_forward(qkv, ukv, am, drop, F64)
    o32, _, _ = R.tf_forward(qkv, ukv, am, drop, F32)
    r = R.compare(want.view(S, T, H, 64), o64, o32)
    assert r["ok"], r


@pytest.mark.parametrize("masked", (False, True))
def test_forward_equals_the_oracle_with_past(masked):
    g = torch.Generator().manual_seed(4)
    S, H, nkeys = 3, O.N_HEAD, 41
    sd = _sd(g)
    x = torch.randn(S, 1, O.D_MODEL, generator=g)
    K, V = torch.randn(S, H, nkeys + 2, 64, generator=g), torch.randn(S, H, nkeys + 2, 64, generator=g)
    kmask = None
    add = torch.zeros(S, 1, 1, nkeys)
    if masked:
        kmask = torch.zeros(S, nkeys + 2)
        kmask[:, 1:] = (torch.rand(S, nkeys + 1, generator=g) < 0.3).float() * R.MASK_VALUE
        add = kmask[:, None, None, :nkeys]
    want, _ = O.pseudo_attention(sd, "a.", x, None, add, (K[:, :, :nkeys - 1], V[:, :, :nkeys - 1]))
    q, kn, vn = (t.view(S, H, 64) for t in O.conv1d(sd, "a.c_attn.", x)[:, 0].split(O.D_MODEL, dim=1))
    o64 = R.decode_forward(q, kn, vn, K, V, nkeys - 2, None, kmask, F64)[0]
    o32 = R.decode_forward(q, kn, vn, K, V, nkeys - 2, None, kmask, F32)[0]
    r = R.compare(want.view(S, H, 64), o64, o32)
    assert r["ok"], r


def test_backward_equals_finite_differences():
    """autograd through tf_forward (float64) against torch.autograd.gradcheck's central differences, and the closed form of the
    backward kernels against that autograd - with a padding mask and a dropout mask."""
    S, T, H = 2, 5, 2
    t = R.tf_inputs(S, T, H, 8, "right", None, "half")
    drop = R.philox_mask(3, 1, 0.25, (S, H, T, T + 1), T + 1)
    f = lambda a, b: R.tf_forward(a, b, t["am"], drop, F64)[0]   # noqa: E731
    a, b = t["qkv"].double().requires_grad_(True), t["ukv"].double().requires_grad_(True)
    assert torch.autograd.gradcheck(f, (a, b), eps=1e-6, atol=1e-7, rtol=1e-6)
    o, lse, _ = R.tf_forward(t["qkv"], t["ukv"], t["am"], drop, F64)
    g = R.tf_grads(t["qkv"], t["ukv"], t["am"], drop, t["d_att"], F64)
    m = R.tf_backward_manual(t["qkv"], t["ukv"], t["am"], drop, t["d_att"], o, lse, F64)
    assert (g[0] - m[0]).abs().max() <= 1e-12 * g[0].abs().max() and (g[1] - m[1]).abs().max() <= 1e-12 * g[1].abs().max()


# Which input variant is meant to catch which mutation (all inputs are edge-weighted: one designated key holds half of the
# softmax of every query that sees it, so losing, moving or rescaling THAT key moves the output by O(|V|)):
#   drop_last_key             designated key = the last key (the current token's slot / the last query's own token)
#   drop_first_of_last_chunk  designated key = the first key of the last chunk (decode: 144 / 72 keys) or 32-key tile
#   read_next_slot            designated key: its neighbour's k / v are plain N(0,1) rows
#   ignore_ancestor           designated slot whose ancestor is another row of the beam group (same key, another value row)
#   ignore_mask_one_key       the designated key sits UNDER the padding mask: unmasked it would take half of the softmax
#   skip_causal_one_column    designated key = the last token: every earlier query would see it
#   wrong_dropout_stream      p = 0.25: a quarter of the designated key's half-weights are dropped differently
#   scale_sqrt65              any weighted input: the designated score of ~5 moves by 0.8 %, its weight by ~1 %
#   round_v_again             fp32 families only (a 16-bit V is a fixed point of the rounding): 2^-9 relative on every value
#   omit_ukv_scale            backward families: d_ukv against the reference times 2^15 / 2^-7
def _rejected(pairs):
    """pairs: (got, ref64, ref32, out16) per output of the family; a mutation counts as seen when any output fails its bound."""
    return any(not R.compare(g.float(), r64, r32, o16)["ok"] for g, r64, r32, o16 in pairs)


def _decode_case(kv16, mut):
    nkeys, tile, S, H = 146, (144 if kv16 is None else 72), 6, 16
    target = {"drop_last_key": nkeys - 1, "drop_first_of_last_chunk": ((nkeys - 1) // tile) * tile}.get(mut, 77)
    kmk = None
    d = R.decode_inputs(S, H, nkeys, nkeys + 2, 21, mut == "ignore_ancestor", None, kv16, "half", tile, desig_all=target)
    if mut == "ignore_mask_one_key":
        d["kmask"] = torch.zeros(S, nkeys + 2)
        d["kmask"][:, target] = R.MASK_VALUE
    Kc, Vc = torch.nan_to_num(d["K"]), torch.nan_to_num(d["V"])
    f = lambda dt, m=None: R.decode_forward(d["q"], d["kn"], d["vn"], Kc, Vc, d["step"], d["src"], d["kmask"], dt, kv16=kv16,  # noqa: E731
                                            out16=kv16 is not None, mut=m, mut_col=target, chunk=tile)[0]
    return f(F64), f(F32), f(F64, mut), kv16


DECODE_MUTS = ("drop_last_key", "drop_first_of_last_chunk", "read_next_slot", "ignore_ancestor", "scale_sqrt65")


@pytest.mark.parametrize("mut", DECODE_MUTS + ("ignore_mask_one_key", "round_v_again"))
def test_sensitivity_decode_f32(mut):
    r64, r32, bad, _ = _decode_case(None, mut)
    assert R.compare(r32, r64, r32)["ok"] and _rejected([(bad, r64, r32, None)])


@pytest.mark.parametrize("kv16", (0, 1))
@pytest.mark.parametrize("mut", DECODE_MUTS)
def test_sensitivity_decode_kv16(mut, kv16):
    """The 16-bit OUTPUT (out16) is the coarser of the two: a mutation it rejects is rejected by the fp32 output as well."""
    r64, r32, bad, o16 = _decode_case(kv16, mut)
    assert _rejected([(bad, r64, r32, o16)])


def _tf_case(mut, fmt16, backward):
    S, T, H = 2, 70, 16
    target = {"drop_last_key": T, "drop_first_of_last_chunk": 64, "skip_causal_one_column": T}.get(mut, 40)
    p = 0.25 if mut == "wrong_dropout_stream" else 0.0
    t = R.tf_inputs(S, T, H, 33, None, fmt16, "half", desig_all=target)
    am = None
    if mut == "ignore_mask_one_key":
        am = torch.ones(S, T)
        am[:, target - 1] = 0.0
    drop = R.philox_mask(5, 9, p, (S, H, T, T + 1), T + 1) if p else None
    alt = R.philox_mask(5, 10, p, (S, H, T, T + 1), T + 1) if p else None
    kw = dict(mut=mut, mut_col=target, drop_alt=alt)
    rd = (lambda x: R.rnd16(x, fmt16)) if fmt16 is not None else (lambda x: x)
    fw = {dt: R.tf_forward(t["qkv"], t["ukv"], am, drop, dt, p16=fmt16) for dt in (F64, F32)}
    if not backward:
        bad = R.tf_forward(t["qkv"], t["ukv"], am, drop, F64, p16=fmt16, **kw)
        return [(rd(bad[0]), rd(fw[F64][0]), rd(fw[F32][0]), fmt16), (bad[1], fw[F64][1], fw[F32][1], None)]
    scale = 2.0 ** 15
    att, lse = rd(fw[F64][0]).float(), fw[F64][1].float()
    if fmt16 is None:   # the fp32 kernels: autograd
        ref = {dt: R.tf_grads(t["qkv"], t["ukv"], am, drop, t["d_att"], dt) for dt in (F64, F32)}
        bad = R.tf_grads(t["qkv"], t["ukv"], am, drop, t["d_att"], F64, **kw) if mut != "omit_ukv_scale" else ref[F64]
    else:
        ref = {dt: R.tf_backward_manual(t["qkv"], t["ukv"], am, drop, t["d_att"], att, lse, dt, p16=fmt16) for dt in (F64, F32)}
        bad = R.tf_backward_manual(t["qkv"], t["ukv"], am, drop, t["d_att"], att, lse, F64, p16=fmt16, **kw) if mut != "omit_ukv_scale" else ref[F64]
    bad_scale = 1.0 if mut == "omit_ukv_scale" else scale
    return [(rd(bad[0]), rd(ref[F64][0]), rd(ref[F32][0]), fmt16), (bad[1] * bad_scale, ref[F64][1] * scale, ref[F32][1] * scale, None)]


TF_MUTS = ("drop_last_key", "drop_first_of_last_chunk", "read_next_slot", "ignore_mask_one_key", "skip_causal_one_column",
           "wrong_dropout_stream", "scale_sqrt65")


@pytest.mark.parametrize("mut", TF_MUTS + ("round_v_again",))
def test_sensitivity_prefill(mut):
    assert _rejected(_tf_case(mut, None, False))


@pytest.mark.parametrize("mut", TF_MUTS + ("round_v_again", "omit_ukv_scale"))
def test_sensitivity_backward_f32(mut):
    assert _rejected(_tf_case(mut, None, True))


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("mut", TF_MUTS)
def test_sensitivity_train16_forward(mut, fp16):
    assert _rejected(_tf_case(mut, fp16, False))


@pytest.mark.parametrize("fp16", (0, 1))
@pytest.mark.parametrize("mut", TF_MUTS + ("omit_ukv_scale",))
def test_sensitivity_train16_backward(mut, fp16):
    assert _rejected(_tf_case(mut, fp16, True))


def test_the_unmutated_reference_passes_its_own_bound():
    """The other half of the sensitivity check: compare() accepts the fp32 evaluation of every family (it is the noise)."""
    for fmt16, backward in ((None, False), (None, True), (0, False), (1, True)):
        for got, r64, r32, o16 in _tf_case("none", fmt16, backward):
            assert R.compare(r32, r64, r32, o16)["ok"]
    assert set(DECODE_MUTS + TF_MUTS + ("ignore_mask_one_key", "round_v_again", "omit_ukv_scale")) == set(R.MUTATIONS)
