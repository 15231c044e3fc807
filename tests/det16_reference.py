"""Plain torch restatements of the kernels the detector runs under torch.autocast (engine.backbone16 / rpn / roi_heads): the
implicit-GEMM convolution rgrg_conv2d_nhwc_bf16 (the CONV instantiations of gemm_bf16_glds_kernel), the 16-bit RoIAlign
rgrg_roi_align_avgpool_bf16maps and fc6 on rgrg_linear_bf16_f32, the inputs the per-kernel tests share and the mutations the
GPU-less test must see rejected.  TEST INFRASTRUCTURE ONLY.  Number formats and the bounds come from attn_reference
(compare, MARGIN) and train_rows_reference (compare16).

Every evaluation takes ``dt``: torch.float64 for the reference, torch.float32 for the noise measurement, and ``mut``: one named
mutation, each as a kernel would get it wrong (tests/test_det16_reference.py: every one must be rejected on the inputs the GPU
test uses).  Tensors are NCHW on the host; nhwc_bits() gives what the kernels read.

What is evaluated:
  conv16      act(conv(x16, round16(fl32(w * bn_scale))) + shift + r16): the 16-bit operands convolved in dt, the fp32 shift and the
              16-bit residual added, the activation; returned unrounded.  stored() is what a kernel keeps of it: fp32, or one
              rounding to the 16-bit type.
  trunk16_walk  the 52 trunk convolutions, rpn_conv and rpn_head of one image, TEACHER-FORCED: the input and the residual of every
              layer are the stored 16-bit outputs of the float64 chain, so a layer's two evaluations differ by that layer's
              float32 noise alone.
  trunk16_free  the same chain free-running in dt (the stem too); ``perm`` permutes the input channels of every convolution in x
              and w alike - the same mathematics in another float32 summation order.
  roi_align16 tv013.roi_align in dt: the 8 x 8 bins (stored as 16-bit values) and their average, taken from the UNROUNDED bins.
  linear16    act(a16 w16^T + shift): float64 over K chunks (a float64 copy of the weights stays small); float32 in the matrix core's
              order, one accumulator taking 16 k values per step (linear16 says why).
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Iterator, List, Optional, Tuple

import torch
import torch.nn.functional as F

from attn_reference import MARGIN, compare, from_bits, rnd16, to_bits  # noqa: F401  (re-exported for the tests)
from oracle import tv013
from train_rows_reference import compare16

Tensor = torch.Tensor
F64, F32 = torch.float64, torch.float32
ACT_NONE, ACT_RELU = 0, 1
BN_EPS = 1e-5
ROW_TILE = 64        # the smallest row tile of the LDS-DMA kernel: what the tile-level mutations assume

MUTATIONS = ("pad_tap_reads_neighbour", "kh_kw_swapped", "h_w_swapped_in_offset", "straddle_reads_next_image",
             "residual_off_by_one_tile", "bn_scale_after_rounding", "last_k_tile_dropped", "stride_offset_plus_1",
             "roi_average_from_rounded")


# ------------------------------------------------------------------------------------------------ layouts
def nhwc_bits(x: Tensor, fp16) -> Tensor:
    """NCHW values that are exactly representable -> the NHWC int16 bit patterns the kernels read."""
    return to_bits(x.permute(0, 2, 3, 1).contiguous(), fp16)


def nchw_values(bits_nhwc: Tensor, fp16) -> Tensor:
    """NHWC int16 bit patterns -> NCHW fp32 values."""
    return from_bits(bits_nhwc, fp16).permute(0, 3, 1, 2)


def weight_bits(w16: Tensor, fp16) -> Tensor:
    """[Cout][Cin][KH][KW] 16-bit values -> [Cout][KH][KW][Cin] bit patterns (engine._Conv's layout)."""
    return to_bits(w16.permute(0, 2, 3, 1).contiguous(), fp16)


def out_size(n: int, k: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - k) // stride + 1


# ------------------------------------------------------------------------------------------------ the convolution
def conv16_weights(w: Tensor, scale: Optional[Tensor], fp16, mut: Optional[str] = None) -> Tensor:
    """round16(fl32(w * scale)) as engine._conv16_weights makes them (fp32 values of the 16-bit weights; fp16 None = unrounded)."""
    if scale is None:
        return w if fp16 is None else rnd16(w, fp16)
    if fp16 is None:
        return w * scale.view(-1, 1, 1, 1)
    if mut == "bn_scale_after_rounding":
        return None     # conv16 applies the scale in dt
    return rnd16(w * scale.view(-1, 1, 1, 1), fp16)


def bn_affine(sd: Dict[str, Tensor], p: str) -> Tuple[Tensor, Tensor]:
    """engine._bn_affine: alpha = w / sqrt(var + eps), beta = b - mean * alpha, in fp32."""
    invstd = 1.0 / torch.sqrt(sd[p + "running_var"] + BN_EPS)
    alpha = sd[p + "weight"] * invstd
    return alpha.contiguous(), (sd[p + "bias"] - sd[p + "running_mean"] * alpha).contiguous()


def _straddling_rows(B: int, OH: int, OW: int) -> Tensor:
    """Mask [B, OH, OW] of the output pixels whose row tile (ROW_TILE flattened pixels) holds pixels of two images."""
    m = torch.arange(B * OH * OW)
    first, last = (m // ROW_TILE) * ROW_TILE, torch.clamp((m // ROW_TILE) * ROW_TILE + ROW_TILE - 1, max=B * OH * OW - 1)
    return (first // (OH * OW) != last // (OH * OW)).reshape(B, OH, OW)


def conv16(x16: Tensor, w: Tensor, scale: Optional[Tensor], shift: Optional[Tensor], r16: Optional[Tensor], stride: int, pad: int,
           act: int, fp16, dt, mut: Optional[str] = None, perm: Optional[Tensor] = None) -> Tensor:
    """x16 [B, Cin, H, W] and r16 [B, Cout, OH, OW]: fp32 values of 16-bit numbers; w [Cout, Cin, KH, KW], scale / shift [Cout] fp32.
    Returns the UNROUNDED result [B, Cout, OH, OW] in dt.  fp16 None: nothing is rounded (the chain against tv013)."""
    B, Cin, H, W = x16.shape
    Cout, _, KH, KW = w.shape
    OH, OW = out_size(H, KH, stride, pad), out_size(W, KW, stride, pad)
    w16 = conv16_weights(w, scale, fp16, mut)
    if w16 is None:
        wd = rnd16(w, fp16).to(dt) * scale.to(dt).view(-1, 1, 1, 1)
    else:
        wd = w16.to(dt)
    if mut == "kh_kw_swapped":
        wd = wd.transpose(2, 3)
    if mut == "last_k_tile_dropped":        # K runs [kh][kw][cin]: the last 64 channels of the last tap
        wd = wd.clone()
        wd[:, Cin - 64:, KH - 1, KW - 1] = 0.0
    xd = x16.to(dt)
    if perm is not None:
        xd, wd = xd[:, perm], wd[:, perm]

    def run(xp: Tensor) -> Tensor:   # xp carries its padding
        return F.conv2d(xp, wd, stride=stride)[:, :, :OH, :OW]

    if mut == "h_w_swapped_in_offset":      # the tap (iy, ix) is read at pixel offset iy * H + ix of the flattened batch
        flat = torch.cat((xd.permute(1, 0, 2, 3).reshape(Cin, -1), torch.zeros(Cin, H * H + W, dtype=dt)), 1)
        iy, ix = torch.arange(H)[:, None], torch.arange(W)[None, :]
        idx = (torch.arange(B)[:, None, None] * H * W + (iy * H + ix)[None]).reshape(-1)
        xd = flat[:, idx].reshape(Cin, B, H, W).permute(1, 0, 2, 3)
    xp = F.pad(xd, (pad, pad, pad, pad))
    if mut == "pad_tap_reads_neighbour" and pad:   # a tap left of column 0 reads the previous row's last pixels, one right of
        xp = xp.clone()                            # column W - 1 the next row's first ones (the unchecked offset iy * W + ix)
        xp[:, :, pad + 1:pad + H, :pad] = xd[:, :, :H - 1, W - pad:]
        xp[:, :, pad:pad + H - 1, W + pad:] = xd[:, :, 1:, :pad]
    if mut == "stride_offset_plus_1":              # iy = oy * stride - pad + 1 + kh
        xp = F.pad(xp, (0, 0, 0, 1))[:, :, 1:]
    v = run(xp)
    if mut == "straddle_reads_next_image" and pad and B > 1:
        tall = F.pad(xd.permute(1, 0, 2, 3).reshape(1, Cin, B * H, W), (pad, pad, pad, pad))   # the images one below the other
        nb = torch.cat([tall[:, :, b * H:b * H + H + 2 * pad] for b in range(B)], 0)
        v = torch.where(_straddling_rows(B, OH, OW)[:, None], run(nb), v)
    if shift is not None:
        v = v + shift.to(dt).view(1, -1, 1, 1)
    if r16 is not None:
        r = r16
        if mut == "residual_off_by_one_tile" and B * OH * OW > ROW_TILE:   # the second row tile reads the first one's residual
            rows = r16.permute(0, 2, 3, 1).reshape(B * OH * OW, Cout).clone()
            n = min(B * OH * OW, 2 * ROW_TILE) - ROW_TILE
            rows[ROW_TILE:ROW_TILE + n] = rows[:n]
            r = rows.reshape(B, OH, OW, Cout).permute(0, 3, 1, 2)
        v = v + r.to(dt)
    return torch.clamp(v, min=0.0) if act == ACT_RELU else v


def stored(v: Tensor, fp16, out_f32: bool) -> Tensor:
    """What a kernel that computed v keeps: the fp32 value, or one rounding to the 16-bit type (as fp32 values)."""
    return v.float() if out_f32 or fp16 is None else rnd16(v.float(), fp16)


def judge(got: Tensor, r64: Tensor, r32: Tensor, fp16, out_f32: bool) -> Dict[str, float]:
    """One output against its bound: attn_reference.compare (fp32) or train_rows_reference.compare16 (16-bit values)."""
    return compare(got, r64, r32) if out_f32 else compare16(got, r64, r32, fp16)


def conv_applies(mut: str, g: dict) -> bool:
    """Whether a mutation changes anything in a convolution case."""
    B, H, W, k, s, p = g["B"], g["H"], g["W"], g["k"], g["stride"], g["pad"]
    M = B * out_size(H, k, s, p) * out_size(W, k, s, p)
    return {"pad_tap_reads_neighbour": p > 0, "kh_kw_swapped": k > 1, "h_w_swapped_in_offset": H != W,
            "straddle_reads_next_image": p > 0 and B > 1 and bool(_straddling_rows(B, out_size(H, k, s, p), out_size(W, k, s, p)).any()),
            "residual_off_by_one_tile": g["res"] and M > ROW_TILE, "bn_scale_after_rounding": g.get("scale", True) is not None,
            "last_k_tile_dropped": True, "stride_offset_plus_1": True, "roi_average_from_rounded": False}[mut]


# ------------------------------------------------------------------------------------------------ forced-tile cases (small maps)
TILE_SHAPES = {1: (128, 128), 2: (64, 64), 3: (128, 64), 4: (64, 128)}
TILES = tuple(shape + 16 * nst for shape in (1, 2, 3, 4) for nst in (2, 3, 4))     # the 12 CONV configurations

# B, H, W, Cin, Cout, k, stride, pad, residual, act
SMALL_GEOMS = (
    dict(B=4, H=9, W=9, Cin=128, Cout=160, k=3, stride=1, pad=1, res=True, act=ACT_RELU),     # M = 324: ragged row tile, tiles straddle images
    dict(B=2, H=7, W=12, Cin=192, Cout=192, k=3, stride=1, pad=1, res=False, act=ACT_NONE),   # non-square, the tap changes at K tile 3
    dict(B=2, H=9, W=9, Cin=64, Cout=64, k=3, stride=2, pad=1, res=True, act=ACT_RELU),       # stride 2 on odd H
    dict(B=3, H=8, W=12, Cin=128, Cout=192, k=3, stride=2, pad=1, res=False, act=ACT_RELU),   # stride 2 on even H, non-square
    dict(B=2, H=9, W=9, Cin=64, Cout=160, k=1, stride=1, pad=0, res=True, act=ACT_NONE),      # K = one tile: 2 stages whatever is asked
    dict(B=2, H=9, W=7, Cin=128, Cout=64, k=1, stride=2, pad=0, res=False, act=ACT_RELU),     # 1 x 1 stride 2; K = 2 tiles < 4 - 1
    dict(B=2, H=12, W=7, Cin=192, Cout=160, k=1, stride=1, pad=0, res=True, act=ACT_RELU),    # 1 x 1 with Cin = 192
)


def _gen(*key) -> torch.Generator:
    s = 1469598103
    for k in key:
        s = (s * 1000003 + int(k)) % 2147483647
    return torch.Generator().manual_seed(s)


def geom_name(g: dict) -> str:
    return f"B{g['B']}_{g['H']}x{g['W']}_c{g['Cin']}-{g['Cout']}_k{g['k']}s{g['stride']}p{g['pad']}_r{int(g['res'])}a{g['act']}"


@functools.lru_cache(maxsize=None)
def small_case(i: int, fp16: bool) -> dict:
    """Inputs of SMALL_GEOMS[i]: activations and residual of unit scale rounded to the type, He-scaled weights, a BatchNorm scale in
    [0.5, 1.5) and a shift of unit scale."""
    g = dict(SMALL_GEOMS[i])
    gen = _gen(17, i, int(fp16))
    B, H, W, Cin, Cout, k = g["B"], g["H"], g["W"], g["Cin"], g["Cout"], g["k"]
    OH, OW = out_size(H, k, g["stride"], g["pad"]), out_size(W, k, g["stride"], g["pad"])
    g.update(name=geom_name(g), fp16=fp16, OH=OH, OW=OW, x16=rnd16(torch.randn(B, Cin, H, W, generator=gen), fp16),
             w=torch.randn(Cout, Cin, k, k, generator=gen) / math.sqrt(Cin * k * k), scale=torch.rand(Cout, generator=gen) + 0.5,
             shift=torch.randn(Cout, generator=gen),
             r16=rnd16(torch.randn(B, Cout, OH, OW, generator=gen), fp16) if g["res"] else None)
    return g


def case_eval(c: dict, dt, mut: Optional[str] = None) -> Tensor:
    return conv16(c["x16"], c["w"], c["scale"], c["shift"], c["r16"], c["stride"], c["pad"], c["act"], c["fp16"], dt, mut)


# ------------------------------------------------------------------------------------------------ the detector's chain
RESNET50_LAYERS = tv013.RESNET50_LAYERS
BB, RPN = "object_detector.backbone.", "object_detector.rpn.head."


def chain_layers(sd: Dict[str, Tensor]) -> List[dict]:
    """The 54 convolutions in the order engine.backbone16 and engine.rpn launch them: name, weights, fp32 scale / shift, stride, pad,
    activation, what it reads ("src": the block input "x" or the previous output "o"), whether the block input is its residual."""
    out = []
    for li, (_planes, blocks, stride) in enumerate(RESNET50_LAYERS):
        for b in range(blocks):
            p = f"{BB}{4 + li}.{b}."
            s = stride if b == 0 else 1
            has_ds = (p + "downsample.0.weight") in sd
            out.append(dict(name=f"l{li + 1}.{b}.c1", w=sd[p + "conv1.weight"], bn=p + "bn1.", stride=1, pad=0, act=ACT_RELU, src="x"))
            out.append(dict(name=f"l{li + 1}.{b}.c2", w=sd[p + "conv2.weight"], bn=p + "bn2.", stride=s, pad=1, act=ACT_RELU, src="o"))
            if has_ds:
                out.append(dict(name=f"l{li + 1}.{b}.ds", w=sd[p + "downsample.0.weight"], bn=p + "downsample.1.", stride=s, pad=0,
                                act=ACT_NONE, src="x", role="ds"))
            out.append(dict(name=f"l{li + 1}.{b}.c3", w=sd[p + "conv3.weight"], bn=p + "bn3.", stride=1, pad=0, act=ACT_RELU, src="o",
                            role="c3", res="ds" if has_ds else "x"))
    out.append(dict(name="rpn_conv", w=sd[RPN + "conv.0.0.weight"], bias=sd[RPN + "conv.0.0.bias"], stride=1, pad=1, act=ACT_RELU, src="x"))
    out.append(dict(name="rpn_head", w=torch.cat([sd[RPN + "cls_logits.weight"], sd[RPN + "bbox_pred.weight"]], 0),
                    bias=torch.cat([sd[RPN + "cls_logits.bias"], sd[RPN + "bbox_pred.bias"]], 0), stride=1, pad=0, act=ACT_NONE, src="o",
                    out_f32=True))
    for L in out:
        L["scale"], L["shift"] = bn_affine(sd, L["bn"]) if "bn" in L else (None, L["bias"])
    return out


def chain_mnk(sd: Dict[str, Tensor], B: int, size: int = 128) -> List[Tuple[str, int, int, int]]:
    """(name, M, N, K) of the implicit GEMMs of the chain at batch B; size: the (square) map the first block reads (512 / 4)."""
    x = o = size
    out = []
    for L in chain_layers(sd):
        Cout, Cin, k, _ = L["w"].shape
        ho = out_size(x if L["src"] == "x" else o, k, L["stride"], L["pad"])
        if L.get("role") == "c3":
            x = ho
        elif L.get("role") != "ds":
            o = ho
        out.append((L["name"], B * ho * ho, Cout, k * k * Cin))
    return out


def stem(sd: Dict[str, Tensor], images: Tensor, dt) -> Tensor:
    """7 x 7 stem + eval BatchNorm as the engine applies it (alpha, beta) + ReLU + 3 x 3 max-pool, in dt."""
    alpha, beta = bn_affine(sd, BB + "1.")
    x = F.conv2d(images.to(dt), sd[BB + "0.weight"].to(dt), stride=2, padding=3)
    x = torch.clamp(x * alpha.to(dt).view(1, -1, 1, 1) + beta.to(dt).view(1, -1, 1, 1), min=0.0)
    return F.max_pool2d(x, kernel_size=3, stride=2, padding=1)


def _chain(sd, x0: Tensor, fp16, dt, perm_seed: Optional[int], forced: bool) -> Iterator[dict]:
    """Both chains.  forced: x0 is the stored stem output; every layer is evaluated in float64 AND float32 on the float64 chain's
    stored outputs.  Otherwise free-running in dt."""
    x = o = ds = None
    x = x0
    for L in chain_layers(sd):
        src = x if L["src"] == "x" else o
        res = None
        if L.get("role") == "c3":
            res = ds if L["res"] == "ds" else x
        perm = None
        if perm_seed is not None:
            perm = torch.randperm(src.shape[1], generator=_gen(perm_seed, src.shape[1]))
        out_f32 = bool(L.get("out_f32"))
        args = (L["w"], L["scale"], L["shift"], res, L["stride"], L["pad"], L["act"], fp16)
        v = conv16(src, *args, F64 if forced else dt, perm=perm)
        rec = dict(L, x16=src, r16=res, v64=v, out_f32=out_f32, B=src.shape[0], H=src.shape[2], W=src.shape[3], Cin=src.shape[1],
                   Cout=L["w"].shape[0], k=L["w"].shape[2], OH=v.shape[2], OW=v.shape[3], fp16=fp16)
        if forced:
            rec["v32"] = conv16(src, *args, F32)
        y = stored(v, fp16, out_f32) if forced else (v if out_f32 or fp16 is None else rnd16(v.float(), fp16).to(dt))
        rec["y"] = y
        if L.get("role") == "ds":
            ds = y
        elif L.get("role") == "c3":
            x = y
        elif L["name"] == "rpn_head":
            pass
        else:
            o = y
        yield rec


def trunk16_walk(sd: Dict[str, Tensor], image: Tensor, fp16) -> Iterator[dict]:
    """One record per convolution of the chain on ``image`` [1, 1, H, W], teacher-forced (module docstring): geometry, x16 / r16 (the
    stored outputs of the float64 chain that the layer reads), v64 / v32 (its unrounded output in both evaluations), out_f32."""
    x0 = rnd16(stem(sd, image, F64).float(), fp16)
    return _chain(sd, x0, fp16, F64, None, True)


def trunk16_free(sd: Dict[str, Tensor], images: Tensor, fp16, dt, perm: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The chain free-running in dt -> (final feature map [B, 2048, h, w] as stored, RPN head output [B, 800, h, w]).  ``perm``: the
    seed of the input-channel permutations.  fp16 None: no rounding anywhere."""
    x0 = stem(sd, images, dt)
    if fp16 is not None:
        x0 = rnd16(x0.float(), fp16).to(dt)
    feat = head = None
    for rec in _chain(sd, x0, fp16, dt, perm, False):
        if rec["name"] == "rpn_conv":
            feat = rec["x16"]
        head = rec["y"]
    return feat, head


# ------------------------------------------------------------------------------------------------ RoIAlign
def roi_align16(feat: Tensor, rois: Tensor, spatial_scale: float, fp16, dt, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """feat [B, C, H, W] fp32, rois [K, 5] -> maps [K, 64, C] (bin-major, UNROUNDED; the kernel stores them as 16-bit values) and
    pooled [K, C], the average of the unrounded bins."""
    return roi_outputs(tv013.roi_align(feat.to(dt), rois.to(dt), spatial_scale, 8, 2), fp16, mut)


def roi_outputs(bins: Tensor, fp16, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """bins [K, C, 8, 8] of tv013.roi_align -> maps, pooled (roi_align16) and the bins themselves.  fp16 matters to the mutation only."""
    K, C = bins.shape[:2]
    src = rnd16(bins.float(), fp16).to(bins.dtype) if mut == "roi_average_from_rounded" else bins
    return {"maps": bins.reshape(K, C, 64).permute(0, 2, 1), "pooled": src.reshape(K, C, 64).mean(dim=2), "bins": bins}


def rois_of(plist: List[Tensor]) -> Tensor:
    return torch.cat([torch.cat([torch.full((p.shape[0], 1), float(i)), p], 1) for i, p in enumerate(plist)], 0)


@functools.lru_cache(maxsize=None)
def roi_oracle_case() -> Tuple[Tensor, List[Tensor]]:
    """The inputs of test_gpu_kernels.test_roi_align_on_oracle_features: the CPU oracle's trunk features of two synthetic images and
    the first 200 of its proposals per image."""
    from conftest import synth_sd
    from rgrg_amd import synth
    sd = synth_sd("bench")
    images = torch.cat([synth.make_images(1, 1234), synth.make_images(1, 77)], 0)
    feat = tv013.resnet50_trunk(sd, BB, images)
    obj, reg = tv013.rpn_head(sd, RPN, feat)    # the proposals as oracle.detector makes them, without running its box head
    anchors = tv013.grid_anchors((512, 512), (16, 16))
    objectness = tv013.permute_and_flatten(obj, 1).reshape(2, -1)
    deltas = tv013.permute_and_flatten(reg, 4).reshape(-1, 4)
    proposals = tv013.box_decode(deltas, anchors.repeat(2, 1), (1.0, 1.0, 1.0, 1.0)).view(2, -1, 4)
    return feat, [p[:200] for p in tv013.filter_proposals(proposals, objectness, (512, 512))[0]]


def roi_edge_case() -> Tuple[Tensor, List[Tensor]]:
    """The inputs of test_gpu_kernels.test_roi_align_edge_boxes."""
    g = torch.Generator().manual_seed(5)
    feat = torch.randn((1, 256, 16, 16), generator=g)
    boxes = torch.tensor([[0.0, 0.0, 512.0, 512.0], [500.0, 500.0, 512.0, 512.0], [100.0, 100.0, 100.5, 100.2],
                          [0.0, 0.0, 1e-3, 1e-3], [31.9, 64.0, 480.1, 96.0], [200.0, 0.0, 232.0, 512.0]])
    return feat, [boxes]


ROI_OTHER_MAPS = ((8, 8, 128), (12, 20, 64), (20, 12, 192))


def roi_other_case(FH: int, FW: int, C: int) -> Tuple[Tensor, List[Tensor]]:
    """The inputs of test_gpu_kernels.test_roi_align_other_map_sizes_and_partial_chunks: 33 / 0 / 1 / 31 RoIs on four images."""
    g = torch.Generator().manual_seed(FH * 100 + FW)
    feat = torch.randn((4, C, FH, FW), generator=g)
    W, H = FW * 32.0, FH * 32.0

    def boxes(n):
        xy = torch.rand((n, 2), generator=g) * torch.tensor([W, H]) * 0.9
        wh = torch.rand((n, 2), generator=g) * torch.tensor([W, H]) * 0.6 + 1.0
        b = torch.cat([xy, torch.minimum(xy + wh, torch.tensor([W, H]))], 1)
        b[0] = torch.tensor([0.0, 0.0, W, H])
        if n > 2:
            b[1] = torch.tensor([W - 3.0, H - 3.0, W, H])
            b[2] = torch.tensor([-40.0, -40.0, 20.0, 20.0])
        return b
    return feat, [boxes(33), torch.zeros((0, 4)), boxes(1), boxes(31)]


ROI_CASES = ("oracle0", "oracle1", "edge") + tuple("other%dx%dx%d" % s for s in ROI_OTHER_MAPS)


def roi_case(name: str) -> Tuple[Tensor, List[Tensor]]:
    """(features [B, C, H, W] fp32, boxes per image) of one of ROI_CASES.  oracle0 / oracle1: both feature maps of the oracle case with
    the 200 boxes of one image at a time (the other image has none) - 26 M map elements per case instead of 52 M."""
    if name.startswith("oracle"):
        feat, plist = roi_oracle_case()
        i = int(name[-1])
        return feat, [p if j == i else p[:0] for j, p in enumerate(plist)]
    return roi_edge_case() if name == "edge" else roi_other_case(*ROI_OTHER_MAPS[ROI_CASES.index(name) - 3])


def judge_roi(got_maps: Tensor, got_pooled: Tensor, r64: Dict[str, Tensor], r32: Dict[str, Tensor], fp16) -> Dict[str, Dict]:
    return {"maps": compare16(got_maps, r64["maps"], r32["maps"], fp16), "pooled": compare(got_pooled, r64["pooled"], r32["pooled"])}


# ------------------------------------------------------------------------------------------------ fc6
FC6_K, FC6_N = 131072, 320
MFMA_K = 16          # K elements one v_mfma_f32_32x32x16_bf16 / _f16 adds to its fp32 accumulator
FC6_ROWS = (130, 300)


def linear16(a16: Tensor, w16: Tensor, shift: Optional[Tensor], act: int, dt, mut: Optional[str] = None, chunk: int = 16384) -> Tensor:
    """act(a16 w16^T + shift), [M, K] x [N, K].  float64: accumulated over K chunks.  float32 (the noise run): ONE fp32 accumulator per
    output that takes the K axis 16 elements at a time, one rounding per step - the design of every matrix-core GEMM here (fp32
    accumulate: v_mfma_f32_32x32x16 adds a 16-element dot product to its accumulator, K / 16 times in a row).  The order is restated,
    as skinny_reference.row_stats restates its kernel's, because the noise run has to carry that accepted property: the rounding
    errors of n sequential additions grow like sqrt(n) ulp of the partial sums (n = 8192 at fc6), while a BLAS GEMM blocks its K
    loop and stays near 2 ulp - a noise no single-accumulator kernel can meet at this K, and none should be asked to."""
    M, K = a16.shape
    if mut == "last_k_tile_dropped":
        K -= 64
    v = torch.zeros(M, w16.shape[0], dtype=dt)
    if dt == F32:
        wt = w16.t().contiguous()
        for k0 in range(0, K, MFMA_K):
            v = v + a16[:, k0:k0 + MFMA_K] @ wt[k0:k0 + MFMA_K]
    else:
        for k0 in range(0, K, chunk):
            k1 = min(K, k0 + chunk)
            v += a16[:, k0:k1].to(dt) @ w16[:, k0:k1].to(dt).t()
    if shift is not None:
        v = v + shift.to(dt)
    return torch.clamp(v, min=0.0) if act == ACT_RELU else v


@functools.lru_cache(maxsize=1)      # 0.3 GB per type: one resident at a time
def fc6_case(fp16: bool) -> dict:
    """fc6's K with few columns: activations like RoIAlign maps of a ReLU feature map (non-negative), weights of 1 / sqrt(K) scale.  The
    rows of FC6_ROWS share one activation matrix (the first M rows of it)."""
    gen = _gen(23, int(fp16))
    M = max(FC6_ROWS)
    a = rnd16(torch.randn(M, FC6_K, generator=gen).clamp_(min=0.0), fp16)
    w = rnd16(torch.randn(FC6_N, FC6_K, generator=gen) / math.sqrt(FC6_K), fp16)
    return {"a16": a, "w16": w, "shift": 0.1 * torch.randn(FC6_N, generator=gen), "fp16": fp16, "act": ACT_RELU}


@functools.lru_cache(maxsize=None)
def fc6_eval(fp16: bool, M: int, dt, mut: Optional[str] = None) -> Tensor:
    c = fc6_case(fp16)
    return linear16(c["a16"][:M], c["w16"], c["shift"], c["act"], dt, mut)


# ------------------------------------------------------------------------------------------------ free-running statistics
def spread(a: Tensor, b: Tensor) -> Dict[str, float]:
    """RMS and 99.9th percentile of |a - b| over all elements."""
    d = (a.double() - b.double()).abs().reshape(-1)
    k = max(1, int(math.ceil(0.999 * d.numel())))
    return {"rms": float(torch.sqrt((d * d).mean())), "p999": float(torch.kthvalue(d, k).values)}
