"""The kernels of the detector under torch.autocast ALONE against the float64 reference of tests/det16_reference.py:
  a. rgrg_conv2d_nhwc_bf16 (the CONV instantiations of gemm_bf16_glds_kernel) on every one of the 12 (tile, stages) configurations,
     forced through rgrg_debug_conv2d_nhwc_bf16_tile, on small maps: ragged row tiles that straddle images, a non-square map,
     3 x 3 / 1 x 1 with stride 1 / 2, Cin 64 / 128 / 192, Cout 64 / 160 / 192, K shorter than the pipeline, residual, both activations;
  b. the detector's own 54 convolutions on the teacher-forced inputs of one image, each on every tile the launcher's heuristic
     (rgrg_debug_bf16_tile_choice) picks for it at batch 1 .. 32, and the plain entry bit for bit against the hook on the batch-1 tile;
  c. rgrg_roi_align_avgpool_bf16maps on the inputs of the three fp32 RoIAlign tests of test_gpu_kernels.py;
  d. rgrg_linear_bf16_f32 at fc6's K = 131072 on the heuristic's tile, on the 128 x 128 tile and on the 256 x 256 kernel;
  e. engine.backbone16 + engine.rpn free-running on two images against the float64 chain.
Both 16-bit types.  fp32 outputs: attn_reference.compare, MARGIN * max|ref32 - ref64| + 2^-23 max|ref|; 16-bit outputs:
train_rows_reference.compare16, per element MARGIN * noise + half an ulp of the type at the element.  The noise is the reference's own
float32 evaluation against its float64 one; no bound comes from the code under test.  (e) has no per-element bound - two correct
16-bit chains decorrelate to quantisation noise: RMS and 99.9th percentile of the difference may reach twice the largest such
statistic among the reference's own chains (float64, float32, float32 in two other summation orders).  (d): the float32 evaluation
adds 16 k values per step to one fp32 accumulator, the matrix core's order (det16_reference.linear16 says why); against a blocked
BLAS sum (noise 7.2e-7, bound 6.1e-6 on outputs of size 3.4) the kernels measure 1.4e-5 and would fail.  Behind every output a
sentinel row must stay untouched.  Each figure is printed before it is asserted (lines starting with DET16); the worst ones observed on
the MI355X are kept in profiles/det16_parity.md.
"""
import itertools

import pytest
import torch

import det16_reference as R
from conftest import gpu_model, synth_sd
from rgrg_amd import _hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
RGRG_EINVAL = -1
SENT, SENT16 = -777.25, 0x7B7B
TYPES = pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])


@pytest.fixture(scope="module")
def eng():
    return gpu_model("bench").engine()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _tile_name(tile):
    return "auto" if tile is None else "%dx%dx%d" % (R.TILE_SHAPES[tile & 15] + (tile >> 4,))


def _report(part, case, fp16, tile, res):
    for name, r in res.items():
        print(f"DET16 part={part} case={case} type={'fp16' if fp16 else 'bf16'} tile={tile} out={name} err={r['err']:.3e} noise={r['noise']:.3e} "
              f"bound={r['bound']:.3e} used={r['used']:.3f}")
    for name, r in res.items():
        assert r["ok"], f"{part} {case} {tile} {name}: err {r['err']:.3e} exceeds {r['bound']:.3e} (noise {r['noise']:.3e})"


def _act16(eng, bits):
    """Host int16 bit patterns -> an engine activation buffer (with the zero line the convolution reads in front of it)."""
    t = eng._act16(tuple(bits.shape))
    t.copy_(bits.to(DEV))
    return t


class _Conv:
    """One convolution's operands on the device; launch(tile, out_f32) -> the output [B, Cout, OH, OW] as fp32 values (host)."""

    def __init__(self, eng, c):
        fp16 = c["fp16"]
        self.eng, self.c, self.fp16 = eng, c, fp16
        self.x = _act16(eng, R.nhwc_bits(c["x16"], fp16))
        self.w = R.weight_bits(R.conv16_weights(c["w"], c["scale"], fp16), fp16).to(DEV)
        self.shift = None if c["shift"] is None else c["shift"].to(DEV)
        self.r = None if c["r16"] is None else _act16(eng, R.nhwc_bits(c["r16"], fp16))

    def launch(self, tile, out_f32):
        c, lib = self.c, self.eng.lib
        n = c["B"] * c["OH"] * c["OW"] * c["Cout"]
        y = torch.full((n + c["Cout"],), SENT, dtype=F32, device=DEV) if out_f32 else torch.full((n + c["Cout"],), SENT16, dtype=torch.int16, device=DEV)
        args = (_hip.ptr(self.x), _hip.ptr(self.w), _hip.ptr(self.shift), _hip.ptr(self.r), _hip.ptr(y) if out_f32 else None,
                None if out_f32 else _hip.ptr(y), c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["k"], c["stride"], c["pad"], c["act"],
                int(self.fp16))
        if tile is None:
            _hip.check(lib.rgrg_conv2d_nhwc_bf16(*args, _s()), "rgrg_conv2d_nhwc_bf16")
        else:
            _hip.check(lib.rgrg_debug_conv2d_nhwc_bf16_tile(*args, tile, _s()), "rgrg_debug_conv2d_nhwc_bf16_tile")
        torch.cuda.synchronize()
        assert bool((y[n:] == (SENT if out_f32 else SENT16)).all()), f"{c['name']} tile {tile}: the row behind the output was written"
        return y[:n].view(c["B"], c["OH"], c["OW"], c["Cout"])

    def values(self, y):
        return y.cpu().permute(0, 3, 1, 2) if y.dtype == F32 else R.nchw_values(y.cpu(), self.fp16)


# ------------------------------------------------------------------------------------------------ a. forced tiles, small maps
@TYPES
@pytest.mark.parametrize("i", range(len(R.SMALL_GEOMS)), ids=[R.geom_name(g) for g in R.SMALL_GEOMS])
def test_conv_on_every_tile_configuration(eng, i, fp16):
    c = R.small_case(i, fp16)
    r64, r32 = R.case_eval(c, F64), R.case_eval(c, F32)
    conv = _Conv(eng, c)
    for out_f32 in (True, False):
        for tile in R.TILES:
            got = conv.values(conv.launch(tile, out_f32))
            _report("a", c["name"], fp16, _tile_name(tile), {"y32" if out_f32 else "y16": R.judge(got, r64, r32, fp16, out_f32)})


def test_conv_tile_hook_refuses_the_other_kernel_families(eng):
    c = R.small_case(4, False)
    conv = _Conv(eng, c)
    for tile in (5, 6, 11, 12, 13, 5 + 16 * 2, 1 + 16 * 5, 2 + 16 * 1, -1):
        y = torch.full((c["B"] * c["OH"] * c["OW"] * c["Cout"],), SENT, dtype=F32, device=DEV)
        rc = eng.lib.rgrg_debug_conv2d_nhwc_bf16_tile(_hip.ptr(conv.x), _hip.ptr(conv.w), _hip.ptr(conv.shift), _hip.ptr(conv.r), _hip.ptr(y), None,
                                                      c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["k"], c["stride"], c["pad"], c["act"], 0,
                                                      tile, _s())
        torch.cuda.synchronize()
        assert rc == RGRG_EINVAL and bool((y == SENT).all()), tile


# ------------------------------------------------------------------------------------------------ b. the detector's own convolutions
@TYPES
def test_detector_convolutions_on_the_tiles_of_batch_1_to_32(eng, fp16):
    """Each of the 54 convolutions, stored as the detector stores it (16 bit; rpn_head fp32), on every tile the heuristic picks for its
    geometry at batch 1, 2, 4, 8, 16, 32 - forced on the batch-1 input (the tile code depends on the batch through image straddling
    only, which part a covers).  An output that repeats the bits of one already judged is not judged again."""
    q = eng.lib.rgrg_debug_bf16_tile_choice
    n, used_tiles = 0, set()
    for rec in R.trunk16_walk(synth_sd("bench"), synth.make_images(1, 1234), fp16):
        conv = _Conv(eng, rec)
        M, N, K = rec["OH"] * rec["OW"], rec["Cout"], rec["k"] * rec["k"] * rec["Cin"]
        t1 = q(M, N, K)
        tiles = sorted({q(b * M, N, K) for b in (1, 2, 4, 8, 16, 32)})
        assert t1 in tiles and set(tiles) <= set(R.TILES), (rec["name"], tiles)
        plain = conv.launch(None, rec["out_f32"])
        judged = []
        for tile in tiles:
            y = conv.launch(tile, rec["out_f32"])
            if tile == t1:
                assert torch.equal(y, plain), f"{rec['name']}: the plain entry differs from the hook on the tile the query names ({_tile_name(t1)})"
            res = next((r for yy, r in judged if torch.equal(yy, y)), None)
            if res is None:
                res = R.judge(conv.values(y), rec["v64"], rec["v32"], fp16, rec["out_f32"])
                judged.append((y, res))
            _report("b", rec["name"], fp16, _tile_name(tile), {"y32" if rec["out_f32"] else "y16": res})
        used_tiles.update(tiles)
        n += 1
    assert n == 54 and 1 + 16 * 2 in used_tiles


# ------------------------------------------------------------------------------------------------ c. RoIAlign with 16-bit maps
@pytest.mark.parametrize("name", R.ROI_CASES)
def test_roi_align_16bit_maps(eng, name):
    feat, plist = R.roi_case(name)
    rois = R.rois_of(plist)
    r64, r32 = R.roi_align16(feat, rois, 1.0 / 32, None, F64), R.roi_align16(feat, rois, 1.0 / 32, None, F32)
    B, Cc, FH, FW = feat.shape
    maxp = 1000
    props = torch.zeros((B, maxp, 4))
    offs = [0]
    for b, p in enumerate(plist):
        props[b, :p.shape[0]] = p
        offs.append(offs[-1] + p.shape[0])
    Rt = offs[-1]
    fd, pd, od = feat.permute(0, 2, 3, 1).contiguous().to(DEV), props.to(DEV), torch.tensor(offs, dtype=torch.int32, device=DEV)
    for fp16 in (False, True):
        maps = torch.full((Rt * 64 * Cc + Cc,), SENT16, dtype=torch.int16, device=DEV)
        pooled = torch.full((Rt * Cc + Cc,), SENT, dtype=F32, device=DEV)
        _hip.check(eng.lib.rgrg_roi_align_avgpool_bf16maps(_hip.ptr(fd), _hip.ptr(pd), _hip.ptr(od), _hip.ptr(maps), _hip.ptr(pooled), B, FH, FW, Cc,
                                                           maxp, Rt, 1.0 / 32, int(fp16), _s()), "rgrg_roi_align_avgpool_bf16maps")
        torch.cuda.synchronize()
        assert bool((maps[Rt * 64 * Cc:] == SENT16).all()) and bool((pooled[Rt * Cc:] == SENT).all())
        got_maps = R.from_bits(maps[:Rt * 64 * Cc].cpu(), fp16).view(Rt, 64, Cc)
        _report("c", name, fp16, "-", R.judge_roi(got_maps, pooled[:Rt * Cc].cpu().view(Rt, Cc), r64, r32, fp16))


# ------------------------------------------------------------------------------------------------ d. fc6's K
@TYPES
def test_linear_at_the_k_of_fc6(eng, fp16):
    c = R.fc6_case(fp16)
    lib, N, K = eng.lib, R.FC6_N, R.FC6_K
    a = R.to_bits(c["a16"], fp16).to(DEV)
    w = R.to_bits(c["w16"], fp16).to(DEV)
    shift = c["shift"].to(DEV)
    for what, M, tile in (("heuristic", 130, None), ("128x128", 130, 1), ("256x256", 300, 5)):
        y = torch.full((M * N + N,), SENT, dtype=F32, device=DEV)
        if tile is None:
            assert lib.rgrg_debug_bf16_tile_choice(M, N, K) == 2 + 16 * 4
            _hip.check(lib.rgrg_linear_bf16_f32(_hip.ptr(a), _hip.ptr(w), _hip.ptr(shift), None, _hip.ptr(y), None, M, N, K, N, c["act"], int(fp16), _s()),
                       "rgrg_linear_bf16_f32")
        else:
            _hip.check(lib.rgrg_debug_linear_bf16_tile(_hip.ptr(a), _hip.ptr(w), _hip.ptr(shift), None, _hip.ptr(y), M, N, K, N, c["act"], tile, 0, 0,
                                                       int(fp16), _s()), "rgrg_debug_linear_bf16_tile")
        torch.cuda.synchronize()
        assert bool((y[M * N:] == SENT).all())
        _report("d", f"M={M},N={N},K={K}", fp16, what, {"y32": R.compare(y[:M * N].cpu().view(M, N), R.fc6_eval(fp16, M, F64), R.fc6_eval(fp16, M, F32))})


# ------------------------------------------------------------------------------------------------ e. free-running
FREE_FACTOR = 2.0     # a correct chain is one more draw from the distribution the floor is taken from (module docstring)


@TYPES
def test_free_running_trunk_and_rpn_head_against_the_float64_chain(eng, fp16):
    sd = synth_sd("bench")
    images = synth.make_images(2, 1234)
    chains = [R.trunk16_free(sd, images, fp16, F64), R.trunk16_free(sd, images, fp16, F32), R.trunk16_free(sd, images, fp16, F32, perm=1),
              R.trunk16_free(sd, images, fp16, F32, perm=2)]
    x16, feat = eng.backbone16(images.to(DEV), int(fp16))
    head = eng.rpn(feat, return_head=True, feat16=x16, f16=int(fp16))[3]
    torch.cuda.synchronize()
    assert torch.equal(R.from_bits(x16.cpu(), fp16), feat.cpu())           # the fp32 map is the 16-bit one widened
    got = (feat.cpu().permute(0, 3, 1, 2), head.cpu().permute(0, 3, 1, 2))
    bad = []
    for j, what in enumerate(("features", "rpn_head")):
        assert got[j].shape == chains[0][j].shape and got[j].numel() >= 100000 and bool(torch.isfinite(got[j]).all())
        pairs = [R.spread(a[j], b[j]) for a, b in itertools.combinations(chains, 2)]
        hip = R.spread(got[j], chains[0][j])
        for stat in ("rms", "p999"):
            floor = max(p[stat] for p in pairs)
            print(f"DET16 part=e case={what} type={'fp16' if fp16 else 'bf16'} stat={stat} hip={hip[stat]:.4e} floor={floor:.4e} "
                  f"pairs={' '.join('%.3e' % p[stat] for p in pairs)} used={hip[stat] / (FREE_FACTOR * floor):.3f} max={float(chains[0][j].abs().max()):.3e}")
            if not hip[stat] <= FREE_FACTOR * floor:
                bad.append((what, stat, hip[stat], floor))
    assert not bad, bad
