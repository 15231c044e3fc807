// Device helpers shared by the 16-bit GEMM kernels of gemm_bf16.hip / gemm_kp.inc (gemm_bf16_glds_kernel, gemm_bf16_kp_kernel,
// gemm_bf16_pr_kernel, gemm_bf16_pp_kernel; gemm_bf16w_kernel where the same text stood in it): the tile order, the operand
// offsets and the pieces of the epilogue exist ONCE, here.  A helper takes plain arguments and holds no barrier, wait or pipeline
// step: a kernel keeps its control flow.
//
// The rule: one copy, checked by comparing the gfx950 assembly per kernel with the commit before the change
// (profiles/gemm_shared_epilogue.md holds the commands).  A kernel whose instruction sequence moves is listed there with its
// opcode-count delta and settled on the MI355X: outputs byte-equal through the debug hooks, time inside the parent's own spread.
// A piece goes back to text in a kernel only if that kernel fails the time check.
// hipcc optimises a helper on its own BEFORE it inlines it, so the kernel's passes see other code than they saw with the text in
// place.  What keeps the code closest to the text: no loop over the 16 C-layout registers in a helper that loads or stores (one
// register per call, the kernel keeps its `#pragma unroll` loop), results by value instead of reference parameters, the terms
// of a sum in the order the kernels wrote them (c_row's base).
// Do NOT put __builtin_amdgcn_raw_ptr_buffer_load_lds in here: a function holding it needs one specialization per calling
// kernel (the TAG parameter of glds_issue / pr_dma4 / pp_dma4 / pp_dma2).
#pragma once
#include "internal.h"

namespace rgrg {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr float LN_EPS16 = 1e-5f;   // nn.LayerNorm(eps=1e-5) of GPT-2

// one 32x32x16 matrix-core step on 16-bit fragments of either type (fp32 accumulate)
template <bool F16>
__device__ __forceinline__ f32x16 mfma16(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t bf16_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// gelu_new for a bf16 consumer: x * sigmoid(2 sqrt(2/pi) (x + 0.044715 x^3)) on the hardware exp2 / rcp (~1e-7 relative
// to the tanhf form, far below bf16 resolution).  tanhf costs ~40 VALU instructions; a lane of the 128 x 128 tile has 64
// outputs and the wave is alone on its SIMD: the tanhf epilogue was 8 of the 25 us of c_fc.
__device__ __forceinline__ float gelu_new_fast(float x) {
    const float u = x * (1.0f + 0.044715f * x * x);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.302208198f * u));  // -2 * sqrt(2/pi) * log2(e)
}
// gelu_new'(x) with s = sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3):  tanh u = 2s - 1, so
//   0.5 (1 + tanh u) + 0.5 x (1 - tanh^2 u) u'  =  s + 2 x s (1 - s) sqrt(2/pi) (1 + 3 * 0.044715 x^2)
__device__ __forceinline__ float gelu_new_grad_fast(float x) {
    const float x2 = x * x;
    const float u = x * (1.0f + 0.044715f * x2);
    const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.302208198f * u));
    return sg + 2.0f * x * sg * (1.0f - sg) * 0.7978845608028654f * (1.0f + 0.134145f * x2);
}
__device__ __forceinline__ float apply_act_fast(float v, int act) {
    if (act == RGRG_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == RGRG_ACT_GELU_NEW) return gelu_new_fast(v);
    return v;
}

// The activation of a consumer epilogue.  CACT = RGRG_ACT_NONE / RGRG_ACT_GELU_NEW: known at compile time; -1: the run-time
// switch on p.act (hipcc does not hoist it out of the element loop although p.act is uniform: ~5 scalar compare-and-branch
// pairs per element).  Same arithmetic either way.
template <int CACT>
__device__ __forceinline__ float cons_act(float v, int act) {
    if constexpr (CACT == RGRG_ACT_NONE) return v;
    else if constexpr (CACT == RGRG_ACT_GELU_NEW) return gelu_new_fast(v);
    else return apply_act_fast(v, act);
}

// ---- tile order
// workgroup id -> XCD-aware band: the 1/8 of the grid an XCD receives (ids i mod 8) becomes a run of consecutive tile ids, so
// its L2 holds A plus one band of W; bijective for any total
__device__ __forceinline__ int xcd_band_tile(int block, int total) {
    const int q = total >> 3, r = total & 7, x = block & 7, i = block >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}
// tile id -> (row tile .x, column tile .y): column-major (rows fastest) when gm <= 0 or gm >= mtiles, else the grouped order of
// GemmBf16Params::gm (all column tiles of gm row tiles before the next group; all groups but the last hold gm row tiles).
// (Results come back by value: with reference out-parameters the 256 x 256 kernel's code changed.)
__device__ __forceinline__ int2 grouped_tile(int t, int gm, int mtiles, int ntiles) {
    int tn, tm;
    if (gm <= 0 || gm >= mtiles) {
        tn = t / mtiles; tm = t - tn * mtiles;
    } else {
        const int gsz = gm * ntiles, g = t / gsz, r = t - g * gsz;
        const int rows = min(gm, mtiles - g * gm);
        tn = r / rows; tm = g * gm + (r - tn * rows);
    }
    return make_int2(tm, tn);
}

// ---- operand staging
// XOR swizzle of the 16-byte chunk lch of tile row `row` (byte offset inside the 128-byte LDS row): spreads the 16 rows of a
// ds_read_b128 lane group over all 16 slots of the 256-byte bank row (design comment of gemm_bf16_glds_kernel)
__device__ __forceinline__ int dma_swizzle(int row, int lch) { return (lch ^ ((row >> 1) & 7)) << 4; }
// per-lane source offset (bytes) of an LDS-DMA request: tile row `row` clamped to the operand's last valid row `limit` (rows
// past the edge read it again, never stored), row pitch ld elements, swizzled chunk
__device__ __forceinline__ int dma_src_off(int row, int limit, int ld, int lch) { return min(row, limit) * ld * 2 + dma_swizzle(row, lch); }
// fragment read offset (bytes inside a 32-row block of 128-byte rows) of K step ks (4 steps of 16 per tile) for the lane that
// reads row frow = lane & 31, k half fh = lane >> 5: the swizzle of dma_swizzle applied again
__device__ __forceinline__ int frag_offset(int frow, int fh, int ks) {
    const int fsw = (frow >> 1) & 7;
    return frow * 128 + (((2 * ks + fh) ^ fsw) << 4);
}
template <int MI, int NI>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[MI][NI]) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
}
// RGRG_PP_DBG measurement modes: the constant A / W fragments that stand in for whatever a mode skips
__device__ __forceinline__ bf16x8 dbg_frag_a() { return bf16x8{1, 2, 3, 4, 5, 6, 7, 8}; }
__device__ __forceinline__ bf16x8 dbg_frag_b() { return bf16x8{8, 7, 6, 5, 4, 3, 2, 1}; }

// ---- the C/D layout of the 32x32 MFMA: register r of a lane = column lane & 31, row c_row(r) + 4 * (lane >> 5) of the block.
// base: the row the sum starts from (base first, then the two terms: the order the kernels' address arithmetic was written in)
__device__ __forceinline__ constexpr int c_row(int r, int base = 0) { return base + (r & 3) + 8 * (r >> 2); }

// The helpers below handle ONE register r of the lane's 16; the kernels keep the unrolled loop over r.
// fp32 value [M, ld] at column colc of row rbase + c_row(r), the row clamped to M - 1 (the loads of a block are issued together
// and unpredicated; only the stores are predicated)
__device__ __forceinline__ float c_load_f32(const float* src, int rbase, int r, int colc, int M, int ld) {
    const int row = min(c_row(r, rbase), M - 1);
    return src[(size_t)row * ld + colc];
}
// the same for a 16-bit value (R16, G16)
template <bool F16>
__device__ __forceinline__ float c_load_16(const u16* src, int rbase, int r, int colc, int M, int ld) {
    const int row = min(c_row(r, rbase), M - 1);
    return from16<F16>(src[(size_t)row * ld + colc]);
}
// element offset of row rbase + c_row(r), column col in a [M, ld] output (32-bit inside the tile's rows)
__device__ __forceinline__ size_t c_offset(int rbase, int r, int col, int ld) { return (size_t)rbase * ld + col + (size_t)(c_row(r) * ld); }
// the final store of ONE result v at offset o (the caller checks row < M and col < N): 16-bit Y16, or fp32 Y - STREAM:
// non-temporal when N > 8192 (logits: streamed, keep A / W in L2) - and, for the producer of a folded LayerNorm (YB), the 16-bit
// copy Yb16 next to it
template <bool F16, bool STREAM, bool YB>
__device__ __forceinline__ void c_store(size_t o, float v, u16* Y16, int N, float* Y, u16* Yb16) {
    if (Y16) Y16[o] = (u16)to16<F16>(v);
    else if (STREAM && N > 8192) __builtin_nontemporal_store(v, &Y[o]);
    else Y[o] = v;
    if constexpr (YB) Yb16[o] = (u16)to16<F16>(v);
}

// ---- LayerNorm folded around the GEMMs (GemmBf16Params)
// Consumer: (sum, sum of squares) of a row from its 16 slots, of which a thread holds PER = 16 / TPR (lsq: PER / 2 pairs of
// slots) and TPR adjacent threads share the row.  ONE summation order for every tile shape (a row's result must not depend on
// the tile the launcher picks for M): the 16 slots are added in groups of four (slot order, from zero), the groups pairwise:
// (G0 + G1) + (G2 + G3).  64-row tiles: a thread owns one group, the shuffles add them; 128-row tiles: a thread owns two groups
// and adds them first.  The caller turns the sums into (mean, rstd): the reciprocal square root stays on the storing thread's
// side of its branch.
template <int TPR, int PER>
__device__ __forceinline__ float2 ln_slot_sums(const f32x4 (&lsq)[PER / 2]) {
    static_assert(TPR * PER == 16 && (PER == 4 || PER == 8), "slot reduction is written for 64- and 128-row tiles");
    float ls1 = 0.f, ls2 = 0.f;
#pragma unroll
    for (int j0 = 0; j0 < PER / 2; j0 += 2) {
        float g1 = 0.f, g2 = 0.f;
#pragma unroll
        for (int j = j0; j < j0 + 2; ++j) { g1 += lsq[j][0]; g2 += lsq[j][1]; g1 += lsq[j][2]; g2 += lsq[j][3]; }
        if (j0 == 0) { ls1 = g1; ls2 = g2; } else { ls1 += g1; ls2 += g2; }
    }
#pragma unroll
    for (int o = 1; o < TPR; o <<= 1) { ls1 += __shfl_xor(ls1, o, 64); ls2 += __shfl_xor(ls2, o, 64); }
    return make_float2(ls1, ls2);
}
__device__ __forceinline__ float ln_mean(float ls1) { return ls1 * (1.0f / 1024.0f); }
__device__ __forceinline__ float ln_var(float ls2, float mean) { return fmaxf(ls2 * (1.0f / 1024.0f) - mean * mean, 0.f); }

// Producer: per-row (sum, sum of squares) of a 32-column block of results vv (C layout): a halving butterfly over the 32 lanes
// that share the block's rows (16 -> 8 -> 4 -> 2 -> 1 rows per lane, then the pair), fixed order.  Lane L (and L ^ 1) ends up
// with row ln_block_sum_row(L) of its half of the block.  (Written with constant steps: as nested loops hipcc kept the arrays
// indexed dynamically - ~900 v_cndmask, 1.5 us per launch.)
__device__ __forceinline__ float2 ln_block_row_sums(const float (&vv)[16], int lane) {
    float a1[16], a2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { a1[r] = vv[r]; a2[r] = vv[r] * vv[r]; }
#define RGRG_BFLY(H, BIT)                                                                 \
    {                                                                                     \
        const bool up = (lane & (BIT)) != 0;                                              \
        _Pragma("unroll") for (int i = 0; i < (H); ++i) {                                 \
            const float s1 = up ? a1[i] : a1[i + (H)], s2 = up ? a2[i] : a2[i + (H)];     \
            const float k1 = up ? a1[i + (H)] : a1[i], k2 = up ? a2[i + (H)] : a2[i];     \
            a1[i] = k1 + __shfl_xor(s1, (BIT), 64);                                       \
            a2[i] = k2 + __shfl_xor(s2, (BIT), 64);                                       \
        }                                                                                 \
    }
    RGRG_BFLY(8, 16) RGRG_BFLY(4, 8) RGRG_BFLY(2, 4) RGRG_BFLY(1, 2)
#undef RGRG_BFLY
    a1[0] += __shfl_xor(a1[0], 1, 64);
    a2[0] += __shfl_xor(a2[0], 1, 64);
    return make_float2(a1[0], a2[0]);
}
__device__ __forceinline__ int ln_block_sum_row(int lane) { return c_row((lane >> 1) & 15) + 4 * (lane >> 5); }
// One slot of stats_out [M][16][2] per 64 columns.  A 128-wide tile's wave covers 64 (its two blocks are already added); in a
// 64-wide tile (NI == 1) the two waves of a row block hold 32 columns each and meet in LDS: wave w (wn = 1) leaves its sums with
// ln_stats_hand_over, the kernel passes a workgroup barrier, wave w - 1 (wn = 0) adds them in ln_stats_store.
// xch: [4 waves][MI][32 rows]; lrow = ln_block_sum_row(lane); row0 = the first matrix row of the wave's sub-tile
template <int MI>
__device__ __forceinline__ void ln_stats_hand_over(float2* xch, int w, int lrow, const float (&blk1)[MI], const float (&blk2)[MI]) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) xch[(w * MI + mi) * 32 + lrow] = make_float2(blk1[mi], blk2[mi]);
}
template <int MI, int NI>
__device__ __forceinline__ void ln_stats_store(const float2* xch, int w, int lrow, const float (&blk1)[MI], const float (&blk2)[MI], int row0,
                                               int slot, int M, float* stats_out) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        float s1 = blk1[mi], s2 = blk2[mi];
        if constexpr (NI == 1) {
            const float2 o = xch[((w + 1) * MI + mi) * 32 + lrow];
            s1 += o.x; s2 += o.y;
        }
        const int row = row0 + mi * 32 + lrow;
        if (row < M) *reinterpret_cast<float2*>(stats_out + ((size_t)row * 16 + slot) * 2) = make_float2(s1, s2);
    }
}

}  // namespace rgrg
