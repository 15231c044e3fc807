// Greedy decoder of the RGRG language model (GPT-2 medium with pseudo self-attention)
// for gfx950.  Replaces LanguageModel.generate(num_beams=1) -> greedy_search ->
// forward -> GPT2PseudoAttention (src/language_model/language_model.py:401-447,
// :609-652, :258-366, :124-180 of ttanida/rgrg).
//
// Design (MI355X-first):
//  * KV cache pre-allocated [layer][k|v][seq][head][slot][64]; slot 0 holds the image
//    key/value (uk/uv of the transformed region feature), slot t+1 the token of step t.
//    Nothing is re-allocated or concatenated per step.
//  * One decode step = a fixed kernel sequence whose only step-dependent inputs live in
//    DEVICE memory (step counter, finished flags, id buffer), so the step is captured
//    once per sequence count into a hipGraph and replayed; EOS bookkeeping, PAD fill and
//    the "all finished" length are computed on device, the host polls every 16 steps.
//  * <= 32 sequences (one image = 29 regions): every projection is a weight-streaming
//    "skinny" GEMM: weights pre-packed into v_mfma_f32_32x32x2_f32 B-fragment order so a
//    wave streams them as fully coalesced 1-KiB loads straight into registers (HBM-bound,
//    no LDS round trip); activations (<=32 rows) are the A operand; the K range is split
//    over the 4 waves of a workgroup (+ over workgroups when N is small) and reduced in a
//    fixed order -> bitwise reproducible.
//  * > 32 sequences: the same step runs on the tiled MFMA GEMM of gemm_f32.hip.
//
// This file: the decode step, the decoder object, forward_cached, set_precision and the timing hooks.  The decode attention is in
// attn_decode.hip, beam search in decoder_beam.hip, the teacher-forced and training passes in decoder_lm.hip; decoder_internal.h
// holds what they share.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <cmath>
#include <vector>

#include "decoder_internal.h"

namespace rgrg {

int skinny_max_rows() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("RGRG_SKINNY_MAX_ROWS"); v = e ? atoi(e) : SKINNY_MAX_ROWS;
        if (v > SKINNY_MAX_ROWS) v = SKINNY_MAX_ROWS; if (v < 32) v = 32; }
    return v;
}

// ------------------------------------------------------------------ weight packing
// W [N,K] row-major -> P [NT][K/8][64 lanes][4]: lane l = (j = l&31, h = l>>5) holds
// W[nt*32+j][kc*8 + 4h .. +3]; rows >= N are zero.
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ W, float* __restrict__ P, int N,
                                                           int K, int NT) {
    const size_t total = (size_t)NT * (K / 8) * 64;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(o & 63);
        const size_t t = o >> 6;
        const int kc = (int)(t % (K / 8));
        const int nt = (int)(t / (K / 8));
        const int n = nt * 32 + (l & 31);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (n < N) v = *reinterpret_cast<const f32x4*>(W + (size_t)n * K + kc * 8 + (l >> 5) * 4);
        reinterpret_cast<f32x4*>(P)[o] = v;
    }
}

// ------------------------------------------------------------------ skinny GEMM
struct SkinnyArgs {
    const float* X;     // [32][K] (rows >= M are zero)
    const float* P;     // packed weights
    const float* bias;  // [N] or null
    const float* R;     // residual [32][ldy] or null
    float* Y;           // [32][ldy]
    float* part;        // [KS][32][NT*32] partial sums when KS > 1
    int M, K, N, NT, KS, ldy, act;
};

__device__ __forceinline__ void skinny_store(const SkinnyArgs& a, int row, int col, float v) {
    if (row >= a.M || col >= a.N) return;
    if (a.bias) v += a.bias[col];
    if (a.R) v += a.R[(size_t)row * a.ldy + col];
    a.Y[(size_t)row * a.ldy + col] = apply_act(v, a.act);
}

constexpr int SK_WAVES = 8;  // K is split over the 8 waves of a workgroup (and over KS workgroups)

typedef float f32x4v __attribute__((ext_vector_type(4)));

// Weight-streaming GEMM of the PREFILL (feature_space_transformation_nn, uk / uv of all layers; <= 128 activation
// rows).  One workgroup = one 32-column tile of the output x one K slice (K / KS):
//   1. the 32 x (K/KS) activation slice is staged ONCE into LDS with fully coalesced 16-B
//      loads (rows padded by 4 floats -> conflict-free ds_read_b128 A fragments);
//   2. each of the 8 waves streams its PW one-KiB chunks of pre-packed weights straight into
//      registers (non-temporal, all PW loads in flight before the first MFMA);
//   3. v_mfma_f32_32x32x2_f32 drains the chunks in arrival order; the 8 per-wave accumulators are summed
//      through LDS in a fixed order.
// KS == 1: bias / residual / activation epilogue; KS > 1: partial sums to a.part, combined by skinny_reduce_kernel.
// (The decode steps use the fragment-direct kernels of skinny_direct.inc.)
template <int PW, int MT>
__global__ __launch_bounds__(512) void rgrg_skinny_gemm_f32(const SkinnyArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KC = 8;                        // k per weight chunk
    constexpr int KWG = PW * SK_WAVES * KC;      // K slice of this workgroup
    constexpr int LDX = KWG + 4;
    constexpr int XQ = KWG / 64;                 // float4 staging loads per thread (32*KWG/4/512)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x, ks = blockIdx.y;
    const int chunks = a.K / KC;
    const int kc0 = (ks * SK_WAVES + wave) * PW;
    const float* xsrc = a.X + (size_t)ks * KWG;
    f32x4 xr[XQ];
    auto load_x = [&](int mt) {  // 32 activation rows of row tile mt, fully coalesced
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = tid + 512 * q;
            const int row = idx / (KWG / 4), c4 = idx - row * (KWG / 4);
            xr[q] = *reinterpret_cast<const f32x4*>(xsrc + (size_t)(mt * 32 + row) * a.K + c4 * 4);
        }
    };
    load_x(0);
    __builtin_amdgcn_sched_barrier(0);  // activations first: they gate the first MFMA
    const f32x4* wp = reinterpret_cast<const f32x4*>(a.P) + ((size_t)nt * chunks + kc0) * 64 + lane;
    f32x4 w[PW];
#pragma unroll
    for (int c = 0; c < PW; ++c) w[c] = __builtin_nontemporal_load(wp + (size_t)c * 64);
    __builtin_amdgcn_sched_barrier(0);
    // The weights stay in registers while up to MT row tiles (32 sequences each) are streamed through LDS:
    // W is fetched from HBM once for up to 128 sequences.
    float acc[MT][16];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (mt > 0) __syncthreads();  // every wave has finished reading the previous tile
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = tid + 512 * q;
            const int row = idx / (KWG / 4), c4 = idx - row * (KWG / 4);
            *reinterpret_cast<f32x4*>(&smem[row * LDX + c4 * 4]) = xr[q];
        }
        __syncthreads();
        if (mt + 1 < MT) load_x(mt + 1);  // in flight during this tile's MFMAs
        f32x16 c16;
#pragma unroll
        for (int r = 0; r < 16; ++r) c16[r] = 0.f;
        const float* xa = &smem[(lane & 31) * LDX + wave * PW * KC + (lane >> 5) * 4];
#pragma unroll
        for (int c = 0; c < PW; ++c) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(xa + c * KC);
#pragma unroll
            for (int j = 0; j < 4; ++j) c16 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[j], w[c][j], c16, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = c16[r];
    }
    float* red = smem;  // re-used after the MFMA loop
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        __syncthreads();  // LDS free: MFMA reads (mt == 0) or the previous tile's reduction are done
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[mt][r];
        __syncthreads();
        const int row0 = mt * 32;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = tid + 512 * q;
            const int r = idx >> 6, l = idx & 63;
            float v = red[r * 64 + l];
#pragma unroll
            for (int w2 = 1; w2 < SK_WAVES; ++w2) v += red[(w2 * 16 + r) * 64 + l];
            const int lrow = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            const int col = nt * 32 + (l & 31);
            if (a.KS == 1) skinny_store(a, row0 + lrow, col, v);
            else a.part[(((size_t)mt * a.KS + ks) * PAD_ROWS + lrow) * (a.NT * 32) + col] = v;
        }
    }
}

// Persistent variant for very wide outputs (uk/uv of all layers: 1536 column tiles): the
// grid is one workgroup per CU; each workgroup stages the (<= 31) activation rows ONCE and
// then walks column tiles nt = blockIdx.x, += gridDim.x.  A tile's 16 weight chunks per wave
// live in two 8-chunk register buffers that are refilled with the NEXT tile's chunks as soon
// as the MFMAs have consumed them, so 8-16 KiB per wave stay in flight through the MFMA
// phase and the (8-wave parallel, fixed-order) reduction + epilogue of the current tile.
__global__ __launch_bounds__(512) void rgrg_skinny_gemm_f32_wide(const SkinnyArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int PW = 16, KC = 8, KWG = PW * SK_WAVES * KC, LDX = KWG + 4, XQ = KWG / 64;
    float* red = smem + a.M * LDX;  // [8][16][64]; rows >= M of the A operand read garbage that only
                                    // reaches output rows >= M, which are never stored
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunks = a.K / KC;
    {
        f32x4 xr[XQ];
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = tid + 512 * q;
            const int row = idx / (KWG / 4), c4 = idx - row * (KWG / 4);
            xr[q] = *reinterpret_cast<const f32x4*>(a.X + (size_t)row * a.K + c4 * 4);
        }
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = tid + 512 * q;
            const int row = idx / (KWG / 4), c4 = idx - row * (KWG / 4);
            if (row < a.M) *reinterpret_cast<f32x4*>(&smem[row * LDX + c4 * 4]) = xr[q];
        }
    }
    __syncthreads();
    const float* xa = &smem[(lane & 31) * LDX + wave * PW * KC + (lane >> 5) * 4];
    const f32x4* wbase = reinterpret_cast<const f32x4*>(a.P) + ((size_t)wave * PW) * 64 + lane;
    f32x4 wa[8], wb[8];
    auto load8 = [&](f32x4(&w)[8], int nt, int half) {
        const f32x4* wp = wbase + ((size_t)nt * chunks + half * 8) * 64;
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c] = __builtin_nontemporal_load(wp + (size_t)c * 64);
    };
    int nt = blockIdx.x;
    if (nt < a.NT) { load8(wa, nt, 0); load8(wb, nt, 1); }
    for (; nt < a.NT; nt += gridDim.x) {
        const int nxt = nt + gridDim.x;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(xa + c * KC);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[j], wa[c][j], acc, 0, 0, 0);
        }
        if (nxt < a.NT) load8(wa, nxt, 0);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(xa + (8 + c) * KC);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[j], wb[c][j], acc, 0, 0, 0);
        }
        if (nxt < a.NT) load8(wb, nxt, 1);
        __syncthreads();  // every thread has finished reading `red` of the previous tile
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[r];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = tid + 512 * q;
            const int r = idx >> 6, l = idx & 63;
            float v = red[r * 64 + l];
#pragma unroll
            for (int w2 = 1; w2 < SK_WAVES; ++w2) v += red[(w2 * 16 + r) * 64 + l];
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            const int col = nt * 32 + (l & 31);
            skinny_store(a, row, col, v);
        }
    }
}


#include "skinny_direct.inc"

constexpr int WIDE_MAX_ROWS = 31;  // 31 staged rows + the 32 KiB reduction buffer fill the 160 KiB LDS
constexpr size_t WIDE_LDS = (size_t)(WIDE_MAX_ROWS * (16 * SK_WAVES * 8 + 4) + SK_WAVES * 16 * 64) * sizeof(float);
static_assert(WIDE_LDS <= 160 * 1024, "wide skinny GEMM must fit the 160 KiB LDS");

template <int PW, int MT>
static int launch_skinny(const SkinnyArgs& a, hipStream_t st) {
    constexpr size_t lds_x = (size_t)32 * (PW * SK_WAVES * 8 + 4) * sizeof(float);
    constexpr size_t lds_r = (size_t)SK_WAVES * 16 * 64 * sizeof(float);
    constexpr size_t lds = lds_x > lds_r ? lds_x : lds_r;
    hipLaunchKernelGGL((rgrg_skinny_gemm_f32<PW, MT>), dim3(a.NT, a.KS), dim3(64 * SK_WAVES), lds, st, a);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

template <int PW>
static int launch_skinny_mt(const SkinnyArgs& a, hipStream_t st) {
    const int mt = (a.M + PAD_ROWS - 1) / PAD_ROWS;
    if (mt <= 1) return launch_skinny<PW, 1>(a, st);
    if (mt == 2) return launch_skinny<PW, 2>(a, st);
    if (mt == 3) return launch_skinny<PW, 3>(a, st);
    if (mt == 4) return launch_skinny<PW, 4>(a, st);
    set_error("skinny GEMM: %d rows exceed 4 row tiles", a.M);
    return RGRG_EINVAL;
}

// chunks-per-wave PW = K / (8 * KS * 8) must be one of the instantiated values
static int launch_skinny_any(const SkinnyArgs& a, hipStream_t st) {
    const int pw = a.K / (8 * a.KS * SK_WAVES);
    if (pw == 16 && a.KS == 1 && a.NT > 512 && a.M <= WIDE_MAX_ROWS) {
        hipLaunchKernelGGL(rgrg_skinny_gemm_f32_wide, dim3(256), dim3(64 * SK_WAVES), WIDE_LDS, st, a);
        RGRG_LAUNCH_CHECK();
        return RGRG_OK;
    }
    if (pw == 4) return launch_skinny_mt<4>(a, st);
    if (pw == 8) return launch_skinny_mt<8>(a, st);
    if (pw == 16) return launch_skinny_mt<16>(a, st);
    set_error("skinny GEMM: unsupported shape K=%d KS=%d (chunks per wave %d)", a.K, a.KS, pw);
    return RGRG_EINVAL;
}

__global__ __launch_bounds__(256) void skinny_reduce_kernel(const SkinnyArgs a) {
    const int ldp = a.NT * 32;
    const int total = a.M * a.N;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int row = i / a.N, col = i - row * a.N;
        float v = 0.f;
        const float* pt = a.part + ((size_t)(row >> 5) * a.KS * PAD_ROWS + (row & 31)) * ldp + col;
        for (int ks = 0; ks < a.KS; ++ks) v += pt[(size_t)ks * PAD_ROWS * ldp];
        skinny_store(a, row, col, v);
    }
}

// ------------------------------------------------------------------ small kernels

// x[s] = wte[ids[s][t]] + wte[t] (quirk: positions are embedded with wte, language_model.py:307),
// xn[s] = ln_1 of layer 0.  One workgroup per sequence, D == 1024.
__global__ __launch_bounds__(256) void embed_ln_kernel(const float* __restrict__ wte, const long long* __restrict__ ids,
                                                       int ld_ids, const int* __restrict__ step, const float* __restrict__ g,
                                                       const float* __restrict__ b, float* __restrict__ x,
                                                       float* __restrict__ xn, int D, const int* __restrict__ tok_override,
                                                       unsigned short* __restrict__ xn16, int f16, const int* __restrict__ pos_override,
                                                       float* __restrict__ stats) {
    __shared__ float sh[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int t = pos_override ? pos_override[s] : *step;   // forward(position_ids=...): the caller's position of this row
    const long long tok = tok_override ? (long long)tok_override[s] : ids[(size_t)s * ld_ids + *step];  // beam search feeds the beam tokens
    const f32x4 v = reinterpret_cast<const f32x4*>(wte + (size_t)tok * D)[tid] + reinterpret_cast<const f32x4*>(wte + (size_t)t * D)[tid];
    reinterpret_cast<f32x4*>(x + (size_t)s * D)[tid] = v;
    if (stats) {
        // LayerNorm folded into the consuming GEMM (16-bit many-sequence path): the RAW row as 16 bit plus its (sum, sum of
        // squares) in slot 0 of the row's 16 slots - the layout the GEMM epilogues write (gemm_bf16.hip)
        store_16x4(xn16 + (size_t)s * D + 4 * tid, v, f16);
        const float s1 = block_sum_256((v[0] + v[1]) + (v[2] + v[3]), sh);
        const float s2 = block_sum_256((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]), sh);
        if (tid < 16) reinterpret_cast<float2*>(stats)[(size_t)s * 16 + tid] = tid ? make_float2(0.f, 0.f) : make_float2(s1, s2);
        return;
    }
    const f32x4 o = ln_row(v, g, b, sh, D);
    if (xn16) store_16x4(xn16 + (size_t)s * D + 4 * tid, o, f16);  // 16-bit-activation mode: the GEMMs read only this copy
    else reinterpret_cast<f32x4*>(xn + (size_t)s * D)[tid] = o;
}
// one workgroup per row; the three output modes are the kernel's: stats (raw 16-bit row + slots), else xn16, else xn
static int launch_embed_ln(const float* wte, const long long* ids, int ld_ids, const int* step, const float* g, const float* b, float* x,
                           float* xn, int D, const int* tok_override, unsigned short* xn16, int f16, const int* pos_override, float* stats,
                           int rows, hipStream_t st) {
    hipLaunchKernelGGL(embed_ln_kernel, dim3(rows), dim3(256), 0, st, wte, ids, ld_ids, step, g, b, x, xn, D, tok_override, xn16, f16,
                       pos_override, stats);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// xn[row] = LayerNorm(x[row]) (many-sequence path and the teacher-forced passes: the tiled GEMM's epilogue already added
// bias + residual into x).  One WAVE per row of 1024 (four rows per workgroup): 16 values per lane as four coalesced 1-KiB
// loads, both reductions by DPP inside the wave - no LDS, no barrier (the one-row-per-workgroup version spent its 5 us
// in two block reductions: 12 192 launches = 6 % of a batch-32 run).  Two-pass variance like nn.LayerNorm.
__global__ __launch_bounds__(256) void ln_rows_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                      const float* __restrict__ b, float* __restrict__ xn, int D,
                                                      unsigned short* __restrict__ xn16, int f16, int rows) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
    f32x4 v[4], gg[4], bb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = xr[j * 64 + lane];
    // gain and bias are requested right behind the row (not after the two reductions): one memory latency per launch
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gg[j] = reinterpret_cast<const f32x4*>(g)[j * 64 + lane];
        bb[j] = reinterpret_cast<const f32x4*>(b)[j * 64 + lane];
    }
    __builtin_amdgcn_sched_barrier(0);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    const float mean = wave_sum_dpp(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[j][e] -= mean; q += v[j][e] * v[j][e]; }
    }
    const float rstd = 1.0f / sqrtf(wave_sum_dpp(q) / (float)D + LN_EPS);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[j][e] * rstd * gg[j][e] + bb[j][e];
        if (xn16) store_16x4(xn16 + (size_t)row * D + 4 * (j * 64 + lane), o, f16);
        else reinterpret_cast<f32x4*>(xn + (size_t)row * D)[j * 64 + lane] = o;
    }
}
int launch_ln_rows(const float* x, const float* g, const float* b, float* xn, int D, unsigned short* xn16, int f16, int rows,
                   hipStream_t st) {
    hipLaunchKernelGGL(ln_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, g, b, xn, D, xn16, f16, rows);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// image key/value (uk/uv outputs) -> cache slot 0 of every layer
template <typename KV>  // float, u16 (16-bit cache) or uint8_t (e4m3 cache: clamp and one rounding, common.h)
__global__ __launch_bounds__(256) void kv_slot0_kernel(const float* __restrict__ ukv, int ld, KV* __restrict__ kv_all,
                                                       size_t layer_stride, size_t kv_stride, int S, int H, int T,
                                                       int L, int row_mul, int f16) {
    const int D = H * 64;
    const size_t total = (size_t)L * 2 * S * D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % D);
        size_t r = i / D;
        const int s = (int)(r % S);
        r /= S;
        const int kv = (int)(r & 1), l = (int)(r >> 1);
        const int hd = d >> 6, e = d & 63;
        const float val = ukv[(size_t)s * ld + ((size_t)l * 2 + kv) * D + d];
        const size_t o = (size_t)l * layer_stride + (size_t)kv * kv_stride + (((size_t)s * row_mul * H + hd) * T) * 64 + e;
        if constexpr (sizeof(KV) == 1) kv_all[o] = (KV)f32_to_e4m3_bits(val);
        else if constexpr (sizeof(KV) == 2) kv_all[o] = (KV)to16_rt(val, f16);
        else kv_all[o] = val;
    }
}
// The cache lives in one allocation with the same ELEMENT strides in every format (half / a quarter of the bytes used); f16 names the
// 16-bit type and is read by that format alone.  1024 workgroups whatever the size: the kernel strides.
static int launch_kv_slot0(const float* ukv, int ld, void* kv, size_t layer_stride, size_t kv_stride, int S, int H, int T, int L, int row_mul,
                           KvFormat fmt, int f16, hipStream_t st) {
    if (fmt == KV_E4M3)
        hipLaunchKernelGGL(kv_slot0_kernel<uint8_t>, dim3(1024), dim3(256), 0, st, ukv, ld, static_cast<uint8_t*>(kv), layer_stride, kv_stride, S,
                           H, T, L, row_mul, 0);
    else if (fmt != KV_F32)
        hipLaunchKernelGGL(kv_slot0_kernel<u16>, dim3(1024), dim3(256), 0, st, ukv, ld, static_cast<u16*>(kv), layer_stride, kv_stride, S, H, T, L,
                           row_mul, f16);
    else
        hipLaunchKernelGGL(kv_slot0_kernel<float>, dim3(1024), dim3(256), 0, st, ukv, ld, static_cast<float*>(kv), layer_stride, kv_stride, S, H,
                           T, L, row_mul, 0);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// First-occurrence arg-max over the vocabulary (torch.argmax) fused with the greedy_search
// bookkeeping (:629-650).  The lm_head GEMM already reduced every 16- / 32-column tile to one
// (max, index) candidate (ties: lower index), so a row is NT <= 3142 candidates: a thread requests its
// (up to 13) candidates up front with clamped indices - one memory latency instead of one per loop trip.
// The bookkeeping (PAD / EOS / the packed arrival ticket) is record_step_token, the reduction argmax_candidates_row (decoder_internal.h).
__global__ __launch_bounds__(256) void argmax_update_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_idx,
                                                            int NT, long long* __restrict__ ids, int ld_ids,
                                                            int* __restrict__ finished, int* __restrict__ step,
                                                            int* __restrict__ done_len, int* __restrict__ sync, int S) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int row = blockIdx.x;
    const int t = *step;
    const int idx = argmax_candidates_row(cand_val + (size_t)row * NT, cand_idx + (size_t)row * NT, NT, bv, bi);
    if (threadIdx.x == 0) {
        const StepBook bk{ids, ld_ids, finished, step, done_len, sync, S};
        record_step_token(bk, row, t, idx == 0x7fffffff ? 0 : idx);
    }
}

// tiled-GEMM path (> 128 sequences): reduce the logits row to per-32-column candidates first.  HBM bound (the logits
// are 186 MB at 928 rows): a lane reads 16 bytes (4 columns), 8 lanes cover a 32-column tile, a wave 8 tiles per load
// with 4 loads in flight; the 8 lanes of a tile reduce with three DPP steps (first maximum wins: lower column on ties).
__global__ __launch_bounds__(256) void logits_candidates_kernel(const float* __restrict__ logits, int ld, int V, int NT,
                                                                float* __restrict__ cand_val, int* __restrict__ cand_idx) {
    const int row = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* x = logits + (size_t)row * ld;
    const int sub = lane & 7, tw = lane >> 3;     // lane -> (16-byte piece of the tile, tile within the wave's 8)
    constexpr int UN = 4;
    for (int t0 = (blockIdx.x * 4 + wave) * 8 * UN; t0 < NT; t0 += gridDim.x * 4 * 8 * UN) {
        f32x4 v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int nt = min(t0 + u * 8 + tw, NT - 1);   // clamped: the tail re-reads the last tile, results unused
            v[u] = *reinterpret_cast<const f32x4*>(x + nt * 32 + sub * 4);   // ld >= NT * 32: always inside the row
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int nt = t0 + u * 8 + tw;
            const int c0 = min(nt, NT - 1) * 32 + sub * 4;
            float bv = -INFINITY;
            int bi = c0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float val = (c0 + e < V) ? v[u][e] : -INFINITY;
                if (val > bv) { bv = val; bi = c0 + e; }
            }
#define CAND_STEP(CTRL)                                                                                     \
    {                                                                                                       \
        const float ov = dpp_get<CTRL, 0xf>(bv);                                                            \
        const int oi = __builtin_amdgcn_update_dpp(0, bi, CTRL, 0xf, 0xf, false);                           \
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }                                         \
    }
            CAND_STEP(0xB1) CAND_STEP(0x4E) CAND_STEP(0x141)   // lanes ^1, ^2, then 7 - i: all 8 lanes of the tile
#undef CAND_STEP
            if (sub == 0 && nt < NT) {
                cand_val[(size_t)row * NT + nt] = bv;
                cand_idx[(size_t)row * NT + nt] = bi;
            }
        }
    }
}

__global__ __launch_bounds__(256) void decode_reset_kernel(long long* __restrict__ ids, int ld_ids, int* __restrict__ finished,
                                                           int* __restrict__ step, int* __restrict__ done_len,
                                                           int* __restrict__ sync, int S, int L) {
    const size_t total = (size_t)S * L;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        ids[(i / L) * ld_ids + (i % L)] = (i % L) == 0 ? BOS_ID : PAD_ID;
    if (blockIdx.x == 0) {
        for (int s = threadIdx.x; s < S; s += 256) finished[s] = 0;
        if (threadIdx.x == 0) { *step = 0; *done_len = 0; }
        if (threadIdx.x < 2) sync[threadIdx.x] = 0;
    }
}
static int launch_decode_reset(long long* ids, int ld_ids, int* finished, int* step, int* done_len, int* sync, int S, int L, hipStream_t st) {
    hipLaunchKernelGGL(decode_reset_kernel, dim3(64), dim3(256), 0, st, ids, ld_ids, finished, step, done_len, sync, S, L);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// LayerNorm(gain, beta) folded into the [N,K] weight of the GEMM behind it, 16-bit flavour (one wave per output column):
// wb[n][k] = round16(gain[k] w[n][k]); cs[n] = sum_k wb[n][k] of the rounded values - what the GEMM really multiplies the
// mean with -, c2[n] = b[n] + sum_k beta[k] w[n][k].  LN(x) W^T + b = rstd (x wb^T - mean cs) + c2 up to the 16-bit
// rounding of x instead of LN(x) (both relative roundings of the same magnitude as long as |mean| is not >> std).
__global__ __launch_bounds__(256) void ln_fold16_kernel(const float* __restrict__ w, const float* __restrict__ gain,
                                                        const float* __restrict__ beta, const float* __restrict__ b,
                                                        unsigned short* __restrict__ wb, float* __restrict__ cs,
                                                        float* __restrict__ c2, int N, int K, int f16) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float a = 0.f, c = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float wv = w[(size_t)n * K + k];
        float gw = gain[k] * wv;
        asm("" : "+v"(gw));   // the fp32 product, THEN the 16-bit rounding (what torch's (W * g).to(half) does): without this the
                              // compiler fuses multiply + conversion into v_fma_mixlo_f16, i.e. one rounding of the exact product
        const unsigned short r = (unsigned short)to16_rt(gw, f16);
        wb[(size_t)n * K + k] = r;
        a += from16_rt(r, f16);
        c += beta[k] * wv;
    }
    a = wave_sum(a);
    c = wave_sum(c);
    if (lane == 0) { cs[n] = a; c2[n] = (b ? b[n] : 0.f) + c; }
}

// ------------------------------------------------------------------ decoder object (struct rgrg_decoder: decoder_internal.h)
int dmalloc(rgrg_decoder* d, void** p, size_t bytes, bool zero) {
    RGRG_HIP(hipMalloc(p, bytes));
    d->allocs.push_back(*p);
    if (zero) RGRG_HIP(hipMemset(*p, 0, bytes));
    return RGRG_OK;
}

static int pick_ks(int NT, int chunks) {
    // Wide outputs (>= 64 column tiles) keep the whole K in one workgroup: no partial sums.
    // Narrow ones (N = 1024) split K over workgroups until ~all CUs stream, keeping a
    // multiple of 4 one-KiB chunks per wave; skinny_reduce_kernel adds the partials.
    int ks = 1;
    if (NT >= 64) return ks;
    while (NT * ks < 256 && chunks % (ks * 2 * SK_WAVES * 4) == 0) ks *= 2;
    return ks;
}

// Shapes and one-time packing of the two weight-streaming families.  make_lin / rgrg_decoder_set_precision run them on the decoder's
// buffers, the test hooks rgrg_debug_direct_pack / rgrg_debug_direct_linear / rgrg_debug_skinny_linear on the caller's - the rules
// exist once, here.
// fused plan: 16-column tiles, one 1024-wide K slice per workgroup (mlp_proj: 4 slices -> 256 workgroups, the fp32 MFMA work needs
// every CU; the 4 partial sums are added by the consumer while it loads its fragments)
static bool direct_shape(int N, int K, bool lnf, int* KS, int* NT) {
    if (N < 1 || !(K == DK_SLICE || (K == 4 * DK_SLICE && !lnf && N == DK_SLICE))) return false;
    *KS = K / DK_SLICE; *NT = (N + 15) / 16;
    return true;
}
// packed [NT][K / 16][64][4] = (W o ln_g) in fragment order; c1 / c2 (ln_g given): the folded LayerNorm vectors
static int direct_pack(const float* w, const float* b, const float* ln_g, const float* ln_b, int N, int K, int NT, float* packed,
                       float* c1, float* c2, hipStream_t st) {
    hipLaunchKernelGGL(pack_weights16_scaled_kernel, dim3(2048), dim3(256), 0, st, w, ln_g, packed, N, K, NT);
    RGRG_LAUNCH_CHECK();
    if (ln_g) {
        hipLaunchKernelGGL(ln_fold_vectors_kernel, dim3((N + 3) / 4), dim3(256), 0, st, w, ln_g, ln_b, b, c1, c2, N, K);
        RGRG_LAUNCH_CHECK();
    }
    return RGRG_OK;
}
// the 16-bit-weight copy: the fp32 fragments rounded to the type, and (c1_16 given: GEMMs behind a LayerNorm) the column sums of the
// ROUNDED values [NT * 16]
static int direct_pack16(const float* packed, void* packed16, float* c1_16, int NT, int K, int f16, hipStream_t st) {
    int r = convert_f32_to_bf16(packed, packed16, (size_t)NT * 16 * K, st, f16);
    if (r) return r;
    if (c1_16) {
        hipLaunchKernelGGL(packed16_colsum_kernel, dim3(NT), dim3(64), 0, st, (const unsigned short*)packed16, c1_16, NT * 16, K, f16);
        RGRG_LAUNCH_CHECK();
    }
    return RGRG_OK;
}
// prefill GEMMs (fst-nn, uk/uv): LDS-staged weight-streaming kernel, 32-column tiles; *pw = one-KiB chunks per wave
static bool skinny_shape(int N, int K, int* KS, int* NT, int* pw) {
    const int kc = 8;
    *NT = (N + 31) / 32;
    *KS = pick_ks(*NT, K / 8);
    *pw = K / (kc * *KS * SK_WAVES);
    return N >= 1 && K >= 1 && (K % (kc * *KS * SK_WAVES) == 0) && (*pw == 4 || *pw == 8 || *pw == 16);
}
static int skinny_pack(const float* w, float* packed, int N, int K, int NT, hipStream_t st) {
    hipLaunchKernelGGL(pack_weights_kernel, dim3(2048), dim3(256), 0, st, w, packed, N, K, NT);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

static int make_lin(rgrg_decoder* d, Lin& l, const float* w, const float* b, int N, int K, bool pack,
                    bool direct = false, const float* ln_g = nullptr, const float* ln_b = nullptr) {
    l.w = w; l.b = b; l.N = N; l.K = K;
    if (direct) {
        if (!direct_shape(N, K, ln_g != nullptr, &l.KS, &l.NT)) { set_error("decoder: N=%d K=%d unsupported by the fused plan", N, K); return RGRG_EINVAL; }
        l.direct = true; l.ntile = 16; l.lnf = ln_g != nullptr;
        int rc = dmalloc(d, (void**)&l.packed, (size_t)l.NT * 16 * K * sizeof(float), false);
        if (rc) return rc;
        if (l.lnf) {
            if ((rc = dmalloc(d, (void**)&l.c1, (size_t)N * sizeof(float), false)) ||
                (rc = dmalloc(d, (void**)&l.c2, (size_t)N * sizeof(float), false)))
                return rc;
        }
        return direct_pack(w, b, ln_g, ln_b, N, K, l.NT, l.packed, l.c1, l.c2, d->stream);
    }
    l.ntile = 32;
    int pw;
    if (!skinny_shape(N, K, &l.KS, &l.NT, &pw)) {
        set_error("decoder: no skinny GEMM instance for N=%d K=%d (ntile %d, KS %d, %d chunks per wave)", N, K, l.ntile, l.KS, pw);
        return RGRG_EINVAL;
    }
    if (pack) {
        const size_t bytes = (size_t)l.NT * l.ntile * K * sizeof(float);
        int rc = dmalloc(d, (void**)&l.packed, bytes, false);
        if (rc) return rc;
        return skinny_pack(w, l.packed, N, K, l.NT, d->stream);
    }
    return RGRG_OK;
}

// hipFuncSetAttribute is not capturable: raise the dynamic-LDS limit of every instance up front
template <int PW, int MT>
static int skinny_attr1() {
    constexpr size_t lds_x = (size_t)32 * (PW * SK_WAVES * 8 + 4) * sizeof(float);
    RGRG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&rgrg_skinny_gemm_f32<PW, MT>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_x > 65536 ? lds_x : 65536)));
    return RGRG_OK;
}
template <int PW>
static int skinny_attr() {
    int rc;
    if ((rc = skinny_attr1<PW, 1>())) return rc;
    if ((rc = skinny_attr1<PW, 2>())) return rc;
    if ((rc = skinny_attr1<PW, 3>())) return rc;
    return skinny_attr1<PW, 4>();
}
static int init_skinny_attrs() {
    int rc;
    RGRG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&rgrg_lm_head_wave_f32<DX_COMBINE4>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)LMH_LDS));
    if ((rc = skinny_attr<4>())) return rc;
    if ((rc = skinny_attr<8>())) return rc;
    RGRG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&rgrg_skinny_gemm_f32_wide),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)WIDE_LDS));
    return skinny_attr<16>();
}

// bf16 K/V cache: with the bf16 GEMMs, i.e. on the many-sequence path of the opt-in bf16 mode.  `rows` is the
// number of token rows of the decode steps (sequences x beams), the same for every launch of one generate call.
// Rows up to which a decode step runs the fused plan (fragment-direct skinny kernels): 128 without autocast (fp32, bit-exact).
// Under torch.autocast (16-bit mode), round 6:
//   * one row tile (<= 32 rows, batch-1 greedy decoding) stays on the bit-exact fp32 kernels;
//   * 33-64 rows run the SAME plan on 16-bit weights (skinny_direct.inc W16: half the weight stream, one 16-bit MFMA per k chunk):
//     greedy batch 2 (58 rows) 193 -> 166 ms per generate() call;
//   * anything larger takes the many-sequence 16-bit path: every workgroup of the fused plan reads ALL rows of its K slice for a
//     16-column tile, and from 3 row tiles on that L2 traffic (116 rows: ~360 MB per layer) costs more than the tiled 16-bit GEMMs'
//     launch chain - 1 image x 4 beams (116 rows, fp16): 914 ms on the fp32 plan, 724 ms on W16, 576 ms on the many-sequence path;
//     greedy batch 4: 352 / 273 / 199 ms (profiles/r06_small_batch_16bit_threshold.log, profiles/r06_w16_fused_ab.log).
// RGRG_SKINNY_MAX_ROWS_16 moves the boundary (32..128), RGRG_W16_FUSED=0 drops the 16-bit-weight copies (boundary 32).
static int skinny_max_rows16(bool w16) {
    static const int env = [] {
        const char* e = getenv("RGRG_SKINNY_MAX_ROWS_16");
        return e ? atoi(e) : 0;
    }();
    int n = env ? env : (w16 ? 64 : 32);
    n = n < 32 ? 32 : n;
    return n > skinny_max_rows() ? skinny_max_rows() : n;
}
static int decode_row_limit(const rgrg_decoder* d) { return d->bf16_gemms ? skinny_max_rows16(d->w16_fused) : skinny_max_rows(); }
static bool kv_is_bf16(const rgrg_decoder* d, int rows) { return d->bf16_gemms && rows > decode_row_limit(d); }
// ... and what that step's cache holds: e4m3 bytes replace the 16-bit type where rgrg_decoder_set_kv_format asked for them
static KvFormat kv_format(const rgrg_decoder* d, int rows) {
    if (!kv_is_bf16(d, rows)) return KV_F32;
    return d->kv8 ? KV_E4M3 : (d->f16() ? KV_F16 : KV_BF16);
}

// Y[:M] = act(X W^T + b + R).  Prefill GEMMs (packed, <= 128 rows): LDS-staged weight-streaming kernel (+ a small
// reduce kernel when the layer splits K over workgroups); everything else: tiled MFMA GEMM (fp32, or the bf16-weight
// kernel in the opt-in bf16 mode, optionally with bf16 activations in / out).
int linear(rgrg_decoder* d, const Lin& l, const float* X, const float* R, float* Y, int M, int ldy, int act,
           bool count, const unsigned short* X16, unsigned short* Y16, const GemmLnFold* ln) {
    if (M <= skinny_max_rows() && l.packed && !l.direct) {
        // up to 4 row tiles of 32 sequences in ONE launch: the weights stay in registers across the tiles
        SkinnyArgs a{X, l.packed, l.b, R, Y, d->part, M, l.K, l.N, l.NT, l.KS, ldy, act};
        int rc = launch_skinny_any(a, d->stream);
        if (rc) return rc;
        if (l.KS > 1) {
            const int total = M * l.N;
            hipLaunchKernelGGL(skinny_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, d->stream, a);
            RGRG_LAUNCH_CHECK();
        }
        if (count) {
            d->gemm_bytes_per_step += (size_t)l.N * l.K * sizeof(float);
            d->gemm_flops_per_step += 2.0 * M * l.N * l.K;
            d->gemm_launches_per_step += 1;
        }
        return RGRG_OK;
    }
    if (count) {
        d->gemm_flops_per_step += 2.0 * M * l.N * l.K;
        d->gemm_launches_per_step += 1;
    }
    if (d->bf16_gemms && l.wb && l.K % 256 == 0) {
        if (count) d->gemm_bytes_per_step += (size_t)l.N * l.K * 2;
        if (ln && ln->ln_colsum) {   // the LayerNorm in front of this GEMM is folded in: gain-scaled weights, folded shift
            if (!l.wb_ln || !X16) { set_error("decoder: folded LayerNorm weights missing"); return RGRG_EINVAL; }
            GemmLnFold f = *ln;
            f.ln_colsum = l.cs16;
            f.kp = (d->kp_gemms == 1 || d->kp_gemms == 3) ? 1 : 0;
            return launch_gemm_bf16w_ex(nullptr, X16, l.wb_ln, l.c2_16, R, Y16 ? nullptr : Y, Y16, M, l.N, l.K, ldy, act, d->stream, d->f16(), &f);
        }
        if (ln && ln->Yb16 && d->sk_ws && M <= d->rows) {
            // a producer of the many-sequence decode step (attn_proj / mlp_proj, N = 1024): split-K with a last-arriver reduce
            int ks = l.K >= 2048 ? d->sk_mlp : d->sk_attn;
            // automatic: a step of <= 256 rows has 16 x (1..4) output tiles of 64 x 64 for 256 CUs and a K loop of 16 / 64 tiles - the
            // hand-off costs less than the idle CUs (116 rows: mlp_proj on 4 slices, attn_proj on 2: 1 image x 4 beams 584 -> 544 ms,
            // greedy batch 4 200 -> 180 ms, profiles/r06_small_rows_splitk.log); larger steps fill the GPU and lose (r05_splitk_decode_ab.log)
            if (ks < 0) ks = (d->step_rows > 0 && d->step_rows <= 256) ? (l.K >= 2048 ? 4 : 2) : 1;
            if (ks > 1) {
                GemmLnFold f = *ln;
                // slabs and tickets are indexed by the launch-local tile id: a row range (enqueue_step runs several of them
                // concurrently on forked streams) gets the slice of the work space that belongs to its first 64-row tile -
                // ranges start on whole tiles, the allocation covers every tile of d->rows (shared slabs raced)
                const size_t r0 = d->xn16 ? (size_t)(reinterpret_cast<const unsigned short*>(ln->Yb16) - d->xn16) / (size_t)d->D : 0;
                const size_t tile0 = (r0 / 64) * (size_t)(l.N / 64);
                f.ksplit = ks; f.sk_ws = d->sk_ws + tile0 * 4 * 4096; f.sk_cnt = d->sk_cnt + tile0;
                return launch_gemm_bf16w_ex(nullptr, X16, l.wb, l.b, R, Y16 ? nullptr : Y, Y16, M, l.N, l.K, ldy, act, d->stream, d->f16(), &f);
            }
        }
        if (ln && ln->Yb16 && X16 && (d->kp_gemms == 1 || d->kp_gemms == 2)) {   // producer of the folded LayerNorm (attn_proj / mlp_proj)
            GemmLnFold f = *ln;
            f.kp = 1;
            return launch_gemm_bf16w_ex(nullptr, X16, l.wb, l.b, R, Y16 ? nullptr : Y, Y16, M, l.N, l.K, ldy, act, d->stream, d->f16(), &f);
        }
        return launch_gemm_bf16w_ex(X16 ? nullptr : X, X16, l.wb, l.b, R, Y16 ? nullptr : Y, Y16, M, l.N, l.K, ldy, act, d->stream, d->f16(), ln);
    }
    if (count) d->gemm_bytes_per_step += (size_t)l.N * l.K * sizeof(float);
    return launch_gemm_dense(X, l.w, l.b, R, Y, M, l.N, l.K, ldy, act, d->gemm_ws, d->gemm_ws_floats, d->stream);
}


// Greedy many-sequence step in 16-bit mode: the lm_head leaves per-tile arg-max candidates instead of logits (gemm_bf16.hip)
bool lm_head_cand_path(const rgrg_decoder* d, int S) {
    return S > decode_row_limit(d) && kv_is_bf16(d, S) && d->xn16 && d->lm_head.wb && d->lm_head.K % 256 == 0 &&
           gemm_bf16_cand_epilogue_ok(S, d->lm_head.N, d->lm_head.K);
}

// The attention of layer l for the S sequences from r0 on of step `s` (the many-sequence step may run as several row ranges on
// several streams, enqueue_step); att16 is the caller's pointer for sequence r0 already
// q_only: c_attn ran with the K/V-cache epilogue (step_qkv_cache / cons_kv_cache below)
static int launch_attention(rgrg_decoder* d, int l, const StepSpec& s, int r0, int S, unsigned short* att16, int frag_out = 0,
                            bool q_only = false) {
    const int D = d->D;
    AttnDecodeLaunch a{};
    a.q_only = q_only;
    a.ld_qkv = 3 * D; a.step = d->step; a.S = S; a.H = d->H; a.T = d->T; a.kmask = s.key_mask;
    a.src = s.src ? s.src + (size_t)r0 * d->T : nullptr;
    a.frag_out = frag_out; a.st = d->stream; a.plane_elems = d->kv_kv_stride;
    a.fmt = kv_format(d, S);
    if (a.fmt != KV_F32) {
        // RGRG_ATTN_WGS_PER_CU = n > 0: at most n * 256 workgroups, each wave walks several (sequence, head) items
        static const int cap = [] { const char* e = getenv("RGRG_ATTN_WGS_PER_CU"); return e ? atoi(e) : 0; }();
        // cache rows of sequence r0 (layout [sequence][head][slot][64]): every format lives in the same allocation with the same
        // ELEMENT strides, so the byte offset of a plane / of row r0 scales with the element size
        const size_t esz = a.fmt == KV_E4M3 ? 1 : sizeof(u16);
        unsigned char* kcr = reinterpret_cast<unsigned char*>(d->kv) + ((size_t)l * d->kv_layer_stride + (size_t)r0 * d->H * d->T * 64) * esz;
        a.f16 = d->f16(); a.max_wgs = cap > 0 ? cap * 256 : 0;
        a.qkv = d->qkv + (size_t)r0 * 3 * D; a.kc = kcr; a.vc = kcr + d->kv_kv_stride * esz;
        a.out = d->att + (size_t)r0 * D; a.out16 = att16;
        a.first = s.kv_first ? s.kv_first + r0 : nullptr;
        a.row_step = s.row_step ? s.row_step + r0 : nullptr;
    } else {
        float* kc = d->kv + (size_t)l * d->kv_layer_stride;
        a.qkv = d->qkv; a.kc = kc; a.vc = kc + d->kv_kv_stride; a.out = d->att;
        a.row_step = s.row_step;
    }
    return launch_attn_decode(a);
}

// The kernel choice of the fused plan for one GEMM whose DirectArgs are complete: lm_head' on one row tile -> a wave per column tile;
// attn_proj' on 17-32 rows -> one row half per workgroup; everything else the generic kernel <row tiles, MODE, LNF, W16>.
// direct_linear calls it with the decoder's buffers, the test hook rgrg_debug_direct_linear with the caller's.  *ran (optional)
// receives the DX_RAN_* code of the kernel that was launched.
constexpr int DX_RAN_GENERIC = 0, DX_RAN_HALF = 1, DX_RAN_LM_WAVE = 2;
static int direct_dispatch(const DirectArgs& a, bool lnf, int mode, int w16, hipStream_t st, int* ran = nullptr) {
    const int mt = (a.M + PAD_ROWS - 1) / PAD_ROWS;
    const dim3 grid(a.NT, a.KS), blk(64 * SK_WAVES);
    if (lnf && mode == DX_COMBINE4 && a.NT > 512 && mt == 1 && a.K == DK_SLICE) {  // lm_head, one row tile: a wave per column tile
        hipLaunchKernelGGL((rgrg_lm_head_wave_f32<DX_COMBINE4>), dim3(256), blk, LMH_LDS, st, a);
        if (ran) *ran = DX_RAN_LM_WAVE;
    } else if (!lnf && mode == DX_PLAIN && a.KS == 1 && mt == 1 && a.NT <= 64 && a.M > 16 && !a.cand_val) {
        // attn_proj': few column tiles, MFMA bound -> one row half per workgroup (2 x NT workgroups)
        hipLaunchKernelGGL(rgrg_skinny_direct_half_f32, dim3(a.NT, 2), blk, 0, st, a);
        if (ran) *ran = DX_RAN_HALF;
    } else {
#define DX_LAUNCH(MT_, MODE_, LNF_)                                                                                          \
    do {                                                                                                                      \
        if constexpr (MT_ > 1) {                                                                                              \
            if (w16 == 1) { hipLaunchKernelGGL((rgrg_skinny_direct_f32<MT_, MODE_, LNF_, 1>), grid, blk, 0, st, a); break; }  \
            if (w16 == 2) { hipLaunchKernelGGL((rgrg_skinny_direct_f32<MT_, MODE_, LNF_, 2>), grid, blk, 0, st, a); break; }  \
        }                                                                                                                     \
        hipLaunchKernelGGL((rgrg_skinny_direct_f32<MT_, MODE_, LNF_>), grid, blk, 0, st, a);                                  \
    } while (0)
#define DX_MODES(MT_)                                                                        \
    do {                                                                                     \
        if (!lnf && mode == DX_PLAIN) DX_LAUNCH(MT_, DX_PLAIN, false);                       \
        else if (lnf && mode == DX_PLAIN) DX_LAUNCH(MT_, DX_PLAIN, true);                    \
        else if (lnf && mode == DX_COMBINE4) DX_LAUNCH(MT_, DX_COMBINE4, true);              \
        else if (lnf && mode == DX_EMBED) DX_LAUNCH(MT_, DX_EMBED, true);                    \
        else if (lnf && mode == DX_EMBED_TOK) DX_LAUNCH(MT_, DX_EMBED_TOK, true);            \
        else if (lnf && mode == DX_EMBED_TOKPOS) DX_LAUNCH(MT_, DX_EMBED_TOKPOS, true);      \
        else { set_error("direct_linear: unsupported mode %d (lnf %d)", mode, (int)lnf); return RGRG_EINVAL; } \
    } while (0)
        if (mt == 1) DX_MODES(1);
        else if (mt == 2) DX_MODES(2);
        else if (mt == 3) DX_MODES(3);
        else if (mt == 4) DX_MODES(4);
        else { set_error("direct_linear: %d rows exceed 4 row tiles", a.M); return RGRG_EINVAL; }
#undef DX_MODES
#undef DX_LAUNCH
        if (ran) *ran = DX_RAN_GENERIC;
    }
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// One GEMM of the fused plan.  `a` arrives with the operand / output pointers and `act` set; the layer fills the rest.
static int direct_linear(rgrg_decoder* d, const Lin& l, DirectArgs a, int mode, int M, bool count, bool cand = false) {
    if (!l.direct) { set_error("direct_linear: layer was not packed for the fused plan"); return RGRG_EINVAL; }
    if (l.lnf && mode == DX_PLAIN && !a.Xf) { set_error("direct_linear: missing operand"); return RGRG_EINVAL; }
    a.P = l.packed; a.bias = l.lnf ? l.c2 : l.b; a.c1 = l.c1;
    a.M = M; a.K = l.K; a.N = l.N; a.NT = l.NT; a.KS = l.KS;
    if (l.KS > 1) a.part_out = d->part;
    if (cand) { a.cand_val = d->cand_val; a.cand_idx = d->cand_idx; }
    const int mt = (M + PAD_ROWS - 1) / PAD_ROWS;
    // under autocast, more than one row tile: the 16-bit-weight kernels (one row tile - batch-1 greedy decoding - stays bit-exact fp32)
    const int w16 = (d->bf16_gemms && d->w16_fused && mt > 1 && l.packed16 && l.packed16_f16 == d->f16() && (!l.lnf || l.c1_16)) ? (d->f16() ? 2 : 1) : 0;
    if (w16) { a.P = reinterpret_cast<const float*>(l.packed16); if (l.lnf) a.c1 = l.c1_16; }
    const int rc = direct_dispatch(a, l.lnf, mode, w16, d->stream);
    if (rc) return rc;
    if (count) {
        d->gemm_bytes_per_step += (size_t)l.N * l.K * (w16 ? 2 : sizeof(float));
        d->gemm_flops_per_step += 2.0 * M * l.N * l.K;
        d->gemm_launches_per_step += 1;
    }
    return RGRG_OK;
}

// The GEMMs of layer l of the fused plan (everything but the attention); `cur` holds x_mid of the previous layer in
// fragment-major order with its mlp_proj partial sums pending in d->part, `nxt` receives this layer's residual stream.
static int enqueue_layer_gemms(rgrg_decoder* d, int l, const StepSpec& s, bool count, const float* cur, float* nxt,
                               int part) {  // part: 0 = c_attn', 1 = attn_proj' .. mlp_proj
    const LayerW& w = d->layers[l];
    const int D = d->D, S = s.rows;
    int rc;
    if (part == 0) {
        DirectArgs a{};
        a.xout = nxt; a.Y = d->qkv; a.ldy = 3 * D; a.act = RGRG_ACT_NONE;
        int mode;
        if (l == 0) {
            a.wte = d->wte; a.ids = d->ids; a.ld_ids = d->max_len; a.step = d->step; a.tok_override = s.tok;
            a.pos_override = s.row_pos;
            mode = s.tok ? (s.row_pos ? DX_EMBED_TOKPOS : DX_EMBED_TOK) : DX_EMBED;
        } else {
            a.Xf = cur; a.part = d->part;
            mode = DX_COMBINE4;
        }
        return direct_linear(d, w.c_attn, a, mode, S, count);
    }
    DirectArgs p{};  // attn_proj': x += att W^T + b, in place (every element is read and written by the same thread);
    p.Xf = d->att; p.Rf = nxt; p.Yf = nxt; p.act = RGRG_ACT_NONE;  // its epilogue also zeroes mlp_proj's accumulators
    p.zero_acc = d->part;
    if ((rc = direct_linear(d, w.attn_proj, p, DX_PLAIN, S, count))) return rc;
    DirectArgs f{};  // c_fc': gelu_new(ln_2(x) W^T + b)
    f.Xf = nxt; f.Yf = d->ff; f.act = RGRG_ACT_GELU_NEW;
    if ((rc = direct_linear(d, w.c_fc, f, DX_PLAIN, S, count))) return rc;
    DirectArgs m{};  // mlp_proj: 4 K slices accumulate pairwise into d->part (slice 0 carries the bias)
    m.Xf = d->ff; m.act = RGRG_ACT_NONE;
    return direct_linear(d, w.mlp_proj, m, DX_PLAIN, S, count);
}

// One decode step of the fused plan (<= 128 token rows): 24 * 5 + 2 = 122 launches
//   per layer: c_attn' [embedding | previous mlp_proj combine; ln_1 folded] -> attention -> attn_proj' [+ bias +
//   residual, in place] -> c_fc' [ln_2 folded, gelu] -> mlp_proj (4 partial sums)
//   lm_head' [combine; ln_f folded; arg-max candidates] -> argmax + bookkeeping.
// The residual stream ping-pongs between d->x and d->x2; x, att, ff and the partial sums are fragment-major.
static int enqueue_step_fused(rgrg_decoder* d, const StepSpec& s, bool count) {
    if (count) { d->gemm_bytes_per_step = 0; d->gemm_flops_per_step = 0.0; d->gemm_launches_per_step = 0; }
    hipStream_t st = d->stream;
    const int S = s.rows;
    const bool logits = s.end != STEP_ARGMAX && s.end != STEP_ROLL;
    int rc;
    float* cur = d->x;
    float* nxt = d->x2;
    for (int l = 0; l < d->n_layer; ++l) {
        if ((rc = enqueue_layer_gemms(d, l, s, count, cur, nxt, 0))) return rc;
        if ((rc = launch_attention(d, l, s, 0, S, nullptr, 1))) return rc;
        if ((rc = enqueue_layer_gemms(d, l, s, count, cur, nxt, 1))) return rc;
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    DirectArgs h{};
    h.Xf = cur; h.part = d->part; h.Y = d->logits; h.ldy = d->ld_logits; h.act = RGRG_ACT_NONE;
    if ((rc = direct_linear(d, d->lm_head, h, DX_COMBINE4, S, count, !logits))) return rc;
    if (logits) return RGRG_OK;
    if (s.end == STEP_ROLL) return enqueue_roll_end(d, S, d->lm_head.NT, s.roll_prompt);
    hipLaunchKernelGGL(argmax_update_kernel, dim3(S), dim3(256), 0, st, d->cand_val, d->cand_idx, d->lm_head.NT, d->ids,
                       d->max_len, d->finished, d->step, d->done_len, d->sync, S);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// The many-sequence 16-bit step as `chains` independent row ranges (whole 64-row tiles): fn(r0, rows) enqueues a range's work on
// d->stream; ranges 1.. run on forked streams (d->stream is swapped around the call) and are joined before this returns, so
// one range's attention (HBM bound) and launch boundaries overlap another range's GEMMs.  Works under stream capture (the step
// graph gets parallel branches) and eagerly.  chains < 0: the ranges one after the other on d->stream (A/B runs).
// the row ranges of a step: whole 64-row tiles, as even as possible, every range above the fused plan's row limit (fewer ranges
// otherwise); -> number of ranges, bounds[0 .. nr]
static int range_bounds(int S, int want, int (&bounds)[MAX_CHAINS + 1]) {
    int nr = want < 1 ? 1 : (want > MAX_CHAINS ? MAX_CHAINS : want);
    const int tiles = (S + 63) / 64;
    for (; nr > 1; --nr) {
        int least = S;
        for (int i = 0; i <= nr; ++i) {
            bounds[i] = std::min(S, ((tiles * i + nr - 1) / nr) * 64);
            if (i) least = std::min(least, bounds[i] - bounds[i - 1]);
        }
        if (least > SKINNY_MAX_ROWS) break;
    }
    if (nr <= 1) { nr = 1; bounds[0] = 0; bounds[1] = S; }
    return nr;
}
template <class F>
static int run_row_ranges(rgrg_decoder* d, int S, int chains, F&& fn) {
    int bounds[MAX_CHAINS + 1];
    // every range must stay on the many-sequence code path (> 128 rows: 16-bit cache, tiled GEMMs): fewer ranges otherwise
    const int nr = range_bounds(S, chains < 0 ? -chains : chains, bounds);
    if (nr <= 1) return fn(0, S);
    if (chains > 0) {
        RGRG_HIP(hipEventRecord(d->ev_fork, d->stream));
        for (int i = 1; i < nr; ++i) RGRG_HIP(hipStreamWaitEvent(d->streams_x[i - 1], d->ev_fork, 0));
    }
    int rc = RGRG_OK;
    for (int i = 0; i < nr && !rc; ++i) {
        if (bounds[i + 1] <= bounds[i]) continue;
        if (chains > 0 && i > 0) std::swap(d->stream, d->streams_x[i - 1]);
        rc = fn(bounds[i], bounds[i + 1] - bounds[i]);
        if (chains > 0 && i > 0) std::swap(d->stream, d->streams_x[i - 1]);
    }
    if (chains > 0)   // join even after an error: a forked stream must not be left inside a capture
        for (int i = 1; i < nr; ++i) {
            RGRG_HIP(hipEventRecord(d->ev_join[i - 1], d->streams_x[i - 1]));
            RGRG_HIP(hipStreamWaitEvent(d->stream, d->ev_join[i - 1], 0));
        }
    return rc;
}
// ... which steps run that way: greedy, LayerNorm-folded 16-bit mode, at least 512 sequences (RGRG_DECODE_CHAINS: 1 = off)
static int step_chains(const rgrg_decoder* d, int S, bool greedy, bool fold) {
    return (greedy && fold && S >= 512 && (d->chains < 0 || d->streams_x[0])) ? d->chains : 1;
}

// measurement only (rgrg_decoder_trace_step): an event on the current stream behind the launch just made.
// tag = layer * 8 + {0 c_attn, 1 attention, 2 attn_proj, 3 c_fc, 4 mlp_proj}; 1000 embedding, 1001 ln_f, 1002 lm_head, 1003 arg-max
static int trace_mark(rgrg_decoder* d, int r0, int tag) {
    if (!d->trace) return RGRG_OK;
    hipEvent_t e;
    RGRG_HIP(hipEventCreate(&e));
    RGRG_HIP(hipEventRecord(e, d->stream));
    d->trace->push_back({e, r0, tag});
    return RGRG_OK;
}

// The LayerNorm-folded 16-bit many-sequence step (see enqueue_step) ...
static bool step_ln_fold(const rgrg_decoder* d, int S) {
    return kv_is_bf16(d, S) && d->xn16 && d->ln_fold && d->ln_stat && d->layers[0].c_attn.wb_ln && d->D == 1024;
}
// ... whose c_attn writes the new token's k / v straight into slot t + 1 of the 16-bit cache and whose attention reads q only:
// plain steps (the step's own token and cache rows: greedy and sampling; not beam search, not forward(use_cache=True)) without a
// slot mask on the bf16 / fp16 cache (not e4m3), c_attn on the LDS-DMA kernel - the row-split kernel of RGRG_GEMM_KP=1/3 has no such
// epilogue and keeps the fp32 q | k | v row.  RGRG_QKV_CACHE=0: the fp32 row everywhere (A/B, tests/test_gpu_qkv_cache.py).
static bool step_qkv_cache(const rgrg_decoder* d, const StepSpec& s) {
    const int S = s.rows;
    const KvFormat f = kv_format(d, S);
    const bool plain = !s.tok && !s.src;
    return d->qkv_cache && plain && step_ln_fold(d, S) && (f == KV_BF16 || f == KV_F16) && d->kp_gemms != 1 && d->kp_gemms != 3 && !s.key_mask;
}
// the consumer fold of layer l's c_attn for the sequences from r0 on, with the cache planes launch_attention passes for them
static GemmLnFold cons_kv_cache(const rgrg_decoder* d, const GemmLnFold& cons, int l, int r0) {
    GemmLnFold f = cons;
    u16* kcr = reinterpret_cast<u16*>(d->kv) + (size_t)l * d->kv_layer_stride + (size_t)r0 * d->H * d->T * 64;
    f.kv_k = kcr; f.kv_v = kcr + d->kv_kv_stride; f.kv_step = d->step; f.kv_H = d->H; f.kv_T = d->T;
    return f;
}

// The end of a step: lm_head over the ln_f rows (d->xn, or xn16 where the step's GEMMs read 16-bit activations).  logits: d->logits
// and nothing else (the sampler or a ranking follows); otherwise per-tile arg-max candidates, arg-max and the bookkeeping - of the
// greedy loop, or (roll) of rolling-batch decoding, from the same candidates.
static int enqueue_head(rgrg_decoder* d, int S, bool count, bool logits, unsigned short* xn16, bool roll = false, bool roll_prompt = false) {
    hipStream_t st = d->stream;
    int rc;
    if (!logits && xn16 && lm_head_cand_path(d, S)) {
        // greedy: the 256 x 256 lm_head leaves one (maximum, column) pair per row and column tile; no logits, no candidates pass
        GemmLnFold ce{};
        ce.cand_val = d->cand_val; ce.cand_idx = d->cand_idx;
        if ((rc = linear(d, d->lm_head, d->xn, nullptr, nullptr, S, d->ld_logits, RGRG_ACT_NONE, count, xn16, nullptr, &ce))) return rc;
        if ((rc = trace_mark(d, 0, 1002))) return rc;
        if (roll) return enqueue_roll_end(d, S, (d->lm_head.N + 255) / 256, roll_prompt);
        hipLaunchKernelGGL(argmax_update_kernel, dim3(S), dim3(256), 0, st, d->cand_val, d->cand_idx, (d->lm_head.N + 255) / 256, d->ids,
                           d->max_len, d->finished, d->step, d->done_len, d->sync, S);
        RGRG_LAUNCH_CHECK();
        return trace_mark(d, 0, 1003);
    }
    if ((rc = linear(d, d->lm_head, d->xn, nullptr, d->logits, S, d->ld_logits, RGRG_ACT_NONE, count, xn16))) return rc;
    if (logits) return RGRG_OK;
    const int cand_nt = (d->V + 31) / 32;  // ld_logits >= 32 * cand_nt, and the candidate buffers hold lm_head.NT >= cand_nt per row
    hipLaunchKernelGGL(logits_candidates_kernel, dim3(4, S), dim3(256), 0, st, d->logits, d->ld_logits, d->V,
                       cand_nt, d->cand_val, d->cand_idx);
    RGRG_LAUNCH_CHECK();
    if (roll) return enqueue_roll_end(d, S, cand_nt, roll_prompt);
    hipLaunchKernelGGL(argmax_update_kernel, dim3(S), dim3(256), 0, st, d->cand_val, d->cand_idx, cand_nt, d->ids,
                       d->max_len, d->finished, d->step, d->done_len, d->sync, S);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
int enqueue_head_argmax(rgrg_decoder* d, int S) {
    return enqueue_head(d, S, false, false, (kv_is_bf16(d, S) && d->xn16) ? d->xn16 : nullptr);
}
int enqueue_head_logits(rgrg_decoder* d, int S) {
    return enqueue_head(d, S, false, true, (kv_is_bf16(d, S) && d->xn16) ? d->xn16 : nullptr);
}

// Beam search behind a left-padded prompt, fp32 cache: the additive mask of every cache slot of every beam row, -1e4 on slots
// 1 .. first[r] (the padding of the row's item) and 0 elsewhere.  Padding belongs to the item and a parent lies inside the item, so
// the rows never move with the ancestor table.
__global__ __launch_bounds__(256) void beam_first_mask_kernel(const int* __restrict__ first, int R, int T, float* __restrict__ kmask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * T) return;
    const int r = i / T, j = i - r * T;
    kmask[i] = (j >= 1 && j <= first[r]) ? -10000.0f : 0.f;
}
int launch_beam_first_mask(const int* first, int R, int T, float* kmask, hipStream_t st) {
    hipLaunchKernelGGL(beam_first_mask_kernel, dim3((R * T + 255) / 256), dim3(256), 0, st, first, R, T, kmask);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// The decode step of more token rows than the fused plan takes (many images, beam rows): tiled MFMA GEMMs
//   embed+ln1 | per layer: c_attn, attention, attn_proj (+ residual), ln2, c_fc+gelu, mlp_proj (+ residual),
//   ln1 of the next layer / ln_f | lm_head, per-32-column arg-max candidates, argmax + bookkeeping
static int enqueue_step_tiled(rgrg_decoder* d, const StepSpec& s, bool count) {
    const int S = s.rows;
    if (count) { d->gemm_bytes_per_step = 0; d->gemm_flops_per_step = 0.0; d->gemm_launches_per_step = 0; }
    d->step_rows = S;
    const int D = d->D;
    int rc;
    // bf16 many-sequence mode: the GEMM inputs (LayerNorm output, attention output, GELU output) are written ONCE as
    // bf16 by their producers - the same round-to-nearest-even the GEMM would apply to an fp32 input, so the results
    // do not change - instead of fp32 that every column tile of the GEMM re-reads and re-rounds
    unsigned short* xn16 = (kv_is_bf16(d, S) && d->xn16) ? d->xn16 : nullptr;
    unsigned short* att16 = xn16 ? d->att16 : nullptr;
    unsigned short* ff16 = xn16 ? d->ff16 : nullptr;
    // ... and the LayerNorms between the GEMMs are FOLDED into them (no launch of their own): the GEMMs that write the
    // residual stream x (attn_proj, mlp_proj; the embedding for layer 0) also leave x as 16 bit in xn16 and per-row
    // (sum, sum of squares) slots in ln_stat; the GEMM behind the LayerNorm (c_attn, c_fc) multiplies the raw 16-bit x with
    // gain-scaled weights and finishes rstd (acc - mean colsum) + shift in its epilogue (gemm_bf16.hip).  ln_f in front of
    // the lm_head stays a launch: the slot reads cost its 3144 workgroups more than the one ln_rows per step
    const bool fold = step_ln_fold(d, S);
    // ... and c_attn's k / v columns go straight to cache slot t + 1 as 16 bit; the attention then reads q only (step_qkv_cache)
    const bool qc = step_qkv_cache(d, s);
    static const float cons_tag = 0.f;   // any non-null pointer: linear() substitutes the GEMM's own column sums
    GemmLnFold prod{}, cons{};
    prod.Yb16 = xn16; prod.stats_out = d->ln_stat;
    cons.ln_stats = d->ln_stat; cons.ln_colsum = &cons_tag;
    const GemmLnFold* pf = fold ? &prod : nullptr;
    const GemmLnFold* cf = fold ? &cons : nullptr;
    // Embedding .. last LayerNorm for the sequences [r0, r0 + rows) on d->stream.  Every kernel of the chain is row-local (a
    // sequence's token, residual stream, cache rows and LayerNorm slots), so a step can run as independent row ranges.
    auto run_rows = [&](int r0, int rows) -> int {
        hipStream_t rs = d->stream;
        const size_t o = (size_t)r0 * D;
        float* x = d->x + o; float* xn = d->xn + o;
        unsigned short* xn16r = xn16 ? xn16 + o : nullptr;
        unsigned short* att16r = att16 ? att16 + o : nullptr;
        unsigned short* ff16r = ff16 ? ff16 + 4 * o : nullptr;
        float* statr = d->ln_stat ? d->ln_stat + (size_t)r0 * 32 : nullptr;
        GemmLnFold prod_r = prod, cons_r = cons;
        prod_r.Yb16 = xn16r; prod_r.stats_out = statr; cons_r.ln_stats = statr;
        const GemmLnFold* pfr = fold ? &prod_r : nullptr;
        const GemmLnFold* cfr = fold ? &cons_r : nullptr;
        int rc2;
        if ((rc2 = launch_embed_ln(d->wte, d->ids + (size_t)r0 * d->max_len, d->max_len, d->step, d->layers[0].ln1_g, d->layers[0].ln1_b, x, xn,
                                   D, s.tok ? s.tok + r0 : nullptr, xn16r, d->f16(), s.row_pos ? s.row_pos + r0 : nullptr,
                                   fold ? statr : (float*)nullptr, rows, rs)))
            return rc2;
        if ((rc2 = trace_mark(d, r0, 1000))) return rc2;
        for (int l = 0; l < d->n_layer; ++l) {
            const LayerW& w = d->layers[l];
            const float* ng = (l + 1 < d->n_layer) ? d->layers[l + 1].ln1_g : d->lnf_g;
            const float* nb = (l + 1 < d->n_layer) ? d->layers[l + 1].ln1_b : d->lnf_b;
            const GemmLnFold cons_kv = qc ? cons_kv_cache(d, cons_r, l, r0) : cons_r;
            if ((rc2 = linear(d, w.c_attn, xn, nullptr, d->qkv + 3 * o, rows, 3 * D, RGRG_ACT_NONE, count, xn16r, nullptr, qc ? &cons_kv : cfr))) return rc2;
            if ((rc2 = trace_mark(d, r0, l * 8 + 0))) return rc2;
            if ((rc2 = launch_attention(d, l, s, r0, rows, att16r, 0, qc))) return rc2;
            if ((rc2 = trace_mark(d, r0, l * 8 + 1))) return rc2;
            if ((rc2 = linear(d, w.attn_proj, d->att + o, x, x, rows, D, RGRG_ACT_NONE, count, att16r, nullptr, pfr))) return rc2;
            if ((rc2 = trace_mark(d, r0, l * 8 + 2))) return rc2;
            if (!fold) {
                if ((rc2 = launch_ln_rows(x, w.ln2_g, w.ln2_b, xn, D, xn16r, d->f16(), rows, rs))) return rc2;
            }
            if ((rc2 = linear(d, w.c_fc, xn, nullptr, d->ff + 4 * o, rows, 4 * D, RGRG_ACT_GELU_NEW, count, xn16r, ff16r, cfr))) return rc2;
            if ((rc2 = trace_mark(d, r0, l * 8 + 3))) return rc2;
            if ((rc2 = linear(d, w.mlp_proj, d->ff + 4 * o, x, x, rows, D, RGRG_ACT_NONE, count, ff16r, nullptr, pfr))) return rc2;
            if ((rc2 = trace_mark(d, r0, l * 8 + 4))) return rc2;
            if (!fold || l + 1 == d->n_layer) {
                if ((rc2 = launch_ln_rows(x, ng, nb, xn, D, xn16r, d->f16(), rows, rs))) return rc2;
                if ((rc2 = trace_mark(d, r0, 1001))) return rc2;
            }
        }
        return RGRG_OK;
    };
    if ((rc = run_row_ranges(d, S, step_chains(d, S, s.end == STEP_ARGMAX && !s.tok && !s.src, fold), run_rows))) return rc;
    return enqueue_head(d, S, count, s.end != STEP_ARGMAX && s.end != STEP_ROLL, xn16, s.end == STEP_ROLL, s.roll_prompt);
}
// One decode step: the fused plan up to its row limit (128 token rows; 64 under autocast), the tiled plan above
int enqueue_step(rgrg_decoder* d, const StepSpec& s, bool count) {
    const int rc = s.rows <= decode_row_limit(d) ? enqueue_step_fused(d, s, count) : enqueue_step_tiled(d, s, count);
    if (rc) return rc;
    if (s.end == STEP_SAMPLE) return enqueue_sampler(d, s.rows);
    return s.end == STEP_ROLL_SAMPLE ? enqueue_roll_sample_end(d, s.rows, s.roll_prompt) : RGRG_OK;
}

StepSpec padded_step_spec(rgrg_decoder* d, StepSpec s, const int* pad) {
    s.row_pos = d->row_pos;
    if (kv_format(d, s.rows) != KV_F32) s.kv_first = pad;
    else s.key_mask = d->key_mask;
    return s;
}

int enqueue_prefill(rgrg_decoder* d, const float* feats, int S, int row_mul) {
    hipStream_t st = d->stream;
    const int D = d->D;
    int rc;
    if ((rc = launch_decode_reset(d->ids, d->max_len, d->finished, d->step, d->done_len, d->sync, S, d->max_len, st))) return rc;
    RGRG_HIP(hipMemcpyAsync(d->feats, feats, (size_t)S * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    // feature_space_transformation_nn (:284) - needed once: only step 0 consumes it (:135-157)
    if ((rc = linear(d, d->fst0, d->feats, nullptr, d->h1, S, D, RGRG_ACT_RELU, false))) return rc;
    if ((rc = linear(d, d->fst2, d->h1, nullptr, d->img, S, D, RGRG_ACT_NONE, false))) return rc;
    // uk / uv of all layers in one GEMM, then scatter to cache slot 0
    if ((rc = linear(d, d->ukv, d->img, nullptr, d->ukv_out, S, d->ld_ukv, RGRG_ACT_NONE, false))) return rc;
    // the 16-bit / e4m3 cache lives in the same allocation with the same ELEMENT strides (half / a quarter of the bytes used)
    const KvFormat fmt = kv_format(d, S * row_mul);
    return launch_kv_slot0(d->ukv_out, d->ld_ukv, d->kv, d->kv_layer_stride, d->kv_kv_stride, S, d->H, d->T, d->n_layer, row_mul, fmt,
                           d->f16(), st);
}

}  // namespace rgrg

using namespace rgrg;

extern "C" size_t rgrg_decoder_kv_cache_bytes(int n_layer, int max_seqs, int max_len) {
    return (size_t)n_layer * 2 * (size_t)max_seqs * 16 * (size_t)(max_len + 1) * 64 * sizeof(float);
}

extern "C" int rgrg_decoder_create(const rgrg_decoder_weights* w, int max_seqs, int max_len, rgrg_decoder** out) {
    return rgrg_decoder_create_with_cache(w, max_seqs, max_len, nullptr, 0, out);
}

extern "C" int rgrg_decoder_create_with_cache(const rgrg_decoder_weights* w, int max_seqs, int max_len, void* kv_cache, size_t kv_cache_bytes,
                                              rgrg_decoder** out) {
    RGRG_CHECK_ARG(w && out && max_seqs > 0 && max_seqs < 65536 && max_len >= 2 && max_len <= 1024);  // 16-bit row tickets (argmax_update_kernel)
    RGRG_CHECK_ARG(w->d_model == 1024 && w->n_head == 16 && w->n_layer > 0 && w->vocab > 0 && w->layers);
    int rc = init_gemm_attrs();
    if (rc) return rc;
    if ((rc = init_skinny_attrs())) return rc;
    // The weights are packed below on the decoder's own non-blocking stream, and this entry point has no stream argument:
    // wait for whatever is still producing them on the caller's streams (creation is rare and allocates GBs anyway).
    RGRG_HIP(hipDeviceSynchronize());
    rgrg_decoder* d = new rgrg_decoder();
    d->n_layer = w->n_layer; d->D = w->d_model; d->H = w->n_head; d->V = w->vocab;
    d->max_seqs = max_seqs; d->max_len = max_len; d->T = max_len + 1;
    d->rows = ((max_seqs + PAD_ROWS - 1) / PAD_ROWS) * PAD_ROWS;
    d->wte = w->wte; d->lnf_g = w->lnf_g; d->lnf_b = w->lnf_b;
    const int D = d->D;
#define TRY(x) do { rc = (x); if (rc) { rgrg_decoder_destroy(d); return rc; } } while (0)
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_in, hipEventDisableTiming) != hipSuccess) {
        set_error("decoder: stream/event creation failed");
        delete d;
        return RGRG_EHIP;
    }
    if (const char* e = getenv("RGRG_GEMM_KP")) d->kp_gemms = atoi(e);
    if (const char* e = getenv("RGRG_W16_FUSED")) d->w16_fused = atoi(e) != 0;
    if (const char* e = getenv("RGRG_QKV_CACHE")) d->qkv_cache = atoi(e) != 0;
    if (const char* e = getenv("RGRG_DECODE_CHAINS")) {
        const int v = atoi(e);
        d->chains = (v >= -MAX_CHAINS && v <= MAX_CHAINS && v != 0 && v != -1) ? v : 1;
    }
    if (d->chains > 1) {
        bool ok = hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < d->chains - 1; ++i)
            ok = hipStreamCreateWithFlags(&d->streams_x[i], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&d->ev_join[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            set_error("decoder: stream/event creation failed");
            rgrg_decoder_destroy(d);
            return RGRG_EHIP;
        }
    }
    if (hipHostMalloc((void**)&d->h_id_error, sizeof(int), 0) == hipSuccess) *d->h_id_error = 0;
    if (hipHostMalloc((void**)&d->h_done, 3 * sizeof(int), 0) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_poll[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_poll[1], hipEventDisableTiming) != hipSuccess) {
        set_error("decoder: hipHostMalloc failed");
        delete d;
        return RGRG_EHIP;
    }
    TRY(make_lin(d, d->fst0, w->fst0_w, w->fst0_b, D, D, true));
    TRY(make_lin(d, d->fst2, w->fst2_w, w->fst2_b, D, D, true));
    TRY(make_lin(d, d->ukv, w->ukv_w, w->ukv_b, w->n_layer * 2 * D, D, true));
    TRY(make_lin(d, d->lm_head, w->wte, nullptr, w->vocab, D, true, true, w->lnf_g, w->lnf_b));
    d->layers.resize(w->n_layer);
    for (int l = 0; l < w->n_layer; ++l) {
        const rgrg_decoder_layer_weights& s = w->layers[l];
        LayerW& t = d->layers[l];
        t.ln1_g = s.ln1_g; t.ln1_b = s.ln1_b; t.ln2_g = s.ln2_g; t.ln2_b = s.ln2_b;
        TRY(make_lin(d, t.c_attn, s.c_attn_w, s.c_attn_b, 3 * D, D, true, true, s.ln1_g, s.ln1_b));
        TRY(make_lin(d, t.attn_proj, s.attn_proj_w, s.attn_proj_b, D, D, true, true));
        TRY(make_lin(d, t.c_fc, s.c_fc_w, s.c_fc_b, 4 * D, D, true, true, s.ln2_g, s.ln2_b));
        TRY(make_lin(d, t.mlp_proj, s.mlp_proj_w, s.mlp_proj_b, D, 4 * D, true, true));
    }
    const size_t R = d->rows;
    d->ld_logits = d->lm_head.NT * d->lm_head.ntile;
    d->ld_ukv = d->ukv.N;
    TRY(dmalloc(d, (void**)&d->feats, R * D * 4, true));
    TRY(dmalloc(d, (void**)&d->h1, R * D * 4, true));
    TRY(dmalloc(d, (void**)&d->img, R * D * 4, true));
    TRY(dmalloc(d, (void**)&d->ukv_out, R * d->ld_ukv * 4, true));
    TRY(dmalloc(d, (void**)&d->x, R * D * 4, true));
    TRY(dmalloc(d, (void**)&d->x2, R * D * 4, true));
    TRY(dmalloc(d, (void**)&d->xn, R * D * 4, true));
    TRY(dmalloc(d, (void**)&d->qkv, R * 3 * D * 4, true));
    TRY(dmalloc(d, (void**)&d->att, R * D * 4, true));
    TRY(dmalloc(d, (void**)&d->ff, R * 4 * D * 4, true));
    TRY(dmalloc(d, (void**)&d->logits, R * d->ld_logits * 4, true));
    TRY(dmalloc(d, (void**)&d->part, (size_t)(SKINNY_MAX_ROWS / PAD_ROWS) * 8 * PAD_ROWS * D * 4, true));  // [tiles<=4][KS<=8][32][N=1024]
    d->kv_kv_stride = (size_t)d->max_seqs * d->H * d->T * 64;
    d->kv_layer_stride = 2 * d->kv_kv_stride;
    if (kv_cache) {   // caller-owned (zero-filled) cache: never freed here
        if (kv_cache_bytes < (size_t)d->n_layer * d->kv_layer_stride * 4) {
            set_error("decoder: the caller's K/V cache holds %zu bytes, %zu needed", kv_cache_bytes, (size_t)d->n_layer * d->kv_layer_stride * 4);
            rgrg_decoder_destroy(d);
            return RGRG_EINVAL;
        }
        d->kv = static_cast<float*>(kv_cache);
    } else {
        TRY(dmalloc(d, (void**)&d->kv, (size_t)d->n_layer * d->kv_layer_stride * 4, true));
    }
    TRY(dmalloc(d, (void**)&d->ids, R * max_len * sizeof(long long), true));
    TRY(dmalloc(d, (void**)&d->next, R * 4, true));
    TRY(dmalloc(d, (void**)&d->finished, R * 4, true));
    TRY(dmalloc(d, (void**)&d->step, 4, true));
    TRY(dmalloc(d, (void**)&d->done_len, 4, true));
    TRY(dmalloc(d, (void**)&d->sync, 64, true));
    TRY(dmalloc(d, (void**)&d->id_error, 8, true));
    TRY(dmalloc(d, (void**)&d->cand_val, R * d->lm_head.NT * 4, true));
    TRY(dmalloc(d, (void**)&d->cand_idx, R * d->lm_head.NT * 4, true));
    TRY(dmalloc(d, (void**)&d->src_a, R * d->T * 4, true));
    TRY(dmalloc(d, (void**)&d->src_b, R * d->T * 4, true));
    TRY(dmalloc(d, (void**)&d->beam_tok, R * 4, true));
    TRY(dmalloc(d, (void**)&d->row_pos, R * 4, true));
    TRY(dmalloc(d, (void**)&d->beam_parent, R * 4, true));
    TRY(dmalloc(d, (void**)&d->beam_scores, R * 4, true));
    TRY(dmalloc(d, (void**)&d->row_max, R * 4, true));
    TRY(dmalloc(d, (void**)&d->row_logsum, R * 4, true));
    TRY(dmalloc(d, (void**)&d->top_val, R * BEAM_K * 4, true));
    TRY(dmalloc(d, (void**)&d->top_tok, R * BEAM_K * 4, true));
    TRY(dmalloc(d, (void**)&d->cand_score, R * BEAM_K * 4, true));
    TRY(dmalloc(d, (void**)&d->cand_tok, R * BEAM_K * 4, true));
    TRY(dmalloc(d, (void**)&d->cand_beam, R * BEAM_K * 4, true));
    d->gemm_ws_floats = (d->max_seqs > 32) ? (size_t)16 * R * 4 * D : 0;  // split-K partials of the tiled GEMM
    d->gemm_ws = nullptr;
    if (d->gemm_ws_floats) TRY(dmalloc(d, (void**)&d->gemm_ws, d->gemm_ws_floats * 4, false));
#undef TRY
    // packing (decoder stream) and the zero fills (null stream) are complete before the first use
    if (hipDeviceSynchronize() != hipSuccess) {
        set_error("decoder: weight packing failed");
        rgrg_decoder_destroy(d);
        return RGRG_EHIP;
    }
    *out = d;
    return RGRG_OK;
}

extern "C" void rgrg_decoder_destroy(rgrg_decoder* d) {
    if (!d) return;
    for (auto& g : d->graphs) (void)hipGraphExecDestroy(g.exec);
    for (void* p : d->allocs) (void)hipFree(p);
    d->tf.free();
    d->tr.free();
    if (d->tr.a16_scratch) (void)hipFree(d->tr.a16_scratch);
    if (d->roll.ukv) (void)hipFree(d->roll.ukv);
    roll_session_free(d);
    if (d->h_done) (void)hipHostFree(d->h_done);
    for (hipEvent_t e : d->ev_poll)
        if (e) (void)hipEventDestroy(e);
    if (d->h_id_error) (void)hipHostFree(d->h_id_error);
    if (d->ev_in) (void)hipEventDestroy(d->ev_in);
    if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
    for (int i = 0; i < MAX_CHAINS - 1; ++i) {
        if (d->ev_join[i]) (void)hipEventDestroy(d->ev_join[i]);
        if (d->streams_x[i]) (void)hipStreamDestroy(d->streams_x[i]);
    }
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

namespace rgrg {
// The decode loop that greedy search and sampling share.  decode_begin: d->stream waits for the caller's stream.
// run_decode_loop: prefill, then `step` (a decode step ending in a kernel that calls record_step_token, `prepare` in front of it)
// limit - 1 times - replayed from its graph when use_graph -, the polling below, and the copies of ids [S, limit] (and of the
// sampler's log-probs, d->sample_lp, when out_logprobs is given) before the one synchronise; *out_len as rgrg_decoder_generate
// documents it.
int decode_begin(rgrg_decoder* d, void* stream) {
    RGRG_HIP(hipEventRecord(d->ev_in, as_stream(stream)));
    RGRG_HIP(hipStreamWaitEvent(d->stream, d->ev_in, 0));
    d->logits_valid = false;   // until the call has completed (an early error return leaves no logits to copy)
    ++d->epoch;                // an open rolling session is stale from here on
    return RGRG_OK;
}
int step_graph(rgrg_decoder* d, const StepSpec& s, const std::function<int()>& body, hipGraphExec_t* exec) {
    for (auto& g : d->graphs)
        if (g.spec == s) { *exec = g.exec; return RGRG_OK; }
    hipGraph_t graph = nullptr;
    RGRG_HIP(hipStreamBeginCapture(d->stream, hipStreamCaptureModeThreadLocal));
    const int rc = body();
    hipError_t e = hipStreamEndCapture(d->stream, &graph);   // also behind a failed step: the stream must not stay in capture mode
    if (rc) return rc;
    if (e != hipSuccess) { set_error("%shipStreamEndCapture: %s", (s.end == STEP_BEAM || s.end == STEP_BEAM_SAMPLE) ? "beam: " : "", hipGetErrorString(e)); return RGRG_EHIP; }
    RGRG_HIP(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    d->graphs.push_back({s, *exec});
    return RGRG_OK;
}
int run_decode_loop(rgrg_decoder* d, const float* feats, const StepSpec& step, int (*prepare)(rgrg_decoder*, int S), int limit,
                    int use_graph, int64_t* out_ids, int out_ld, float* out_logprobs, int* out_len, const DecodePrologue* prologue) {
    const int S = step.rows;
    int rc = enqueue_prefill(d, feats, S);
    if (rc) return rc;
    if (prologue && (rc = prologue->fn(d, S, prologue->arg))) return rc;

    auto enqueue = [&](bool count) -> int {
        const int r = prepare ? prepare(d, S) : RGRG_OK;
        return r ? r : enqueue_step(d, step, count);
    };
    hipGraphExec_t exec = nullptr;
    if (use_graph && (rc = step_graph(d, step, [&] { return enqueue(true); }, &exec))) return rc;
    const int steps = limit - 1 - (prologue ? prologue->steps_done : 0);
    int done = 0;
    // "every row has emitted EOS" is polled WITHOUT draining the pipeline: every 16 steps the device-side length word is
    // copied to a pinned slot behind the step that produced it, and the host then waits for the copy it queued 16 steps
    // EARLIER - so 16 steps are always queued behind the one it waits for (round 2 synchronised the stream here: a
    // bubble of an idle GPU + a relaunch every 16 steps), and the host never runs more than 32 steps ahead; after the
    // last row finishes at most 32 more steps run, which only write PAD behind the recorded length.
    int polls = 0;
    d->h_done[1] = d->h_done[2] = 0;
    for (int t = 0; t < steps; ++t) {
        if (exec) {
            RGRG_HIP(hipGraphLaunch(exec, d->stream));
        } else {
            rc = enqueue(t == 0);
            if (rc) return rc;
        }
        if ((t & 15) == 15 && t + 1 < steps) {
            if (polls > 0) {
                const int prev = (polls - 1) & 1;
                RGRG_HIP(hipEventSynchronize(d->ev_poll[prev]));
                if (d->h_done[1 + prev]) break;
            }
            const int cur = polls & 1;
            RGRG_HIP(hipMemcpyAsync(d->h_done + 1 + cur, d->done_len, sizeof(int), hipMemcpyDeviceToHost, d->stream));
            RGRG_HIP(hipEventRecord(d->ev_poll[cur], d->stream));
            ++polls;
        }
    }
    RGRG_HIP(hipMemcpyAsync(d->h_done, d->done_len, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    RGRG_HIP(hipMemcpy2DAsync(out_ids, (size_t)out_ld * sizeof(int64_t), d->ids, (size_t)d->max_len * sizeof(long long),
                              (size_t)limit * sizeof(int64_t), S, hipMemcpyDeviceToDevice, d->stream));
    if (out_logprobs)
        RGRG_HIP(hipMemcpy2DAsync(out_logprobs, (size_t)out_ld * sizeof(float), d->sample_lp, (size_t)d->max_len * sizeof(float),
                                  (size_t)limit * sizeof(float), S, hipMemcpyDeviceToDevice, d->stream));
    RGRG_HIP(hipStreamSynchronize(d->stream));
    done = *d->h_done;
    *out_len = (done > 0 && done < limit) ? done : limit;
    d->logits_valid = true;
    return RGRG_OK;
}
}  // namespace rgrg

extern "C" int rgrg_decoder_generate(rgrg_decoder* d, const float* feats, int S, int max_length, int64_t* out_ids,
                                     int out_ld, int* out_len, int use_graph, void* stream) {
    RGRG_CHECK_ARG(d && feats && out_ids && out_len && S > 0 && S <= d->max_seqs);
    int limit = (max_length > 0) ? max_length : d->max_len;
    RGRG_CHECK_ARG(limit >= 2 && limit <= d->max_len && out_ld >= limit);
    int rc = decode_begin(d, stream);
    if (rc) return rc;
    const StepSpec step{S};
    if ((rc = run_decode_loop(d, feats, step, nullptr, limit, use_graph, out_ids, out_ld, nullptr, out_len))) return rc;
    d->logits_stale_rows = lm_head_cand_path(d, S) ? S : 0;
    return RGRG_OK;
}

namespace rgrg {
// forward(use_cache=True): attention_mask [S][L] over the L = past_len + T token keys -> additive mask of the cache slots,
// slot 0 (the image key) never masked (language_model.py:316-334: a ones column is concatenated in front)
__global__ __launch_bounds__(256) void key_mask_kernel(const float* __restrict__ am, int L, int S, int T, float* __restrict__ kmask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * T) return;
    const int s = i / T, j = i - s * T;
    kmask[i] = (j >= 1 && j <= L) ? (1.0f - am[(size_t)s * L + (j - 1)]) * -10000.0f : 0.f;
}
__global__ void set_int_kernel(int* p, int v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *p = v;
}
// incremental forward: the tokens of input position j (clamped into the vocabulary) -> the step's token-override buffer,
// and the step counter = the position (cache slot position + 1, embedding row wte[position])
__global__ __launch_bounds__(256) void forward_cached_tokens_kernel(const long long* __restrict__ ids, const long long* __restrict__ pos_ids,
                                                                    int T, int j, int S, int V, int* __restrict__ tok,
                                                                    int* __restrict__ row_pos, int* __restrict__ step, int position) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < S) {
        const long long t = ids[(size_t)s * T + j];
        tok[s] = (int)(t < 0 ? 0 : (t >= V ? V - 1 : t));   // (the host mirror rejects ids / positions outside the table beforehand)
        if (pos_ids) {
            const long long q = pos_ids[(size_t)s * T + j];
            row_pos[s] = (int)(q < 0 ? 0 : (q >= V ? V - 1 : q));
        }
    }
    if (s == 0) *step = position;
}
static int launch_key_mask(const float* am, int L, int S, int T, float* kmask, hipStream_t st) {
    hipLaunchKernelGGL(key_mask_kernel, dim3((S * T + 255) / 256), dim3(256), 0, st, am, L, S, T, kmask);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
static int launch_forward_cached_tokens(const long long* ids, const long long* pos_ids, int T, int j, int S, int V, int* tok, int* row_pos,
                                        int* step, int position, hipStream_t st) {
    hipLaunchKernelGGL(forward_cached_tokens_kernel, dim3((S + 255) / 256), dim3(256), 0, st, ids, pos_ids, T, j, S, V, tok, row_pos, step,
                       position);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
}  // namespace rgrg

// LanguageModel.forward(input_ids, ..., past_key_values, use_cache=True) (language_model.py:258-366, :396-399): the
// incremental form the reference's own generate loop is built on, over THIS decoder's K/V cache.  past_len == 0: the image
// key / value is computed from feats and stored in slot 0 (past_key_values=None, :135-157); then the T tokens of every row
// are fed one position at a time (position = past_len + j; wte[token] + wte[position], :298-307), each appending its
// key / value to the cache; logits_out [S, T, vocab] receives lm_head of every fed position.  No arg-max, no EOS bookkeeping.
extern "C" int rgrg_decoder_forward_cached(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const int64_t* position_ids,
                                           const float* attention_mask, int S, int T, int past_len, float* logits_out, void* stream) {
    RGRG_CHECK_ARG(d && input_ids && logits_out && S > 0 && S <= d->max_seqs && T >= 1 && past_len >= 0);
    // feats == NULL with past_len == 0: the caller put a past that holds ONLY the image slot into the cache (a foreign
    // past_key_values of shape [.., 1, 64], language_model.py:162-166 uses the supplied past and ignores the image then)
    RGRG_CHECK_ARG(past_len == 0 || feats == nullptr);
    RGRG_CHECK_ARG(past_len + T <= d->max_len);   // slot of the last token = past_len + T <= T_cache - 1
    // The padding mask exists only in the fp32 attention kernel: in a 16-bit mode above the row limit the step reads the 16-bit
    // cache with attn_decode_kv16_wave_kernel, which has no mask operand - refuse, rather than return unmasked logits
    if (attention_mask && kv_is_bf16(d, S)) {
        set_error("rgrg_decoder_forward_cached: attention_mask is not supported in precision mode %d for %d sequences (more than the "
                  "%d rows of the fp32-cache path): call rgrg_decoder_set_precision(d, 0) first", d->bf16_gemms, S, decode_row_limit(d));
        return RGRG_EINVAL;
    }
    hipStream_t caller = as_stream(stream), st = d->stream;
    ++d->epoch;   // the cache rows are rewritten: an open rolling session is stale
    RGRG_HIP(hipEventRecord(d->ev_in, caller));
    RGRG_HIP(hipStreamWaitEvent(st, d->ev_in, 0));
    int rc;
    d->logits_stale_rows = 0;   // every step below writes d->logits
    d->logits_valid = false;
    if (past_len == 0 && feats && (rc = enqueue_prefill(d, feats, S))) return rc;   // also resets the step counter to 0
    if (attention_mask) {   // [S][past_len + T]: padding inside the prompt / the past -> additive mask per cache slot
        if (!d->key_mask && (rc = dmalloc(d, (void**)&d->key_mask, (size_t)d->rows * d->T * sizeof(float), true))) return rc;
        if ((rc = launch_key_mask(attention_mask, past_len + T, S, d->T, d->key_mask, st))) return rc;
    }
    StepSpec step;   // ... lm_head: logits, nothing else
    step.rows = S; step.tok = d->beam_tok; step.end = STEP_LOGITS;
    step.row_pos = position_ids ? d->row_pos : nullptr;   // embedding rows wte[position_ids[s][j]]; the cache slot stays past_len + j + 1
    step.key_mask = attention_mask ? d->key_mask : nullptr;
    for (int j = 0; j < T; ++j) {
        if ((rc = launch_forward_cached_tokens(reinterpret_cast<const long long*>(input_ids), reinterpret_cast<const long long*>(position_ids), T,
                                               j, S, d->V, d->beam_tok, d->row_pos, d->step, past_len + j, st)))
            return rc;
        if ((rc = enqueue_step(d, step, false))) return rc;
        RGRG_HIP(hipMemcpy2DAsync(logits_out + (size_t)j * d->V, (size_t)T * d->V * sizeof(float), d->logits,
                                  (size_t)d->ld_logits * sizeof(float), (size_t)d->V * sizeof(float), S, hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, st, d->step, past_len + T);
    RGRG_LAUNCH_CHECK();
    RGRG_HIP(hipEventRecord(d->ev_in, st));
    RGRG_HIP(hipStreamWaitEvent(caller, d->ev_in, 0));
    d->logits_valid = true;
    return RGRG_OK;
}

// Where the cache of layer `layer` lives: K (kv = 0) or V (kv = 1) plane [max_seqs][16][max_len + 1][64] fp32 (bf16 in the
// opt-in many-sequence mode: *is_bf16); slots 0 .. past_len of a row are valid.  The host wraps these as the `presents`
// views forward(use_cache=True) returns - no copy.
extern "C" int rgrg_decoder_cache_plane(rgrg_decoder* d, int layer, int kv, void** ptr, int* max_seqs, int* slots, int* is_bf16) {
    RGRG_CHECK_ARG(d && ptr && layer >= 0 && layer < d->n_layer && (kv == 0 || kv == 1));
    *ptr = d->kv + (size_t)layer * d->kv_layer_stride + (size_t)kv * d->kv_kv_stride;
    if (max_seqs) *max_seqs = d->max_seqs;
    if (slots) *slots = d->T;
    if (is_bf16) *is_bf16 = 0;   // forward_cached always runs the fp32 path (rows <= 128 or fp32 mode)
    return RGRG_OK;
}

extern "C" int rgrg_decoder_take_id_error(rgrg_decoder* d, int* pending) {
    RGRG_CHECK_ARG(d && pending);
    RGRG_HIP(hipStreamSynchronize(d->stream));
    *pending = (d->h_id_error && *d->h_id_error) ? 1 : 0;
    if (*pending) {
        *d->h_id_error = 0;
        RGRG_HIP(hipMemsetAsync(d->id_error, 0, 2 * sizeof(int), d->stream));
    }
    return RGRG_OK;
}

extern "C" int rgrg_decoder_refresh_trainable(rgrg_decoder* d, void* stream) {
    RGRG_CHECK_ARG(d);
    hipStream_t caller = as_stream(stream), st = d->stream;
    ++d->epoch;   // the cache rows are rewritten: an open rolling session is stale
    RGRG_HIP(hipEventRecord(d->ev_in, caller));
    RGRG_HIP(hipStreamWaitEvent(st, d->ev_in, 0));
    Lin* ls[] = {&d->fst0, &d->fst2, &d->ukv};
    for (Lin* l : ls) {
        if (l->packed) {
            int rc = skinny_pack(l->w, l->packed, l->N, l->K, l->NT, st);
            if (rc) return rc;
        }
        if (l->wT) {
            int rc = launch_transpose_pad(l->w, l->wT, l->N, l->K, pad256(l->N), st);
            if (rc) return rc;
        }
    }
    RGRG_HIP(hipEventRecord(d->ev_in, st));
    RGRG_HIP(hipStreamWaitEvent(caller, d->ev_in, 0));
    return RGRG_OK;
}

// Test hook: the weight side of the folded LayerNorm (ln_fold16_kernel, used by rgrg_decoder_set_precision).
extern "C" int rgrg_debug_ln_fold16(const float* w, const float* gain, const float* beta, const float* bias, uint16_t* wb,
                                    float* colsum, float* shift, int N, int K, int fp16, void* stream) {
    RGRG_CHECK_ARG(w && gain && beta && wb && colsum && shift && N > 0 && K > 0);
    hipLaunchKernelGGL(ln_fold16_kernel, dim3((N + 3) / 4), dim3(256), 0, as_stream(stream), w, gain, beta, bias, wb, colsum, shift, N, K,
                       fp16 ? 1 : 0);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// Test hooks of the kernels that start a decode step and of the bookkeeping kernels between steps (tests/test_gpu_step_rows.py; the
// other files' kernels have theirs next to them).  No decoder: the caller's device buffers, the given stream, the launchers above.
extern "C" int rgrg_debug_ln_rows(const float* x, const float* g, const float* b, float* xn, uint16_t* xn16, int fp16, int rows, int D,
                                  void* stream) {
    RGRG_CHECK_ARG(x && g && b && (xn || xn16) && rows >= 1 && D == 1024);   // both given, as the step gives them: xn16 is written
    RGRG_CHECK_ARG(xn16 || !fp16);
    return launch_ln_rows(x, g, b, xn, D, xn16, fp16 ? 1 : 0, rows, as_stream(stream));
}

extern "C" int rgrg_debug_embed_ln(const float* wte, const int64_t* ids, int ld_ids, const int* step, const int* tok_override,
                                   const int* pos_override, const float* g, const float* b, float* x, float* xn, uint16_t* xn16,
                                   float* stats, int fp16, int rows, int D, void* stream) {
    RGRG_CHECK_ARG(wte && step && x && rows >= 1 && D == 1024);
    RGRG_CHECK_ARG(tok_override || (ids && ld_ids >= 1));
    if (stats) RGRG_CHECK_ARG(xn16);                        // the raw 16-bit row and its slots
    else RGRG_CHECK_ARG(g && b && (xn || xn16));            // LayerNorm as 16 bit where xn16 is given, else as fp32
    RGRG_CHECK_ARG(xn16 || !fp16);
    return launch_embed_ln(wte, reinterpret_cast<const long long*>(ids), ld_ids, step, g, b, x, xn, D, tok_override, xn16, fp16 ? 1 : 0,
                           pos_override, stats, rows, as_stream(stream));
}

extern "C" int rgrg_debug_kv_slot0(const float* ukv, int ld, void* kv, int64_t layer_stride, int64_t kv_stride, int S, int H, int slots, int L,
                                   int row_mul, int kv_bytes, int fp16, void* stream) {
    RGRG_CHECK_ARG(ukv && kv && S >= 1 && H >= 1 && slots >= 1 && L >= 1 && row_mul >= 1);
    RGRG_CHECK_ARG(kv_bytes == 4 || kv_bytes == 2 || kv_bytes == 1);
    RGRG_CHECK_ARG(kv_bytes == 2 || !fp16);   // the 16-bit type of a cache that is not 16 bit
    const int64_t plane = ((int64_t)(S - 1) * row_mul + 1) * H * slots * 64;   // elements up to the end of the last row written
    RGRG_CHECK_ARG((int64_t)ld >= (int64_t)L * 2 * H * 64 && kv_stride >= plane && layer_stride >= kv_stride + plane);
    const KvFormat fmt = kv_bytes == 4 ? KV_F32 : kv_bytes == 1 ? KV_E4M3 : (fp16 ? KV_F16 : KV_BF16);
    return launch_kv_slot0(ukv, ld, kv, (size_t)layer_stride, (size_t)kv_stride, S, H, slots, L, row_mul, fmt, fp16 ? 1 : 0, as_stream(stream));
}

extern "C" int rgrg_debug_decode_reset(int64_t* ids, int ld_ids, int* finished, int* step, int* done_len, int* sync, int S, int L,
                                       void* stream) {
    RGRG_CHECK_ARG(ids && finished && step && done_len && sync && S >= 1 && L >= 1 && ld_ids >= L);
    return launch_decode_reset(reinterpret_cast<long long*>(ids), ld_ids, finished, step, done_len, sync, S, L, as_stream(stream));
}

extern "C" int rgrg_debug_beam_first_mask(const int* first, int R, int slots, float* kmask, void* stream) {
    RGRG_CHECK_ARG(first && kmask && R >= 1 && slots >= 1);
    return launch_beam_first_mask(first, R, slots, kmask, as_stream(stream));
}

extern "C" int rgrg_debug_key_mask(const float* am, int L, int S, int slots, float* kmask, void* stream) {
    RGRG_CHECK_ARG(am && kmask && S >= 1 && L >= 1 && slots >= 1);
    return launch_key_mask(am, L, S, slots, kmask, as_stream(stream));
}

extern "C" int rgrg_debug_forward_cached_tokens(const int64_t* ids, const int64_t* pos_ids, int T, int j, int S, int V, int* tok, int* row_pos,
                                                int* step, int position, void* stream) {
    RGRG_CHECK_ARG(ids && tok && step && S >= 1 && T >= 1 && j >= 0 && j < T && V >= 1);
    RGRG_CHECK_ARG(!pos_ids || row_pos);
    return launch_forward_cached_tokens(reinterpret_cast<const long long*>(ids), reinterpret_cast<const long long*>(pos_ids), T, j, S, V, tok,
                                        row_pos, step, position, as_stream(stream));
}

// Test hooks of the two weight-streaming families (tests/test_gpu_skinny_gemms.py).  No decoder: the caller's device buffers, the
// given stream, and the shape rules / packing steps / kernel dispatch of the product path (direct_shape, direct_pack, direct_pack16,
// direct_dispatch, skinny_shape, skinny_pack, launch_skinny_any).  Every argument is validated before anything is launched.
#define DBG_REJECT(cond, ...)                                     \
    do {                                                          \
        if (cond) { set_error(__VA_ARGS__); return RGRG_EINVAL; } \
    } while (0)

extern "C" int rgrg_debug_direct_pack(const float* W, const float* ln_g, const float* ln_b, const float* bias, int N, int K, int w16,
                                      float* packed, uint16_t* packed16, float* c1, float* c2, float* c1_16, void* stream) {
    const bool lnf = ln_g != nullptr;
    int KS, NT;
    DBG_REJECT(!W || !packed, "rgrg_debug_direct_pack: missing operand (W / packed)");
    DBG_REJECT((ln_g != nullptr) != (ln_b != nullptr), "rgrg_debug_direct_pack: LayerNorm gain and beta go together");
    DBG_REJECT(w16 < 0 || w16 > 2, "rgrg_debug_direct_pack: w16 = %d (0 fp32, 1 bf16, 2 fp16)", w16);
    DBG_REJECT(!direct_shape(N, K, lnf, &KS, &NT), "rgrg_debug_direct_pack: N=%d K=%d unsupported by the fused plan", N, K);
    DBG_REJECT(lnf && (!c1 || !c2), "rgrg_debug_direct_pack: missing operand (c1 / c2 of a folded LayerNorm)");
    DBG_REJECT(w16 && !packed16, "rgrg_debug_direct_pack: missing operand (packed16)");
    DBG_REJECT(w16 && lnf && !c1_16, "rgrg_debug_direct_pack: missing operand (c1_16)");
    hipStream_t st = as_stream(stream);
    int rc = direct_pack(W, bias, ln_g, ln_b, N, K, NT, packed, c1, c2, st);
    if (rc || !w16) return rc;
    return direct_pack16(packed, packed16, lnf ? c1_16 : nullptr, NT, K, w16 == 2 ? 1 : 0, st);
}

extern "C" int rgrg_debug_direct_linear(const rgrg_direct_args* u, int mode, int lnf, int w16, int M, int* kernel_ran, void* stream) {
    DBG_REJECT(!u, "rgrg_debug_direct_linear: missing operand (args)");
    DBG_REJECT(M < 1 || M > SKINNY_MAX_ROWS, "rgrg_debug_direct_linear: %d rows (1 .. %d)", M, SKINNY_MAX_ROWS);
    DBG_REJECT(lnf != 0 && lnf != 1, "rgrg_debug_direct_linear: lnf = %d", lnf);
    DBG_REJECT(!((!lnf && mode == DX_PLAIN) || (lnf && mode >= DX_PLAIN && mode <= DX_EMBED_TOKPOS)),
               "rgrg_debug_direct_linear: unsupported mode %d (lnf %d)", mode, lnf);
    DBG_REJECT(w16 < 0 || w16 > 2, "rgrg_debug_direct_linear: w16 = %d (0 fp32, 1 bf16, 2 fp16)", w16);
    DBG_REJECT(w16 && M <= PAD_ROWS, "rgrg_debug_direct_linear: the 16-bit-weight kernels need more than one row tile (%d rows)", M);
    DBG_REJECT(u->act < RGRG_ACT_NONE || u->act > RGRG_ACT_GELU_NEW, "rgrg_debug_direct_linear: act = %d", u->act);
    DirectArgs a{};
    DBG_REJECT(!direct_shape(u->N, u->K, lnf != 0, &a.KS, &a.NT), "rgrg_debug_direct_linear: N=%d K=%d unsupported by the fused plan", u->N, u->K);
    DBG_REJECT(!u->P || (lnf && (!u->bias || !u->c1)), "rgrg_debug_direct_linear: missing operand (P; c2 as bias and c1 when lnf)");
    DBG_REJECT((mode == DX_PLAIN || mode == DX_COMBINE4) && !u->Xf, "rgrg_debug_direct_linear: missing operand (Xf)");
    DBG_REJECT(mode == DX_COMBINE4 && !u->part, "rgrg_debug_direct_linear: missing operand (part)");
    DBG_REJECT(mode >= DX_EMBED && !u->wte, "rgrg_debug_direct_linear: missing operand (wte)");
    DBG_REJECT(mode == DX_EMBED && (!u->ids || !u->step || u->ld_ids < 1), "rgrg_debug_direct_linear: missing operand (ids / ld_ids / step)");
    DBG_REJECT(mode == DX_EMBED_TOK && (!u->tok_override || !u->step), "rgrg_debug_direct_linear: missing operand (tok_override / step)");
    DBG_REJECT(mode == DX_EMBED_TOKPOS && (!u->tok_override || !u->pos_override), "rgrg_debug_direct_linear: missing operand (tok_override / pos_override)");
    DBG_REJECT(mode == DX_PLAIN && u->xout, "rgrg_debug_direct_linear: xout goes with a mode that rebuilds the residual stream");
    DBG_REJECT((u->cand_val != nullptr) != (u->cand_idx != nullptr), "rgrg_debug_direct_linear: missing operand (cand_val and cand_idx go together)");
    if (a.KS > 1) {
        DBG_REJECT(!u->part_out, "rgrg_debug_direct_linear: missing operand (part_out of a split-K GEMM)");
        DBG_REJECT(u->Y || u->Yf || u->Rf || u->zero_acc || u->cand_val, "rgrg_debug_direct_linear: a split-K GEMM writes part_out only");
    } else {
        DBG_REJECT(u->part_out, "rgrg_debug_direct_linear: part_out goes with K = %d", 4 * DK_SLICE);
        DBG_REJECT(!u->Y && !u->Yf, "rgrg_debug_direct_linear: missing operand (Y or Yf)");
        DBG_REJECT(u->Y && u->ldy < u->N, "rgrg_debug_direct_linear: ldy %d < N %d", u->ldy, u->N);
    }
    DBG_REJECT((u->Yf || u->Rf || u->zero_acc || u->part_out) && u->N % 16 != 0,
               "rgrg_debug_direct_linear: N = %d with a fragment-major output, residual or accumulator (N %% 16 == 0)", u->N);
    a.Xf = u->Xf; a.part = u->part; a.xout = u->xout; a.wte = u->wte; a.ids = reinterpret_cast<const long long*>(u->ids); a.ld_ids = u->ld_ids;
    a.step = u->step; a.tok_override = u->tok_override; a.pos_override = u->pos_override;
    a.P = reinterpret_cast<const float*>(u->P); a.bias = u->bias; a.c1 = u->c1; a.Rf = u->Rf; a.Y = u->Y; a.ldy = u->ldy; a.Yf = u->Yf;
    a.part_out = u->part_out; a.zero_acc = u->zero_acc; a.M = M; a.K = u->K; a.N = u->N; a.act = u->act;
    a.cand_val = u->cand_val; a.cand_idx = u->cand_idx;
    int rc = init_skinny_attrs();
    if (rc) return rc;
    return direct_dispatch(a, lnf != 0, mode, w16, as_stream(stream), kernel_ran);
}

extern "C" int rgrg_debug_skinny_linear(const float* X, const float* W, const float* bias, const float* R, float* Y, int M, int N, int K,
                                        int ldy, int act, void* stream) {
    DBG_REJECT(!X || !W || !Y, "rgrg_debug_skinny_linear: missing operand (X / W / Y)");
    DBG_REJECT(M < 1 || M > SKINNY_MAX_ROWS, "rgrg_debug_skinny_linear: %d rows (1 .. %d)", M, SKINNY_MAX_ROWS);
    DBG_REJECT(act < RGRG_ACT_NONE || act > RGRG_ACT_GELU_NEW, "rgrg_debug_skinny_linear: act = %d", act);
    int KS, NT, pw;
    DBG_REJECT(N < 1 || K < 64 || !skinny_shape(N, K, &KS, &NT, &pw), "rgrg_debug_skinny_linear: no skinny GEMM instance for N=%d K=%d", N, K);
    DBG_REJECT(ldy < N, "rgrg_debug_skinny_linear: ldy %d < N %d", ldy, N);
    hipStream_t st = as_stream(stream);
    int rc = init_skinny_attrs();
    if (rc) return rc;
    const int mt = (M + PAD_ROWS - 1) / PAD_ROWS;
    float *packed = nullptr, *part = nullptr;
    RGRG_HIP(hipMalloc((void**)&packed, (size_t)NT * 32 * K * sizeof(float)));
    if (KS > 1 && hipMalloc((void**)&part, (size_t)mt * KS * PAD_ROWS * NT * 32 * sizeof(float)) != hipSuccess) {
        (void)hipFree(packed);
        set_error("rgrg_debug_skinny_linear: out of device memory");
        return RGRG_EHIP;
    }
    rc = skinny_pack(W, packed, N, K, NT, st);
    SkinnyArgs a{X, packed, bias, R, Y, part, M, K, N, NT, KS, ldy, act};
    if (!rc) rc = launch_skinny_any(a, st);
    if (!rc && KS > 1) {
        const int total = M * N;
        hipLaunchKernelGGL(skinny_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, a);
        if (hipGetLastError() != hipSuccess) { set_error("rgrg_debug_skinny_linear: skinny_reduce_kernel launch failed"); rc = RGRG_EHIP; }
    }
    const hipError_t e = hipStreamSynchronize(st);   // the temporaries are the call's own: they must outlive the launches
    (void)hipFree(packed);
    (void)hipFree(part);
    if (!rc && e != hipSuccess) { set_error("rgrg_debug_skinny_linear: %s", hipGetErrorString(e)); return RGRG_EHIP; }
    return rc;
}
#undef DBG_REJECT

static int set_precision_impl(rgrg_decoder* d, int mode);
extern "C" int rgrg_decoder_set_precision(rgrg_decoder* d, int mode) {
    RGRG_CHECK_ARG(d && mode >= 0 && mode <= 2);
    if (mode == d->bf16_gemms) return RGRG_OK;
    const int prev = d->bf16_gemms;
    ++d->epoch;   // an open rolling session is stale
    const int rc = set_precision_impl(d, mode);
    if (rc) {
        // a copy or an allocation failed half way: the decoder goes back to the mode it was in - whose copies may
        // have been re-typed already, so every 16-bit copy is marked stale (the next successful switch redoes them all) and the
        // mode falls back to fp32 unless it already was - and graphs captured for either type are dropped
        auto stale = [](Lin& l) { l.wb_f16 = -1; l.wb_ln_f16 = -1; l.wTb_f16 = -1; };
        stale(d->lm_head); stale(d->ukv); stale(d->fst2);
        for (auto& w : d->layers) { stale(w.c_attn); stale(w.attn_proj); stale(w.c_fc); stale(w.mlp_proj); }
        d->bf16_gemms = 0;
        (void)prev;
        for (auto& g : d->graphs) (void)hipGraphExecDestroy(g.exec);
        d->graphs.clear();
    }
    return rc;
}
static int set_precision_impl(rgrg_decoder* d, int mode) {
    d->logits_valid = false;   // (called on a mode CHANGE only) the retained ln_f rows belong to the other mode's weights
    const int prev = d->bf16_gemms;
    d->bf16_gemms = mode;   // d->f16() below is the NEW type
    if (mode) {
        int rc = init_gemm_bf16_attrs();
        if (rc) { d->bf16_gemms = prev; return rc; }
        auto mk = [&](Lin& l) -> int {   // 16-bit copy of the weight in the requested type (re-converted when the type changes)
            if (l.wb && l.wb_f16 == d->f16()) return RGRG_OK;
            if (!l.wb) {
                int r = dmalloc(d, &l.wb, (size_t)l.N * l.K * 2, false);
                if (r) return r;
            }
            l.wb_f16 = d->f16();
            return convert_f32_to_bf16(l.w, l.wb, (size_t)l.N * l.K, d->stream, d->f16());
        };
        int rc2;
        RGRG_HIP(hipStreamSynchronize(d->stream));   // nothing queued still reads the copies that are about to be rewritten
        if (!d->xn16) {
            if ((rc2 = dmalloc(d, (void**)&d->xn16, (size_t)d->rows * d->D * 2, false)) ||
                (rc2 = dmalloc(d, (void**)&d->att16, (size_t)d->rows * d->D * 2, false)) ||
                (rc2 = dmalloc(d, (void**)&d->ff16, (size_t)d->rows * 4 * d->D * 2, false)))
                return rc2;
        }
        if ((rc2 = mk(d->lm_head))) return rc2;
        for (auto& w : d->layers) {
            if ((rc2 = mk(w.c_attn)) || (rc2 = mk(w.attn_proj)) || (rc2 = mk(w.c_fc)) || (rc2 = mk(w.mlp_proj))) return rc2;
        }
        // the fragment-packed weights of the fused plan rounded to the autocast type (33-128 rows, skinny_direct.inc W16), and for the
        // GEMMs behind a LayerNorm the column sums of the ROUNDED values (the folded mean term must match what the MFMA multiplies)
        if (d->w16_fused && d->rows > PAD_ROWS) {   // (a decoder of <= 32 rows never leaves the bit-exact fp32 kernels: no copies)
            auto mk16 = [&](Lin& l) -> int {
                if (!l.direct || !l.packed || (l.packed16 && l.packed16_f16 == d->f16())) return RGRG_OK;
                const size_t n = (size_t)l.NT * 16 * l.K;
                int r;
                if (!l.packed16 && (r = dmalloc(d, &l.packed16, n * 2, false))) return r;
                if (l.lnf && !l.c1_16 && (r = dmalloc(d, (void**)&l.c1_16, (size_t)l.NT * 16 * sizeof(float), false))) return r;
                if ((r = direct_pack16(l.packed, l.packed16, l.lnf ? l.c1_16 : nullptr, l.NT, l.K, d->f16(), d->stream))) return r;
                l.packed16_f16 = d->f16();
                return RGRG_OK;
            };
            if ((rc2 = mk16(d->lm_head))) return rc2;
            for (auto& w : d->layers) {
                if ((rc2 = mk16(w.c_attn)) || (rc2 = mk16(w.attn_proj)) || (rc2 = mk16(w.c_fc)) || (rc2 = mk16(w.mlp_proj))) return rc2;
            }
        }
        // the gain-scaled copies of the GEMMs that sit behind a LayerNorm (c_attn: ln_1, c_fc: ln_2, lm_head: ln_f)
        if (const char* e = getenv("RGRG_LN_FOLD")) d->ln_fold = atoi(e) != 0;
        if (d->ln_fold && d->D == 1024) {
            auto mkln = [&](Lin& l, const float* g, const float* be) -> int {
                if (l.wb_ln && l.wb_ln_f16 == d->f16()) return RGRG_OK;
                int r;
                if (!l.wb_ln && ((r = dmalloc(d, &l.wb_ln, (size_t)l.N * l.K * 2, false)) ||
                                 (r = dmalloc(d, (void**)&l.cs16, (size_t)l.N * sizeof(float), false)) ||
                                 (r = dmalloc(d, (void**)&l.c2_16, (size_t)l.N * sizeof(float), false))))
                    return r;
                l.wb_ln_f16 = d->f16();
                hipLaunchKernelGGL(ln_fold16_kernel, dim3((l.N + 3) / 4), dim3(256), 0, d->stream, l.w, g, be, l.b,
                                   reinterpret_cast<unsigned short*>(l.wb_ln), l.cs16, l.c2_16, l.N, l.K, d->f16());
                RGRG_LAUNCH_CHECK();
                return RGRG_OK;
            };
            if (!d->ln_stat && (rc2 = dmalloc(d, (void**)&d->ln_stat, (size_t)d->rows * 32 * sizeof(float), true))) return rc2;
            if (!d->sk_ws) {   // split-K of the two N = 1024 projections: up to 4 slabs of 64 x 64 fp32 per tile + a ticket per tile
                // (c_attn / c_fc of a <= 256-row step use it too: up to 4 row tiles x 64 column tiles x 2 slices)
                const size_t tiles = (size_t)((d->rows + 63) / 64) * (d->D / 64);
                const size_t small_rows = (size_t)((std::min(d->rows, 256) + 127) / 128) * 2;   // (the launcher may pick 128-row tiles)
                const size_t slabs = std::max(tiles * 4, small_rows * (size_t)(4 * d->D / 64) * 2), tickets = std::max(tiles, small_rows * (size_t)(4 * d->D / 64));
                if ((rc2 = dmalloc(d, (void**)&d->sk_ws, slabs * 4096 * sizeof(float), false)) ||
                    (rc2 = dmalloc(d, (void**)&d->sk_cnt, tickets * sizeof(unsigned), true)))
                    return rc2;
                const char* e1 = getenv("RGRG_SK_MLP");
                const char* e2 = getenv("RGRG_SK_ATTN");
                // measured (profiles/r05_splitk_decode_ab.log): at hundreds of rows the hand-off costs what the shorter K loop saves; unset =
                // automatic (steps of <= 256 rows only, linear())
                d->sk_mlp = e1 ? atoi(e1) : -1;
                d->sk_attn = e2 ? atoi(e2) : -1;
                if (d->sk_mlp == 0) d->sk_mlp = 1;
                if (d->sk_attn == 0) d->sk_attn = 1;
                if (d->sk_mlp > 4) d->sk_mlp = 4;
                if (d->sk_attn > 4) d->sk_attn = 4;
            }
            for (auto& w : d->layers) {
                if ((rc2 = mkln(w.c_attn, w.ln1_g, w.ln1_b)) || (rc2 = mkln(w.c_fc, w.ln2_g, w.ln2_b))) return rc2;
            }
        }
        RGRG_HIP(hipStreamSynchronize(d->stream));
    }
    // captured graphs bake the GEMM choice in: drop them
    for (auto& g : d->graphs) (void)hipGraphExecDestroy(g.exec);
    d->graphs.clear();
    return RGRG_OK;
}

extern "C" int rgrg_decoder_set_kv_format(rgrg_decoder* d, int fmt) {
    RGRG_CHECK_ARG(d && (fmt == 0 || fmt == 1));
    if (fmt == d->kv8) return RGRG_OK;
    RGRG_HIP(hipStreamSynchronize(d->stream));
    d->kv8 = fmt;
    d->logits_valid = false;
    ++d->epoch;   // an open rolling session is stale
    // captured graphs bake the attention kernel and the cache addresses in: drop them
    for (auto& g : d->graphs) (void)hipGraphExecDestroy(g.exec);
    d->graphs.clear();
    return RGRG_OK;
}

extern "C" int rgrg_decoder_kv_format_in_use(rgrg_decoder* d, int rows) { return d && rows > 0 ? (int)kv_format(d, rows) : -1; }

extern "C" int rgrg_decoder_copy_last_logits(rgrg_decoder* d, float* dst, int S, void* stream) {
    RGRG_CHECK_ARG(d && dst && S > 0 && S <= d->max_seqs);
    if (!d->logits_valid) {
        set_error("decoder: no logits of a completed step to copy - the last generate / beam / cached call failed, or a timing hook or a "
                  "precision change has reused the decoder's work space since");
        return RGRG_EINVAL;
    }
    if (d->logits_stale_rows > 0) {   // the greedy step kept only arg-max candidates: the logits of its last step from the retained ln_f rows
        const int rows = d->logits_stale_rows;
        RGRG_CHECK_ARG(S <= rows);
        int rc = linear(d, d->lm_head, d->xn, nullptr, d->logits, rows, d->ld_logits, RGRG_ACT_NONE, false, d->xn16);
        if (rc) return rc;
        RGRG_HIP(hipStreamSynchronize(d->stream));
        d->logits_stale_rows = 0;
    }
    RGRG_HIP(hipMemcpy2DAsync(dst, (size_t)d->V * 4, d->logits, (size_t)d->ld_logits * 4, (size_t)d->V * 4, S,
                              hipMemcpyDeviceToDevice, as_stream(stream)));
    RGRG_HIP(hipStreamSynchronize(as_stream(stream)));
    return RGRG_OK;
}

// Live timing of the two kernel families of one decode step, each as `iters` back-to-back replays of ITS launches of
// one step (24 layers [+ lm_head]) between one pair of HIP events on the decoder's stream:
//   * the projection GEMMs exactly as the step would launch them for S token rows in the current precision mode
//     (fused fragment-direct kernels <= 128 rows, tiled fp32 / bf16-weight MFMA GEMMs above);
//   * the single-query attention at `nkeys` keys per sequence (the step counter is set to nkeys - 2 for the timing).
// Token / cache contents are whatever the last generate() left: timing only.
// Token rows (sequences x beams) up to which a decode step of `d` runs the fused fragment-direct plan IN ITS CURRENT precision mode
// (128 in fp32; 64 under autocast - 33-64 on 16-bit weights; decode_row_limit above); more rows take the many-sequence path.
extern "C" int rgrg_decoder_row_limit(rgrg_decoder* d) { return d ? decode_row_limit(d) : -1; }

// Measurement hook (tools/overlap_probe.py): `iters` x n_layer attention launches of the many-sequence step at `nkeys` keys on the
// caller's stream (asynchronous; the state of the last generate() of S sequences) - the HBM-bound half of a decode step as a
// background load beside other work.
extern "C" int rgrg_decoder_attention_only(rgrg_decoder* d, int S, int nkeys, int iters, void* stream) {
    RGRG_CHECK_ARG(d && S > decode_row_limit(d) && S <= d->rows && nkeys >= 2 && nkeys <= d->T && iters > 0);
    hipStream_t keep = d->stream;
    d->stream = as_stream(stream);
    hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, d->stream, d->step, nkeys - 2);
    int rc = RGRG_OK;
    unsigned short* att16 = (kv_is_bf16(d, S) && d->xn16) ? d->att16 : nullptr;
    const StepSpec step{S};   // the variant the greedy step launches
    const bool qc = step_qkv_cache(d, step);
    for (int it = 0; it < iters && !rc; ++it)
        for (int l = 0; l < d->n_layer && !rc; ++l) rc = launch_attention(d, l, step, 0, S, att16, 0, qc);
    hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, d->stream, d->step, 0);
    d->stream = keep;
    return rc;
}

// Measurement hook (tools/step_trace.py): enqueue `iters` + 1 many-sequence decode steps EAGERLY at `nkeys` keys (the state of
// the last generate() of S sequences), the last one with a hipEvent behind every launch on the stream it went to, and return
// (first row of the range, tag, ms since the step's first launch) per launch - the true timeline of the row-range chains
// under concurrency (rocprofv3's kernel trace serialises the queues).  recs: 3 floats per launch.
extern "C" int rgrg_decoder_trace_step(rgrg_decoder* d, int S, int nkeys, int iters, float* recs, int max_recs, int* n_out) {
    RGRG_CHECK_ARG(d && S > decode_row_limit(d) && S <= d->rows && nkeys >= 2 && nkeys <= d->T && recs && n_out && iters >= 0);
    d->logits_valid = false;
    ++d->epoch;   // an open rolling session is stale
    std::vector<rgrg_decoder::TraceMark> marks;
    hipEvent_t base;
    RGRG_HIP(hipEventCreate(&base));
    int rc = RGRG_OK;
    const StepSpec step{S};
    for (int it = 0; it <= iters && !rc; ++it) {
        hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, d->stream, d->step, nkeys - 2);
        if (it == iters) { d->trace = &marks; RGRG_HIP(hipEventRecord(base, d->stream)); }
        rc = enqueue_step(d, step, false);
    }
    d->trace = nullptr;
    (void)hipStreamSynchronize(d->stream);
    int n = 0;
    for (auto& m : marks) {
        float ms = 0.f;
        if (!rc && n < max_recs && hipEventElapsedTime(&ms, base, m.ev) == hipSuccess) {
            recs[3 * n] = (float)m.r0; recs[3 * n + 1] = (float)m.tag; recs[3 * n + 2] = ms;
            ++n;
        }
        (void)hipEventDestroy(m.ev);
    }
    (void)hipEventDestroy(base);
    hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, d->stream, d->step, 0);
    (void)hipStreamSynchronize(d->stream);
    *n_out = n;
    return rc;
}

extern "C" int rgrg_decoder_time_step_parts(rgrg_decoder* d, int S, int nkeys, int iters, int one_range, float* ms_gemm, float* ms_attn,
                                            double* gemm_flops, double* gemm_weight_bytes, double* kv_bytes,
                                            int* gemm_launches) {
    RGRG_CHECK_ARG(d && S > 0 && S <= d->max_seqs && nkeys >= 2 && nkeys <= d->T && iters > 0 && ms_gemm && ms_attn);
    // one_range: every launch covers all S rows (the kernels alone on the GPU at the step's full size), whatever the step's own
    // row-range split is; 0: as the step launches them (concurrent row ranges on forked streams where it does that)
    d->logits_valid = false;   // the replays below overwrite x / xn16 / the logits work space
    ++d->epoch;   // an open rolling session is stale
    const int keep_chains = d->chains;
    if (one_range) d->chains = 1;
    struct Restore { rgrg_decoder* d; int c; ~Restore() { d->chains = c; } } restore{d, keep_chains};
    hipEvent_t e0, e1;
    RGRG_HIP(hipEventCreate(&e0));
    RGRG_HIP(hipEventCreate(&e1));
    const int D = d->D;
    const bool fused = d->lm_head.direct && S <= decode_row_limit(d);
    const bool bf = kv_is_bf16(d, S);
    d->step_rows = S;   // (linear()'s automatic split-K looks at the step's rows)
    unsigned short* xn16 = (bf && d->xn16) ? d->xn16 : nullptr;
    unsigned short* att16 = xn16 ? d->att16 : nullptr;
    unsigned short* ff16 = xn16 ? d->ff16 : nullptr;
    // the folded-LayerNorm variants the step launches in the 16-bit mode
    const bool fold = step_ln_fold(d, S);
    const StepSpec step{S};   // c_attn with the K/V-cache epilogue, q-only attention: as the greedy step
    const bool qc = step_qkv_cache(d, step);
    static const float cons_tag = 0.f;
    GemmLnFold prod{}, cons{};
    prod.Yb16 = xn16; prod.stats_out = d->ln_stat;
    cons.ln_stats = d->ln_stat; cons.ln_colsum = &cons_tag;
    const GemmLnFold* pf = fold ? &prod : nullptr;
    const GemmLnFold* cf = fold ? &cons : nullptr;
    int rc = RGRG_OK;
    float tg = 0.f, ta = 0.f;
    d->gemm_bytes_per_step = 0; d->gemm_flops_per_step = 0.0; d->gemm_launches_per_step = 0;
    // (c_attn's K/V-cache epilogue stores to slot *step + 1: the slot the attention replays below read last)
    if (qc) hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, d->stream, d->step, nkeys - 2);
    // ONE event pair around all `iters` replays (plus an untimed one in front): a pair per replay with a host wait in
    // between lets the GPU go idle between replays, and each then starts on ramping clocks (read 3-6 % slow)
    for (int it = -1; it < iters && !rc; ++it) {
        const bool c = it == -1;   // the untimed replay also counts the step's bytes / flops / launches
        if (it == 0) RGRG_HIP(hipEventRecord(e0, d->stream));
        // the per-layer GEMMs as the step launches them: in row ranges on forked streams where the step does (run_row_ranges)
        rc = run_row_ranges(d, S, fused ? 1 : step_chains(d, S, true, fold), [&](int r0, int rows) -> int {
            const size_t o = (size_t)r0 * D;
            GemmLnFold prod_r = prod, cons_r = cons;
            prod_r.Yb16 = xn16 ? xn16 + o : nullptr;
            prod_r.stats_out = d->ln_stat ? d->ln_stat + (size_t)r0 * 32 : nullptr;
            cons_r.ln_stats = prod_r.stats_out;
            const GemmLnFold* pfr = pf ? &prod_r : nullptr;
            const GemmLnFold* cfr = cf ? &cons_r : nullptr;
            unsigned short* xn16r = xn16 ? xn16 + o : nullptr;
            unsigned short* att16r = att16 ? att16 + o : nullptr;
            unsigned short* ff16r = ff16 ? ff16 + 4 * o : nullptr;
            int rc2 = RGRG_OK;
            for (int l = 0; l < d->n_layer && !rc2; ++l) {
                const LayerW& w = d->layers[l];
                if (fused) {
                    if ((rc2 = enqueue_layer_gemms(d, l ? l : 1, step, c, d->x, d->x2, 0))) break;
                    if ((rc2 = enqueue_layer_gemms(d, l, step, c, d->x, d->x2, 1))) break;
                    continue;
                }
                const GemmLnFold cons_kv = qc ? cons_kv_cache(d, cons_r, l, r0) : cons_r;
                if ((rc2 = linear(d, w.c_attn, d->xn + o, nullptr, d->qkv + 3 * o, rows, 3 * D, RGRG_ACT_NONE, c, xn16r, nullptr, qc ? &cons_kv : cfr))) break;
                if ((rc2 = linear(d, w.attn_proj, d->att + o, d->x + o, d->h1 + o, rows, D, RGRG_ACT_NONE, c, att16r, nullptr, pfr))) break;
                if ((rc2 = linear(d, w.c_fc, d->xn + o, nullptr, d->ff + 4 * o, rows, 4 * D, RGRG_ACT_GELU_NEW, c, xn16r, ff16r, cfr))) break;
                if ((rc2 = linear(d, w.mlp_proj, d->ff + 4 * o, d->x + o, d->h1 + o, rows, D, RGRG_ACT_NONE, c, ff16r, nullptr, pfr))) break;
            }
            return rc2;
        });
        if (!rc && fused) {
            DirectArgs h{};
            h.Xf = d->x; h.part = d->part; h.Y = d->logits; h.ldy = d->ld_logits; h.act = RGRG_ACT_NONE;
            rc = direct_linear(d, d->lm_head, h, DX_COMBINE4, S, c, true);
        } else if (!rc) {
            if (xn16 && lm_head_cand_path(d, S)) {   // as the greedy step launches it: arg-max epilogue, no logits
                GemmLnFold ce{};
                ce.cand_val = d->cand_val; ce.cand_idx = d->cand_idx;
                rc = linear(d, d->lm_head, d->xn, nullptr, nullptr, S, d->ld_logits, RGRG_ACT_NONE, c, xn16, nullptr, &ce);
            } else {
                rc = linear(d, d->lm_head, d->xn, nullptr, d->logits, S, d->ld_logits, RGRG_ACT_NONE, c, xn16);
            }
        }
    }
    if (!rc) {
        RGRG_HIP(hipEventRecord(e1, d->stream));
        RGRG_HIP(hipEventSynchronize(e1));
        RGRG_HIP(hipEventElapsedTime(&tg, e0, e1));
        hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, d->stream, d->step, nkeys - 2);
        for (int it = -1; it < iters && !rc; ++it) {
            if (it == 0) RGRG_HIP(hipEventRecord(e0, d->stream));
            rc = run_row_ranges(d, S, fused ? 1 : step_chains(d, S, true, fold), [&](int r0, int rows) -> int {
                int rc2 = RGRG_OK;
                for (int l = 0; l < d->n_layer && !rc2; ++l)
                    rc2 = launch_attention(d, l, step, r0, rows, att16 ? att16 + (size_t)r0 * D : nullptr, fused ? 1 : 0, qc);
                return rc2;
            });
        }
        if (!rc) {
            RGRG_HIP(hipEventRecord(e1, d->stream));
            RGRG_HIP(hipEventSynchronize(e1));
            RGRG_HIP(hipEventElapsedTime(&ta, e0, e1));
        }
        hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, d->stream, d->step, 0);
        (void)hipStreamSynchronize(d->stream);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    *ms_gemm = tg;
    *ms_attn = ta;
    if (gemm_flops) *gemm_flops = d->gemm_flops_per_step;
    if (gemm_weight_bytes) *gemm_weight_bytes = (double)d->gemm_bytes_per_step;
    if (kv_bytes) *kv_bytes = (double)d->n_layer * 2.0 * S * D * nkeys * (kv_format(d, S) == KV_E4M3 ? 1.0 : bf ? 2.0 : 4.0);
    if (gemm_launches) *gemm_launches = d->gemm_launches_per_step;
    return RGRG_OK;
}

// Test hooks: the two kernels behind a greedy step's logits alone on caller buffers, launched as enqueue_head launches them.
// logits_candidates_kernel: NT = ceil(V / 32) tiles per row on a (4, rows) grid.
extern "C" int rgrg_debug_logits_candidates(const float* logits, int ld, int V, int rows, float* cand_val, int* cand_idx, void* stream) {
    RGRG_CHECK_ARG(logits && cand_val && cand_idx && V >= 1 && rows >= 1 && rows <= 65535);
    const int NT = (V + 31) / 32;
    RGRG_CHECK_ARG(ld >= V && ld >= 32 * NT && ld % 4 == 0 && ((uintptr_t)logits & 15) == 0);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(logits_candidates_kernel, dim3(4, rows), dim3(256), 0, st, logits, ld, V, NT, cand_val, cand_idx);
    hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { set_error("rgrg_debug_logits_candidates: %s", hipGetErrorString(e)); return RGRG_EHIP; }
    return RGRG_OK;
}
// argmax_update_kernel with record_step_token: one workgroup per row.  *step is read back first: column *step + 1 must exist.
extern "C" int rgrg_debug_argmax_update(const float* cand_val, const int* cand_idx, int NT, int64_t* ids, int ld_ids, int* finished,
                                        int* step, int* done_len, int* sync, int S, void* stream) {
    RGRG_CHECK_ARG(cand_val && cand_idx && ids && finished && step && done_len && sync && NT >= 1 && S >= 1 && S <= 65535 && ld_ids >= 2);
    hipStream_t st = as_stream(stream);
    int t = -1;
    RGRG_HIP(hipMemcpyAsync(&t, step, sizeof(int), hipMemcpyDeviceToHost, st));
    RGRG_HIP(hipStreamSynchronize(st));
    RGRG_CHECK_ARG(t >= 0 && t + 1 < ld_ids);
    hipLaunchKernelGGL(argmax_update_kernel, dim3(S), dim3(256), 0, st, cand_val, cand_idx, NT, reinterpret_cast<long long*>(ids), ld_ids,
                       finished, step, done_len, sync, S);
    hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { set_error("rgrg_debug_argmax_update: %s", hipGetErrorString(e)); return RGRG_EHIP; }
    return RGRG_OK;
}
