// Decode attention of the RGRG language model for gfx950: ONE new token per sequence against the K/V cache (fp32 or 16 bit; the e4m3
// kernel is attn_kv8.hip), the one launcher that chooses among the kernels' variants, and the test hooks that drive it on the caller's
// buffers.  launch_attention (decoder.hip) fills an AttnDecodeLaunch (decoder_internal.h) from the decoder object and the step.
#include <math.h>

#include <algorithm>
#include <vector>

#include "decoder_internal.h"

namespace rgrg {

// Pseudo self-attention for ONE new token per sequence (GPT2PseudoAttention.forward with
// layer_past, :162-174, and _attn :84-122: scores / 8, softmax, . V; the causal mask row
// of a single query and the all-zero padding mask are no-ops in greedy generation).
// One workgroup per (sequence, head), 4 waves.  A 16-lane GROUP owns one key at a time (4 dims per lane), so a wave
// covers 4 consecutive keys (1 KiB of the cache row block) and the workgroup 16 keys per pass.  Every K and V row of a
// chunk of 16 * ATT_NI keys (144: one chunk up to max_length 142) is requested up front with UNCONDITIONAL loads
// (indices clamped, results selected afterwards): a conditional load costs a branch + a full s_waitcnt per load and
// serialises the latencies (the round-1 kernel: 9.7 us).  Each group keeps its own running softmax
// statistics (max, sum, weighted V sum over ITS keys) - no cross-lane traffic besides the 4-step DPP dot product -
// and the 16 partial results are merged once through LDS (flash-decoding inside the workgroup, one barrier).

__device__ __forceinline__ float group16_sum_dpp(float v) {  // sum over the 16 lanes of a DPP row, result in every lane
    v += dpp_get<0xB1, 0xf>(v);
    v += dpp_get<0x4E, 0xf>(v);
    v += dpp_get<0x141, 0xf>(v);
    v += dpp_get<0x140, 0xf>(v);
    return v;
}

// one chunk of 16 * NI keys starting at `base` (see the kernel below)
template <bool HAS_SRC, int NI, bool HAS_MASK = false>
__device__ __forceinline__ void attn_chunk(const float* __restrict__ kc, const float* __restrict__ vc, const int* __restrict__ srow, int s,
                                           int hd, int H, int T, int base, int nkeys, int slot, int wave, int g, int d4,
                                           const f32x4& q4, const f32x4& k4, const f32x4& v4, float& m, float& l, f32x4& acc,
                                           const float* __restrict__ kmask = nullptr) {
    int rowi[NI];  // beam search: the table entries are the oldest loads of the chunk, so that waiting for them waits for nothing else
#pragma unroll
    for (int i = 0; i < NI; ++i) rowi[i] = HAS_SRC ? srow[min(base + (i * 4 + wave) * 4 + g, nkeys - 1)] : s;
    // slot t + 1 of the table is stale: that key comes from k4 / v4 below
    f32x4 kk[NI], vv[NI];
    float mk[NI];   // HAS_MASK: the additive padding mask of the key's slot, (1 - attention_mask) * -1e4 (language_model.py:325-334)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int jc = min(base + (i * 4 + wave) * 4 + g, nkeys - 1);
        const size_t off = (((size_t)rowi[i] * H + hd) * T + jc) * 64 + d4 * 4;
        kk[i] = *reinterpret_cast<const f32x4*>(kc + off);
        vv[i] = *reinterpret_cast<const f32x4*>(vc + off);
        mk[i] = HAS_MASK ? kmask[(size_t)s * T + jc] : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);  // all 2 * NI loads are in flight before the first dot product waits
    // The running softmax advances ONE KEY AT A TIME, so that a group's result is a function of its sequence of keys alone and
    // not of how the launcher cuts that sequence into chunks: the 9- and the 2-key instantiation, and every size of the tail
    // chunk, give the same bits (tests/test_gpu_attention_kernels.py).  Per key one of (rescale of the past, weight of the key)
    // is 1 and the other exp(-|score - max|): one exponential per key, as before.  Contraction is spelled out (fmaf) and
    // otherwise off, so that the compiler cannot fuse the differently unrolled instantiations differently.
    {
#pragma clang fp contract(off)
    float sc[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = base + (i * 4 + wave) * 4 + g;
        if (j == slot) { kk[i] = k4; vv[i] = v4; }  // selects, not branches: the new token's key / value
        const float dot = group16_sum_dpp(fmaf(q4[0], kk[i][0], q4[1] * kk[i][1]) + fmaf(q4[2], kk[i][2], q4[3] * kk[i][3]));
        sc[i] = HAS_MASK ? dot / 8.0f + mk[i] : dot / 8.0f;
    }
    // prefix maxima first (a chain of compares), so that the exponentials below do not wait for one another
    float ex[NI];
    bool up[NI];
    float mp = m;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const bool valid = base + (i * 4 + wave) * 4 + g < nkeys;
        up[i] = valid && sc[i] > mp;                                 // this key raises the maximum (the first key: from -inf)
        ex[i] = valid ? expf(-fabsf(sc[i] - mp)) : 0.f;              // exp(-inf) = 0 on the first key, never NaN
        mp = up[i] ? sc[i] : mp;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const bool valid = base + (i * 4 + wave) * 4 + g < nkeys;
        const float scale = up[i] ? ex[i] : 1.f;
        const float p = up[i] ? 1.f : ex[i];                         // 0 for a key that does not exist
        l = fmaf(l, scale, p);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(p, valid ? vv[i][e] : 0.f, acc[e] * scale);
    }
    m = mp;
    }
}

// ATT_NI = keys per group per FULL chunk: 9 (up to 144 keys with everything in flight at once) when the grid is a
// fraction of a wave of workgroups per CU and the kernel is latency bound - the last (usually only) chunk is then sized
// to the keys that exist in steps of 16 (a wave-uniform switch; round 4: it used to request, dot and exponentiate 144
// rows whatever the step, 2.2x what a 128-token decode needs on average); 2 when thousands of workgroups queue up
// (throughput bound: fewer registers -> more resident workgroups).  A key's group and register do not depend on the
// chunk size and the running softmax advances key by key (attn_chunk): results are unchanged bit for bit, across the
// tail sizes and between the two instantiations.
// HAS_MASK (round 6, forward(use_cache=True) with padding): kmask [S][T] = the additive mask of every cache slot (slot 0, the image,
// holds 0); the default instantiation carries none of it.
// ROWSTEP (rolling-batch decoding, decoder_roll.hip): `step` is [S], the step of every sequence's OWN row - the workgroup of sequence s
// reads step[s] where the others read the one word *step; everything behind t is the same code, so a row at its own step t gives the
// bits the default instantiation gives at *step = t.  With HAS_SRC (rolling beam search, decoder_beam_roll.hip) the two are orthogonal:
// t, nkeys, slot and the chunk switch stay uniform over the workgroup (the wave, in the 16-bit kernel), the table is read per lane.
template <bool HAS_SRC, int ATT_NI, bool HAS_MASK = false, bool ROWSTEP = false>  // HAS_SRC (beam search): per-slot ancestor table (one more dependent load per key, requested first)
__global__ __launch_bounds__(256) void attn_decode_kernel(const float* __restrict__ qkv, int ld_qkv,
                                                          float* __restrict__ kc, float* __restrict__ vc,
                                                          const int* __restrict__ step, float* __restrict__ out,
                                                          int S, int H, int T, const int* __restrict__ src, int frag_out,
                                                          const float* __restrict__ kmask = nullptr) {
    __shared__ float pm[16], pl[16];
    __shared__ __attribute__((aligned(16))) float pacc[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x / H, hd = blockIdx.x - s * H;
    const int t = ROWSTEP ? step[s] : *step, nkeys = t + 2, slot = t + 1;
    const int g = lane >> 4, d4 = lane & 15;
    const float* row = qkv + (size_t)s * ld_qkv;
    const int D = H * 64;
    // beam search: slot j of this beam's history lives in the cache row of the ancestor that wrote it
    // (src[s][j]); the cache is never physically re-ordered (the reference's _reorder_cache, :492-496)
    const int* srow = HAS_SRC ? src + (size_t)s * T : nullptr;
    constexpr int ATT_CHUNK = 16 * ATT_NI;
    const f32x4 q4 = *reinterpret_cast<const f32x4*>(row + hd * 64 + d4 * 4);
    const f32x4 k4 = *reinterpret_cast<const f32x4*>(row + D + hd * 64 + d4 * 4);
    const f32x4 v4 = *reinterpret_cast<const f32x4*>(row + 2 * D + hd * 64 + d4 * 4);
    float m = -INFINITY, l = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#define ATT_CHUNK_CALL(NI_, BASE_) attn_chunk<HAS_SRC, NI_, HAS_MASK>(kc, vc, srow, s, hd, H, T, BASE_, nkeys, slot, wave, g, d4, q4, k4, v4, m, l, acc, kmask)
    if constexpr (ATT_NI == 9) {
        int base = 0;
        for (; nkeys - base > ATT_CHUNK; base += ATT_CHUNK) ATT_CHUNK_CALL(9, base);
        switch ((nkeys - base + 15) >> 4) {
            case 1: ATT_CHUNK_CALL(1, base); break;
            case 2: ATT_CHUNK_CALL(2, base); break;
            case 3: ATT_CHUNK_CALL(3, base); break;
            case 4: ATT_CHUNK_CALL(4, base); break;
            case 5: ATT_CHUNK_CALL(5, base); break;
            case 6: ATT_CHUNK_CALL(6, base); break;
            case 7: ATT_CHUNK_CALL(7, base); break;
            case 8: ATT_CHUNK_CALL(8, base); break;
            default: ATT_CHUNK_CALL(9, base); break;
        }
    } else {
        for (int base = 0; base < nkeys; base += ATT_CHUNK) ATT_CHUNK_CALL(ATT_NI, base);
    }
#undef ATT_CHUNK_CALL
    if (wave == 0 && g == 0) {
        *reinterpret_cast<f32x4*>(kc + (((size_t)s * H + hd) * T + slot) * 64 + d4 * 4) = k4;
        *reinterpret_cast<f32x4*>(vc + (((size_t)s * H + hd) * T + slot) * 64 + d4 * 4) = v4;
    }
    const int grp = wave * 4 + g;
    if (d4 == 0) { pm[grp] = m; pl[grp] = l; }
    *reinterpret_cast<f32x4*>(&pacc[grp][d4 * 4]) = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        float M = pm[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) M = fmaxf(M, pm[k]);
        float L = 0.f, o = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {  // groups without a key have max -inf and weight exp(-inf) = 0
            const float wgt = expf(pm[k] - M);
            L += pl[k] * wgt;
            o += pacc[k][threadIdx.x] * wgt;
        }
        // fused plan: the attention output is attn_proj's A operand -> fragment-major (skinny_direct.inc)
        out[frag_out ? frag_off(s, hd * 64 + threadIdx.x, D) : (size_t)s * D + hd * 64 + threadIdx.x] = o / L;
    }
}

// bf16 helpers for the opt-in bf16 K/V cache (torch.autocast(bf16) in the reference makes c_attn's output,
// hence ``present``, bf16 as well)
// the two values of a packed 16-bit pair as fp32 (bf16: shift / mask; fp16: v_cvt_f32_f16)
template <bool F16>
__device__ __forceinline__ float pair_lo(unsigned u) {
    if constexpr (F16) return f16_bits_to_f32(u & 0xffffu);
    else return __uint_as_float(u << 16);
}
template <bool F16>
__device__ __forceinline__ float pair_hi(unsigned u) {
    if constexpr (F16) return f16_bits_to_f32(u >> 16);
    else return __uint_as_float(u & 0xffff0000u);
}

// Wave-per-head variant of the bf16-cache attention (round 2): a WAVE owns one (sequence, head) - the 4 waves of a
// workgroup are 4 consecutive heads of one sequence - so there is no LDS, no barrier and a quarter of the workgroups
// (3712 instead of 14 848 at batch 32).  An 8-lane group still owns one key (one 16-byte load per lane and operand); a
// wave covers 8 keys per load instruction and keeps a whole chunk of 8 * NI keys (K and V: 2 * NI loads per lane)
// in flight.  The chunk size is picked per chunk from the wave-uniform key count (72 / 48 / 24 keys: a uniform branch
// around a fully unrolled, unconditional, clamped load block - never a branch around a single load), each group keeps
// a running softmax, and the 8 groups are merged at the end with cross-lane exchanges (lane ^ 8 by DPP row rotate,
// ^ 16 / ^ 32 through the LDS crossbar).
struct Kv16Row {  // this lane's 8 dims of the current token's q / k / v (fp32, as c_attn wrote them)
    f32x4 q0, q1, k0, k1, v0, v1;
};
template <bool F16>
__device__ __forceinline__ u32x4 kv16_pack_round(const f32x4& lo, const f32x4& hi) {  // 8 fp32 -> 8 16-bit values (RNE), packed
    u32x4 o;
    o[0] = to16<F16>(lo[0]) | (to16<F16>(lo[1]) << 16);
    o[1] = to16<F16>(lo[2]) | (to16<F16>(lo[3]) << 16);
    o[2] = to16<F16>(hi[0]) | (to16<F16>(hi[1]) << 16);
    o[3] = to16<F16>(hi[2]) | (to16<F16>(hi[3]) << 16);
    return o;
}

// FIRST: the first chunk of a wave turns the raw q / k / v into q[8] and the packed bf16 kn16 / vn16 (after its loads)
// QONLY: c_attn's epilogue already stored the new token's k / v in cache slot t + 1 (gemm_bf16.hip, GemmBf16Params::kv_k): the
// row brings q only, slot t + 1 is read like every other key - no k / v row, no kn16 / vn16, no patch
// HAS_FIRST (rgrg_decoder_generate_prompted, a left-padded prompt): cache slots 1 .. npad of the row are padding and are left out
// (score -inf); the reference adds -1e4 to their scores (language_model.py:316-334), whose weight next to the never-masked image
// key is exp(-1e4 + O(10)) = 0 in fp32 - the same result
template <int NI, bool HAS_SRC, bool FIRST, bool F16, bool QONLY, bool HAS_FIRST = false>
__device__ __forceinline__ void kv16_wave_chunk(const __amdgpu_buffer_rsrc_t kc, const __amdgpu_buffer_rsrc_t vc, const int* __restrict__ srow,
                                                int s, int hd, int H, int T, int base, int nkeys, int slot, int g, int d8,
                                                Kv16Row& r, float (&q)[8], u32x4& kn16, u32x4& vn16, float& m, float& l, float (&acc)[8],
                                                int npad = 0) {
    int rowi[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) rowi[i] = HAS_SRC ? srow[min(base + i * 8 + g, nkeys - 1)] : s;
    u32x4 kk[NI], vv[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int jc = min(base + i * 8 + g, nkeys - 1);
        // 32-bit byte offsets into one layer's K (V) plane through a buffer descriptor (the launcher checks that the
        // plane is < 2 GiB): half the address registers of 64-bit pointers; nt: a cache row is read once per step
        const unsigned off = ((unsigned)((rowi[i] * H + hd) * T + jc) * 64u + (unsigned)d8 * 8u) * 2u;
        kk[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(kc, (int)off, 0, 2));
        vv[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(vc, (int)off, 0, 2));
    }
    // All 2 * NI cache loads are in flight before anything waits.  The current token's q / k / v (requested before
    // the cache rows, so they arrive first) are consumed only HERE: used ahead of the chunk they would make the wave
    // wait for them before it has even issued the cache loads - two serialised memory latencies per wave.
    // (the empty asm pins the use below the loads: the compiler otherwise schedules / hoists the conversions of k and v
    // in front of the cache loads again)
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (FIRST) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (QONLY) asm volatile("" : "+v"(r.q0[e]), "+v"(r.q1[e]));
            else asm volatile("" : "+v"(r.q0[e]), "+v"(r.q1[e]), "+v"(r.k0[e]), "+v"(r.k1[e]), "+v"(r.v0[e]), "+v"(r.v1[e]));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { q[e] = r.q0[e]; q[4 + e] = r.q1[e]; }
        if constexpr (!QONLY) {
            kn16 = kv16_pack_round<F16>(r.k0, r.k1);
            vn16 = kv16_pack_round<F16>(r.v0, r.v1);
        }
    }
    float sc[NI];
    float cmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = base + i * 8 + g;
        if constexpr (!QONLY) {
            if (j == slot) { kk[i] = kn16; vv[i] = vn16; }
        }
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            dot += q[2 * e] * pair_lo<F16>(kk[i][e]) + q[2 * e + 1] * pair_hi<F16>(kk[i][e]);
        dot += dpp_get<0xB1, 0xf>(dot);
        dot += dpp_get<0x4E, 0xf>(dot);
        dot += dpp_get<0x141, 0xf>(dot);  // row_half_mirror: sum over the 8 lanes of the group
        if constexpr (HAS_FIRST) sc[i] = (j < nkeys && (j == 0 || j > npad)) ? dot / 8.0f : -INFINITY;
        else sc[i] = j < nkeys ? dot / 8.0f : -INFINITY;
        cmax = fmaxf(cmax, sc[i]);
    }
    const float m_new = fmaxf(m, cmax);
    const float scale = (m == -INFINITY) ? 0.f : expf(m - m_new);  // a group without any key yet keeps m = -inf
    const bool any = m_new != -INFINITY;
    l *= scale;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= scale;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = base + i * 8 + g;
        const float pj = (j < nkeys && any) ? expf(sc[i] - m_new) : 0.f;
        l += pj;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned u = j < nkeys ? vv[i][e] : 0u;
            acc[2 * e] += pj * pair_lo<F16>(u);
            acc[2 * e + 1] += pj * pair_hi<F16>(u);
        }
    }
    m = m_new;
}

// HAS_FIRST without HAS_SRC: `src` is [S], the padded prompt slots of every sequence (kv16_wave_chunk).  HAS_FIRST with HAS_SRC
// (beam search from a left-padded prompt, rgrg_decoder_beam_search_prompted): `src` is the ancestor table and the padded slots
// come in `first` [S], an operand only that instantiation reads
// ROWSTEP (rolling-batch decoding, decoder_roll.hip): `step` is [S] and a wave reads its item's step[s] inside the item loop: key
// count, slot of the new key / value and the chunk switch follow the ROW (all of them uniform over the wave, which owns one item at a
// time); the key-to-group-to-register mapping and the order of the sums are those of the default instantiation at *step = step[s]
template <bool HAS_SRC, bool F16, bool QONLY = false, bool HAS_FIRST = false, bool ROWSTEP = false>
__global__ __launch_bounds__(256) void attn_decode_kv16_wave_kernel(const float* __restrict__ qkv, int ld_qkv,
                                                                    u16* __restrict__ kc, u16* __restrict__ vc,
                                                                    const int* __restrict__ step, float* __restrict__ out,
                                                                    int S, int H, int T, const int* __restrict__ src,
                                                                    u16* __restrict__ out16, const int* __restrict__ first = nullptr) {
    const int lane = threadIdx.x & 63;
    int t = ROWSTEP ? 0 : *step, nkeys = t + 2, slot = t + 1;
    const int g = lane >> 3, d8 = lane & 7;
    const int D = H * 64;
    const __amdgpu_buffer_rsrc_t rk = dx_rsrc(kc), rv = dx_rsrc(vc);
    // (sequence, head) items: wave w of workgroup b takes items b * 4 + w, + 4 * gridDim.x, ...  The launcher either gives every
    // item its own wave (grid = S * H / 4) or - round 6, many-sequence step - caps the grid at a few workgroups per CU, so that
    // the kernel keeps the HBM stream going from a handful of resident waves and leaves the CU's wave slots, registers and LDS to
    // the GEMM workgroups of the other row ranges that run beside it (decoder.hip run_row_ranges).
    for (int item = blockIdx.x * 4 + (threadIdx.x >> 6); item < S * H; item += gridDim.x * 4) {
    const int s = item / H, hd = item - s * H;
    if constexpr (ROWSTEP) { t = step[s]; nkeys = t + 2; slot = t + 1; }
    const float* row = qkv + (size_t)s * ld_qkv;
    const int* srow = HAS_SRC ? src + (size_t)s * T : nullptr;
    const int npad = HAS_FIRST ? (HAS_SRC ? first[s] : src[s]) : 0;
    Kv16Row r;
    r.q0 = *reinterpret_cast<const f32x4*>(row + hd * 64 + d8 * 8);
    r.q1 = *reinterpret_cast<const f32x4*>(row + hd * 64 + d8 * 8 + 4);
    if constexpr (!QONLY) {
        r.k0 = *reinterpret_cast<const f32x4*>(row + D + hd * 64 + d8 * 8);
        r.k1 = *reinterpret_cast<const f32x4*>(row + D + hd * 64 + d8 * 8 + 4);
        r.v0 = *reinterpret_cast<const f32x4*>(row + 2 * D + hd * 64 + d8 * 8);
        r.v1 = *reinterpret_cast<const f32x4*>(row + 2 * D + hd * 64 + d8 * 8 + 4);
    }
    float m = -INFINITY, l = 0.f, acc[8], q[8];
    u32x4 kn16, vn16;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#define KV16_CHUNK(NI_, FIRST_, BASE_) \
    kv16_wave_chunk<NI_, HAS_SRC, FIRST_, F16, QONLY, HAS_FIRST>(rk, rv, srow, s, hd, H, T, BASE_, nkeys, slot, g, d8, r, q, kn16, vn16, m, l, acc, npad)
    // chunks of 72 keys while more than 72 remain, then ONE chunk sized to what is left in steps of 8 keys (a wave-uniform
    // switch around fully unrolled, unconditional, clamped load blocks - never a branch around a single load).  Round 4:
    // the tail used to be 24 / 48 / 72 keys, i.e. 18 % more rows requested (and exponentiated) than a 128-token decode
    // needs on average; in steps of 8 it is 5 %.  (nkeys >= 2: at least one chunk runs; a key's group and register do not
    // depend on the chunk size, so the result does not change.)
#define KV16_TAIL(FIRST_, BASE_, REM_)                                                                   \
    switch (((REM_) + 7) >> 3) {                                                                         \
        case 1: KV16_CHUNK(1, FIRST_, BASE_); break;                                                     \
        case 2: KV16_CHUNK(2, FIRST_, BASE_); break;                                                     \
        case 3: KV16_CHUNK(3, FIRST_, BASE_); break;                                                     \
        case 4: KV16_CHUNK(4, FIRST_, BASE_); break;                                                     \
        case 5: KV16_CHUNK(5, FIRST_, BASE_); break;                                                     \
        case 6: KV16_CHUNK(6, FIRST_, BASE_); break;                                                     \
        case 7: KV16_CHUNK(7, FIRST_, BASE_); break;                                                     \
        case 8: KV16_CHUNK(8, FIRST_, BASE_); break;                                                     \
        default: KV16_CHUNK(9, FIRST_, BASE_); break;                                                    \
    }
    if (nkeys > 72) {
        KV16_CHUNK(9, true, 0);
        int base = 72;
        for (; nkeys - base > 72; base += 72) KV16_CHUNK(9, false, base);
        KV16_TAIL(false, base, nkeys - base)
    } else {
        KV16_TAIL(true, 0, nkeys)
    }
#undef KV16_TAIL
#undef KV16_CHUNK
    if constexpr (!QONLY) {
        if (g == 0) {  // the new token's key / value -> cache slot t + 1 (8 lanes x 16 B = the 128-byte row)
            const size_t o = (((size_t)s * H + hd) * T + slot) * 64 + d8 * 8;
            *reinterpret_cast<u32x4*>(kc + o) = kn16;
            *reinterpret_cast<u32x4*>(vc + o) = vn16;
        }
    }
    // merge the 8 groups (lanes with equal d8): global max, rescale, sums
    float M = fmaxf(m, dpp_get<0x128, 0xf>(m));  // row_ror:8 = lane ^ 8 inside a 16-lane row
    M = fmaxf(M, __shfl_xor(M, 16, 64));
    M = fmaxf(M, __shfl_xor(M, 32, 64));
    const float wgt = (m == -INFINITY) ? 0.f : expf(m - M);  // M is finite: key 0 (the image) always exists
    l *= wgt;
    l += dpp_get<0x128, 0xf>(l);
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float o = acc[e] * wgt;
        o += dpp_get<0x128, 0xf>(o);
        o += __shfl_xor(o, 16, 64);
        o += __shfl_xor(o, 32, 64);
        acc[e] = o / l;
    }
    if (g == 0) {
        const size_t o = (size_t)s * D + hd * 64 + d8 * 8;
        if (out16) {
            u32x4 pk;
#pragma unroll
            for (int i = 0; i < 4; ++i) pk[i] = to16<F16>(acc[2 * i]) | (to16<F16>(acc[2 * i + 1]) << 16);
            *reinterpret_cast<u32x4*>(out16 + o) = pk;  // feeds the 16-bit attn_proj GEMM only
        } else {
            *reinterpret_cast<f32x4*>(out + o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
            *reinterpret_cast<f32x4*>(out + o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
        }
    }
    }   // items
}

// ------------------------------------------------------------------ the launcher
// The legal variants: every instantiation the library holds stands on exactly one line here, and a launch whose key is on no line is
// refused.  A new variant is one more line (and its kernel instantiation with it).
typedef void (*AttnKv16Kernel)(const float*, int, u16*, u16*, const int*, float*, int, int, int, const int*, u16*, const int*);
typedef void (*AttnF32Kernel)(const float*, int, float*, float*, const int*, float*, int, int, int, const int*, int, const float*);
struct AttnKv16Variant { bool src, q_only, first, row_step; AttnKv16Kernel bf16, fp16; };
struct AttnF32Variant { bool src, mask, row_step; AttnF32Kernel ni9, ni2; };
template <bool SRC, bool QONLY, bool FIRST, bool ROWSTEP>
constexpr AttnKv16Variant kv16_variant() {
    return {SRC, QONLY, FIRST, ROWSTEP, attn_decode_kv16_wave_kernel<SRC, false, QONLY, FIRST, ROWSTEP>,
            attn_decode_kv16_wave_kernel<SRC, true, QONLY, FIRST, ROWSTEP>};
}
template <bool SRC, bool MASK, bool ROWSTEP>
constexpr AttnF32Variant f32_variant() {
    return {SRC, MASK, ROWSTEP, attn_decode_kernel<SRC, 9, MASK, ROWSTEP>, attn_decode_kernel<SRC, 2, MASK, ROWSTEP>};
}
//                                                       src  q_only first row_step
static const AttnKv16Variant ATTN_KV16_VARIANTS[] = {
    kv16_variant<false, false, false, false>(),   // greedy / sampled steps that bring q | k | v
    kv16_variant<true,  false, false, false>(),   // beam search
    kv16_variant<false, true,  false, false>(),   // c_attn stored k / v (K/V-cache epilogue)
    kv16_variant<false, false, true,  false>(),   // behind a left-padded prompt
    kv16_variant<false, true,  true,  false>(),   // ... with c_attn's K/V-cache epilogue
    kv16_variant<true,  false, true,  false>(),   // beam search behind a left-padded prompt
    kv16_variant<false, false, false, true>(),    // rolling batch
    kv16_variant<true,  false, false, true>(),    // rolling beams
};
//                                                     src   mask  row_step
static const AttnF32Variant ATTN_F32_VARIANTS[] = {
    f32_variant<false, false, false>(),   // greedy / sampled steps
    f32_variant<true,  false, false>(),   // beam search
    f32_variant<false, true,  false>(),   // forward(use_cache=True) with a padded attention_mask (rgrg_decoder_forward_cached)
    f32_variant<true,  true,  false>(),   // beam search behind a left-padded prompt (rgrg_decoder_beam_search_prompted)
    f32_variant<false, false, true>(),    // rolling batch
    f32_variant<true,  false, true>(),    // rolling beams
};

int launch_attn_decode(const AttnDecodeLaunch& a) {
    // 1. normalise
    const bool f32 = a.fmt == KV_F32, e4m3 = a.fmt == KV_E4M3, kv16 = !f32 && !e4m3;
    const char* wave_fmt = e4m3 ? "e4m3" : "16-bit";
    const int ni = a.ni ? a.ni : (a.S * a.H <= 4096 ? 9 : 2);             // fp32 kernel
    const size_t plane_bytes = a.plane_elems * (e4m3 ? 1 : sizeof(u16));   // wave kernels
    const int* step = a.row_step ? a.row_step : a.step;   // the ROWSTEP instantiations take the rows' steps where the others take *step

    // 2. refusals
    if (a.kmask && !f32) {
        set_error("decode attention: the padding mask exists only in the fp32 kernel (%s)", e4m3 ? "e4m3 K/V cache" : "16-bit K/V cache");
        return RGRG_EINVAL;
    }
    if (a.first && !kv16) {
        set_error("decode attention: the padded-prompt variant exists for the 16-bit K/V cache (%s)",
                  e4m3 ? "e4m3 K/V cache" : "fp32 K/V cache: pass the additive mask");
        return RGRG_EINVAL;
    }
    if (a.row_step && (a.kmask || a.first || a.q_only || e4m3)) {
        set_error("decode attention: the per-row step exists for the fp32 and 16-bit kernels, plain or with an ancestor table (%s)",
                  e4m3 ? "e4m3 K/V cache" : a.q_only ? "q-only" : a.first ? "padded prompt slots" : "padding mask");
        return RGRG_EINVAL;
    }
    if (!f32 && (a.H & 3) != 0) {
        set_error("decode attention: %d heads - the %s K/V cache kernel takes 4 heads per workgroup, the head count must be a multiple of 4",
                  a.H, wave_fmt);
        return RGRG_EINVAL;
    }
    // the wave kernels address the cache rows with 32-bit byte offsets into one layer's K (V) plane through a buffer descriptor,
    // which bounds a plane at 2 GiB (8128 sequences at max_length 128 in 16 bit)
    if (!f32 && plane_bytes >= ((size_t)1 << 31)) {
        set_error("decoder: the %s K/V cache plane of one layer (%zu bytes) exceeds the 2 GiB the attention kernel addresses: "
                  "lower the batch or max_length", wave_fmt, plane_bytes);
        return RGRG_EINVAL;
    }
    if (a.q_only && !f32 && (e4m3 || a.src)) {
        set_error("decode attention: the q-only variant exists for the 16-bit K/V cache without an ancestor table (%s)",
                  a.src ? "beam search" : "e4m3 K/V cache");
        return RGRG_EINVAL;
    }
    if (a.q_only && f32) { set_error("decode attention: the q-only variant exists for the 16-bit K/V cache only"); return RGRG_EINVAL; }
    if (f32 && ni != 9 && ni != 2) { set_error("decode attention: %d keys per group, the kernel is built for 9 and 2", ni); return RGRG_EINVAL; }

    // 3. the variant, 4. the launch
    if (f32) {   // one workgroup per (sequence, head)
        AttnF32Kernel kern = nullptr;
        for (const AttnF32Variant& v : ATTN_F32_VARIANTS)
            if (v.src == (a.src != nullptr) && v.mask == (a.kmask != nullptr) && v.row_step == (a.row_step != nullptr)) kern = ni == 9 ? v.ni9 : v.ni2;
        if (!kern) {
            set_error("decode attention: no fp32 kernel for src %d, mask %d, row_step %d", a.src != nullptr, a.kmask != nullptr, a.row_step != nullptr);
            return RGRG_EINVAL;
        }
        hipLaunchKernelGGL(kern, dim3(a.S * a.H), dim3(256), 0, a.st, a.qkv, a.ld_qkv, static_cast<float*>(a.kc), static_cast<float*>(a.vc), step,
                           a.out, a.S, a.H, a.T, a.src, a.frag_out, a.kmask);
    } else {     // one wave per (sequence, head), or fewer workgroups whose waves walk several
        const int wgs = a.S * a.H / 4, grid = a.max_wgs > 0 ? std::min(wgs, a.max_wgs) : wgs;
        if (e4m3)
            return launch_attn_decode_kv8(a.qkv, a.ld_qkv, static_cast<uint8_t*>(a.kc), static_cast<uint8_t*>(a.vc), a.step, a.out, a.out16,
                                          a.S, a.H, a.T, a.src, a.f16, grid, a.st);
        AttnKv16Kernel kern = nullptr;
        for (const AttnKv16Variant& v : ATTN_KV16_VARIANTS)
            if (v.src == (a.src != nullptr) && v.q_only == a.q_only && v.first == (a.first != nullptr) && v.row_step == (a.row_step != nullptr))
                kern = a.f16 ? v.fp16 : v.bf16;
        if (!kern) {
            set_error("decode attention: no 16-bit kernel for src %d, q_only %d, first %d, row_step %d", a.src != nullptr, (int)a.q_only,
                      a.first != nullptr, a.row_step != nullptr);
            return RGRG_EINVAL;
        }
        // the kernel's `src` parameter doubles as the padded-slot vector when HAS_FIRST && !HAS_SRC; with both, the slots come in `first`
        const int* src_or_first = a.src ? a.src : a.first;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, a.st, a.qkv, a.ld_qkv, static_cast<u16*>(a.kc), static_cast<u16*>(a.vc), step, a.out,
                           a.S, a.H, a.T, src_or_first, a.out16, a.first);
    }
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

}  // namespace rgrg

using namespace rgrg;

// ------------------------------------------------------------------ test hooks
// Each is ONE decode-attention launch on the caller's buffers through the launcher of the product path (launch_attn_decode).
// hook_launch: the argument checks the hooks share and the launch they describe; a hook adds the one or two fields that make its variant.
static int hook_launch(AttnDecodeLaunch& a, const float* qkv, int ld_qkv, int ld_cols, void* kcache, void* vcache, float* out, uint16_t* out16,
                       int S, int H, int T_slots, KvFormat fmt, int fp16, int ni, int max_workgroups, void* stream) {
    RGRG_CHECK_ARG(qkv && kcache && vcache && S > 0 && H > 0 && T_slots >= 2 && ld_qkv >= ld_cols * H * 64);
    RGRG_CHECK_ARG(out || (fmt != KV_F32 && out16));
    RGRG_CHECK_ARG(fmt != KV_F32 || (!out16 && max_workgroups == 0));
    RGRG_CHECK_ARG(fmt == KV_F32 || ni == 0);
    a.qkv = qkv; a.ld_qkv = ld_qkv; a.kc = kcache; a.vc = vcache; a.plane_elems = (size_t)S * H * T_slots * 64;
    a.out = out; a.out16 = out16; a.S = S; a.H = H; a.T = T_slots;
    a.fmt = fmt; a.f16 = fp16 ? 1 : 0; a.ni = ni; a.max_wgs = max_workgroups; a.st = as_stream(stream);
    return RGRG_OK;
}
static KvFormat hook_fmt(int kv16, int fp16) { return kv16 ? (fp16 ? KV_F16 : KV_BF16) : KV_F32; }

// row_step int32 [S] - and, where given, src int32 [S][T_slots] - on the device are read back and checked (one synchronisation):
// 0 <= row_step[s] <= T_slots - 2, the slot a row writes, and every table entry a row can read - slots 0 .. row_step[s] + 1, the last
// one stale but requested - names a row 0 .. S - 1.
static int check_row_step(const char* who, const int* row_step, int S, int T_slots, const int* src, hipStream_t st) {
    std::vector<int> host(S), tab(src ? (size_t)S * T_slots : 0);
    RGRG_HIP(hipStreamSynchronize(st));
    RGRG_HIP(hipMemcpy(host.data(), row_step, (size_t)S * sizeof(int), hipMemcpyDeviceToHost));
    if (src) RGRG_HIP(hipMemcpy(tab.data(), src, tab.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int s = 0; s < S; ++s) {
        if (host[s] < 0 || host[s] > T_slots - 2) {
            set_error("%s: row_step[%d] = %d, a cache of %d slots takes 0 .. %d", who, s, host[s], T_slots, T_slots - 2);
            return RGRG_EINVAL;
        }
        for (int j = 0; src && j <= host[s] + 1; ++j) {
            const int r = tab[(size_t)s * T_slots + j];
            if (r < 0 || r >= S) {
                set_error("%s: src[%d][%d] = %d, the cache has rows 0 .. %d", who, s, j, r, S - 1);
                return RGRG_EINVAL;
            }
        }
    }
    return RGRG_OK;
}

// fp32 or 16-bit cache; plain, with an ancestor table, or (fp32, no table) with the additive padding mask
extern "C" int rgrg_debug_attn_decode(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* step_dev, float* out,
                                      uint16_t* out16, int S, int H, int T_slots, const int* src, const float* kmask, int kv16,
                                      int fp16, int ni, int frag_out, int max_workgroups, void* stream) {
    AttnDecodeLaunch a{};
    RGRG_CHECK_ARG(step_dev && (!kv16 || frag_out == 0));
    if (int rc = hook_launch(a, qkv, ld_qkv, 3, kcache, vcache, out, out16, S, H, T_slots, hook_fmt(kv16, fp16), fp16, ni, max_workgroups, stream)) return rc;
    if (kmask && (kv16 || src)) {   // (mask and table together: rgrg_debug_attn_decode_beam_first)
        set_error("rgrg_debug_attn_decode: the padding mask goes with the fp32 cache and no ancestor table (%s)", kv16 ? "16-bit K/V cache" : "beam search");
        return RGRG_EINVAL;
    }
    a.step = step_dev; a.src = src; a.kmask = kmask; a.frag_out = frag_out ? 1 : 0;
    return launch_attn_decode(a);
}

// The q-only variant of the 16-bit kernel (the many-sequence step behind c_attn's K/V-cache epilogue): q [S][ld_q] fp32, every key
// including slot *step_dev + 1 comes from the cache, nothing is stored to it.
extern "C" int rgrg_debug_attn_decode_qonly(const float* q, int ld_q, const void* kcache, const void* vcache, const int* step_dev, float* out,
                                            uint16_t* out16, int S, int H, int T_slots, int fp16, int max_workgroups, void* stream) {
    AttnDecodeLaunch a{};
    RGRG_CHECK_ARG(step_dev);
    if (int rc = hook_launch(a, q, ld_q, 1, const_cast<void*>(kcache), const_cast<void*>(vcache), out, out16, S, H, T_slots, hook_fmt(1, fp16), fp16, 0,
                             max_workgroups, stream)) return rc;
    a.step = step_dev; a.q_only = true;
    return launch_attn_decode(a);
}

// The padded-prompt variant of the 16-bit kernel (attn_decode_kv16_wave_kernel<false, fp16, q_only, true>, the steps of
// rgrg_decoder_generate_prompted behind a left-padded prompt): first [S] = padded prompt slots of every row.
extern "C" int rgrg_debug_attn_decode_first(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* step_dev, float* out,
                                            uint16_t* out16, int S, int H, int T_slots, const int* first, int fp16, int q_only,
                                            int max_workgroups, void* stream) {
    AttnDecodeLaunch a{};
    RGRG_CHECK_ARG(step_dev && first);
    if (int rc = hook_launch(a, qkv, ld_qkv, q_only ? 1 : 3, kcache, vcache, out, out16, S, H, T_slots, hook_fmt(1, fp16), fp16, 0, max_workgroups, stream))
        return rc;
    a.step = step_dev; a.first = first; a.q_only = q_only != 0;
    return launch_attn_decode(a);
}

// The per-row-step variants (the steps of rgrg_decoder_generate_rolling), on either cache format: attn_decode_kernel<false, ni, false, true> /
// attn_decode_kv16_wave_kernel<false, fp16, false, false, true>.  row_step is checked first (check_row_step).
extern "C" int rgrg_debug_attn_decode_rowstep(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* row_step, float* out,
                                              uint16_t* out16, int S, int H, int T_slots, int kv16, int fp16, int ni, int max_workgroups,
                                              void* stream) {
    AttnDecodeLaunch a{};
    RGRG_CHECK_ARG(row_step);
    if (int rc = hook_launch(a, qkv, ld_qkv, 3, kcache, vcache, out, out16, S, H, T_slots, hook_fmt(kv16, fp16), fp16, ni, max_workgroups, stream)) return rc;
    if (int rc = check_row_step("rgrg_debug_attn_decode_rowstep", row_step, S, T_slots, nullptr, a.st)) return rc;
    a.row_step = row_step;
    return launch_attn_decode(a);
}

// The per-row-step variants WITH an ancestor table (the steps of rgrg_decoder_beam_search_rolling): attn_decode_kernel<true, ni, false, true> /
// attn_decode_kv16_wave_kernel<true, fp16, false, false, true>.  row_step and src [S][T_slots] are checked first (check_row_step).
extern "C" int rgrg_debug_attn_decode_rowstep_src(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* row_step,
                                                  const int* src, float* out, uint16_t* out16, int S, int H, int T_slots, int kv16,
                                                  int fp16, int ni, int max_workgroups, void* stream) {
    AttnDecodeLaunch a{};
    RGRG_CHECK_ARG(row_step && src);
    if (int rc = hook_launch(a, qkv, ld_qkv, 3, kcache, vcache, out, out16, S, H, T_slots, hook_fmt(kv16, fp16), fp16, ni, max_workgroups, stream)) return rc;
    if (int rc = check_row_step("rgrg_debug_attn_decode_rowstep_src", row_step, S, T_slots, src, a.st)) return rc;
    a.row_step = row_step; a.src = src;
    return launch_attn_decode(a);
}

// The two variants of a beam step behind a left-padded prompt (rgrg_decoder_beam_search_prompted): ancestor table src [S][T_slots] AND
// padded prompt slots first [S] (cache slots 1 .. first[s] are left out).  16-bit cache: attn_decode_kv16_wave_kernel<true, fp16, false, true>.
// fp32 cache: attn_decode_kernel<true, ni, true> on the additive mask the product builds from `first` (launch_beam_first_mask), in a
// buffer of the call's own.
extern "C" int rgrg_debug_attn_decode_beam_first(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* step_dev, float* out,
                                                 uint16_t* out16, int S, int H, int T_slots, const int* src, const int* first, int kv16,
                                                 int fp16, int ni, int max_workgroups, void* stream) {
    AttnDecodeLaunch a{};
    RGRG_CHECK_ARG(step_dev && src && first);
    if (int rc = hook_launch(a, qkv, ld_qkv, 3, kcache, vcache, out, out16, S, H, T_slots, hook_fmt(kv16, fp16), fp16, ni, max_workgroups, stream)) return rc;
    a.step = step_dev; a.src = src;
    if (kv16) { a.first = first; return launch_attn_decode(a); }
    float* kmask = nullptr;
    RGRG_HIP(hipMalloc((void**)&kmask, (size_t)S * T_slots * sizeof(float)));
    int rc = launch_beam_first_mask(first, S, T_slots, kmask, a.st);
    a.kmask = kmask;
    if (!rc) rc = launch_attn_decode(a);
    const hipError_t e = hipStreamSynchronize(a.st);   // the mask is the call's own: it must outlive the launch
    (void)hipFree(kmask);
    if (!rc && e != hipSuccess) { set_error("rgrg_debug_attn_decode_beam_first: %s", hipGetErrorString(e)); return RGRG_EHIP; }
    return rc;
}

// An e4m3 cache (attn_decode_kv8_wave_kernel): K / V planes of bytes, out (fp32) or out16 (bf16 / fp16 by `fp16`), exactly as
// launch_attention fills it for a decoder in that format.
extern "C" int rgrg_debug_attn_decode_kv8(const float* qkv, int ld_qkv, uint8_t* kcache, uint8_t* vcache, const int* step_dev, float* out,
                                          uint16_t* out16, int S, int H, int T_slots, const int* src, const float* kmask, int fp16,
                                          int max_workgroups, void* stream) {
    AttnDecodeLaunch a{};
    RGRG_CHECK_ARG(step_dev);
    if (int rc = hook_launch(a, qkv, ld_qkv, 3, kcache, vcache, out, out16, S, H, T_slots, KV_E4M3, fp16, 0, max_workgroups, stream)) return rc;
    a.step = step_dev; a.src = src; a.kmask = kmask;
    return launch_attn_decode(a);
}
