// Decode attention over the opt-in e4m3 K/V cache (rgrg_decoder_set_kv_format): the 8-bit sibling of
// attn_decode_kv16_wave_kernel (decoder.hip).  The cache holds plain OCP e4m3fn bytes, no scales, in the layout of the other
// formats - [sequence][head][slot][64], 64 BYTES per key row.  A WAVE owns one (sequence, head) item; a 4-lane group owns one key
// (one 16-byte load per lane and operand: 8-byte loads stream at 0.54 - 0.70 of the 16-byte rate on this chip, so the row is
// spread over 4 lanes x 16 B rather than 8 x 8 B), a wave covers 16 keys per load instruction and keeps a whole chunk of 16 * NI
// keys (K and V: 2 * NI loads per lane) in flight.  Chunks of 144 keys while more than 144 remain, then one chunk sized to the
// rest in steps of 16 keys (a wave-uniform switch around fully unrolled, unconditional, clamped load blocks); every group keeps
// a running softmax in fp32 and the 16 groups are merged at the end.  The new token's k / v are clamped to +-448, rounded ONCE
// from fp32 (common.h f32x4_to_e4m3_bits), take part as the last key in that rounded form and are stored to slot step + 1.
#include "decoder_internal.h"

namespace rgrg {

typedef float f32x2 __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ __amdgpu_buffer_rsrc_t kv8_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}

struct Kv8Row {  // this lane's 16 dims of the current token's q / k / v (fp32, as c_attn wrote them)
    f32x4 q[4], k[4], v[4];
};
static __device__ __forceinline__ u32x4 kv8_pack_round(const f32x4 (&x)[4]) {  // 16 fp32 -> 16 e4m3 bytes
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = f32x4_to_e4m3_bits(x[e][0], x[e][1], x[e][2], x[e][3]);
    return o;
}

// FIRST: the first chunk of a wave turns the raw q / k / v into q[16] and the packed kn8 / vn8 (after its loads)
template <int NI, bool HAS_SRC, bool FIRST>
static __device__ __forceinline__ void kv8_wave_chunk(const __amdgpu_buffer_rsrc_t kc, const __amdgpu_buffer_rsrc_t vc,
                                                      const int* __restrict__ srow, int s, int hd, int H, int T, int base, int nkeys,
                                                      int slot, int g, int d16, Kv8Row& r, float (&q)[16], u32x4& kn8, u32x4& vn8,
                                                      float& m, float& l, float (&acc)[16]) {
    int rowi[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) rowi[i] = HAS_SRC ? srow[min(base + i * 16 + g, nkeys - 1)] : s;
    u32x4 kk[NI], vv[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int jc = min(base + i * 16 + g, nkeys - 1);
        // 32-bit byte offsets into one layer's K (V) plane through a buffer descriptor (the launcher checks that the plane is
        // < 2 GiB); nt: a cache row is read once per step
        const unsigned off = (unsigned)((rowi[i] * H + hd) * T + jc) * 64u + (unsigned)d16 * 16u;
        kk[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(kc, (int)off, 0, 2));
        vv[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(vc, (int)off, 0, 2));
    }
    // All 2 * NI cache loads are in flight before anything consumes the current token's q / k / v (requested before the cache
    // rows, so they arrive first): the rule of the 16-bit kernel, for its reason - used ahead of the chunk they would make the
    // wave wait for them before it has issued the cache loads, two serialised memory latencies per wave.
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (FIRST) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(r.q[c][e]), "+v"(r.k[c][e]), "+v"(r.v[c][e]));
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) q[4 * c + e] = r.q[c][e];
        }
        kn8 = kv8_pack_round(r.k);
        vn8 = kv8_pack_round(r.v);
    }
    float sc[NI];
    float cmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = base + i * 16 + g;
        if (j == slot) { kk[i] = kn8; vv[i] = vn8; }
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)kk[i][e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)kk[i][e], true);
            dot += (q[4 * e] * lo[0] + q[4 * e + 1] * lo[1]) + (q[4 * e + 2] * hi[0] + q[4 * e + 3] * hi[1]);
        }
        dot += dpp_get<0xB1, 0xf>(dot);
        dot += dpp_get<0x4E, 0xf>(dot);   // sum over the 4 lanes of the group
        sc[i] = j < nkeys ? dot / 8.0f : -INFINITY;
        cmax = fmaxf(cmax, sc[i]);
    }
    const float m_new = fmaxf(m, cmax);
    const float scale = (m == -INFINITY) ? 0.f : expf(m - m_new);  // a group without any key yet keeps m = -inf
    const bool any = m_new != -INFINITY;
    l *= scale;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] *= scale;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = base + i * 16 + g;
        const float pj = (j < nkeys && any) ? expf(sc[i] - m_new) : 0.f;
        l += pj;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int u = j < nkeys ? (int)vv[i][e] : 0;   // a clamped load may hold anything, NaN bytes included
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(u, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(u, true);
            acc[4 * e] += pj * lo[0];
            acc[4 * e + 1] += pj * lo[1];
            acc[4 * e + 2] += pj * hi[0];
            acc[4 * e + 3] += pj * hi[1];
        }
    }
    m = m_new;
}

// F16: the 16-bit type of out16 (the autocast type the attn_proj GEMM reads), nothing else
template <bool HAS_SRC, bool F16>
__global__ __launch_bounds__(256) void attn_decode_kv8_wave_kernel(const float* __restrict__ qkv, int ld_qkv, uint8_t* __restrict__ kc,
                                                                   uint8_t* __restrict__ vc, const int* __restrict__ step,
                                                                   float* __restrict__ out, int S, int H, int T,
                                                                   const int* __restrict__ src, unsigned short* __restrict__ out16) {
    const int lane = threadIdx.x & 63;
    const int t = *step, nkeys = t + 2, slot = t + 1;
    const int g = lane >> 2, d16 = lane & 3;
    const int D = H * 64;
    const __amdgpu_buffer_rsrc_t rk = kv8_rsrc(kc), rv = kv8_rsrc(vc);
    // (sequence, head) items: wave w of workgroup b takes items b * 4 + w, + 4 * gridDim.x, ... (one wave per item, or a capped
    // grid whose waves walk several items: launch_attn_decode)
    for (int item = blockIdx.x * 4 + (threadIdx.x >> 6); item < S * H; item += gridDim.x * 4) {
    const int s = item / H, hd = item - s * H;
    const float* row = qkv + (size_t)s * ld_qkv + hd * 64 + d16 * 16;
    const int* srow = HAS_SRC ? src + (size_t)s * T : nullptr;
    Kv8Row r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        r.q[c] = *reinterpret_cast<const f32x4*>(row + 4 * c);
        r.k[c] = *reinterpret_cast<const f32x4*>(row + D + 4 * c);
        r.v[c] = *reinterpret_cast<const f32x4*>(row + 2 * D + 4 * c);
    }
    float m = -INFINITY, l = 0.f, acc[16], q[16];
    u32x4 kn8, vn8;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#define KV8_CHUNK(NI_, FIRST_, BASE_) \
    kv8_wave_chunk<NI_, HAS_SRC, FIRST_>(rk, rv, srow, s, hd, H, T, BASE_, nkeys, slot, g, d16, r, q, kn8, vn8, m, l, acc)
    // (nkeys >= 2: at least one chunk runs; a key's group and register do not depend on the chunk size)
#define KV8_TAIL(FIRST_, BASE_, REM_)                                                                    \
    switch (((REM_) + 15) >> 4) {                                                                        \
        case 1: KV8_CHUNK(1, FIRST_, BASE_); break;                                                      \
        case 2: KV8_CHUNK(2, FIRST_, BASE_); break;                                                      \
        case 3: KV8_CHUNK(3, FIRST_, BASE_); break;                                                      \
        case 4: KV8_CHUNK(4, FIRST_, BASE_); break;                                                      \
        case 5: KV8_CHUNK(5, FIRST_, BASE_); break;                                                      \
        case 6: KV8_CHUNK(6, FIRST_, BASE_); break;                                                      \
        case 7: KV8_CHUNK(7, FIRST_, BASE_); break;                                                      \
        case 8: KV8_CHUNK(8, FIRST_, BASE_); break;                                                      \
        default: KV8_CHUNK(9, FIRST_, BASE_); break;                                                     \
    }
    if (nkeys > KV8_CHUNK_KEYS) {
        KV8_CHUNK(9, true, 0);
        int base = KV8_CHUNK_KEYS;
        for (; nkeys - base > KV8_CHUNK_KEYS; base += KV8_CHUNK_KEYS) KV8_CHUNK(9, false, base);
        KV8_TAIL(false, base, nkeys - base)
    } else {
        KV8_TAIL(true, 0, nkeys)
    }
#undef KV8_TAIL
#undef KV8_CHUNK
    if (g == 0) {  // the new token's key / value -> cache slot t + 1 (4 lanes x 16 B = the 64-byte row)
        const size_t o = (((size_t)s * H + hd) * T + slot) * 64 + d16 * 16;
        *reinterpret_cast<u32x4*>(kc + o) = kn8;
        *reinterpret_cast<u32x4*>(vc + o) = vn8;
    }
    // merge the 16 groups (lanes with equal d16): lane + 4, + 8 inside a 16-lane row by DPP row rotates, ^ 16 / ^ 32 through the
    // LDS crossbar.  Lanes 0 - 3 (g == 0) store, each from its own sums.
    float M = fmaxf(m, dpp_get<0x124, 0xf>(m));   // row_ror:4
    M = fmaxf(M, dpp_get<0x128, 0xf>(M));         // row_ror:8
    M = fmaxf(M, __shfl_xor(M, 16, 64));
    M = fmaxf(M, __shfl_xor(M, 32, 64));
    const float wgt = (m == -INFINITY) ? 0.f : expf(m - M);  // M is finite: key 0 (the image) always exists
    l *= wgt;
    l += dpp_get<0x124, 0xf>(l);
    l += dpp_get<0x128, 0xf>(l);
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        float o = acc[e] * wgt;
        o += dpp_get<0x124, 0xf>(o);
        o += dpp_get<0x128, 0xf>(o);
        o += __shfl_xor(o, 16, 64);
        o += __shfl_xor(o, 32, 64);
        acc[e] = o / l;
    }
    if (g == 0) {
        const size_t o = (size_t)s * D + hd * 64 + d16 * 16;
        if (out16) {   // feeds the 16-bit attn_proj GEMM only
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                u32x4 pk;
#pragma unroll
                for (int i = 0; i < 4; ++i) pk[i] = to16<F16>(acc[8 * c + 2 * i]) | (to16<F16>(acc[8 * c + 2 * i + 1]) << 16);
                *reinterpret_cast<u32x4*>(out16 + o + 8 * c) = pk;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                *reinterpret_cast<f32x4*>(out + o + 4 * c) = f32x4{acc[4 * c], acc[4 * c + 1], acc[4 * c + 2], acc[4 * c + 3]};
            }
        }
    }
    }   // items
}

int launch_attn_decode_kv8(const float* qkv, int ld_qkv, uint8_t* kc, uint8_t* vc, const int* step, float* out, unsigned short* out16,
                           int S, int H, int T, const int* src, int f16, int workgroups, hipStream_t st) {
    const dim3 grid(workgroups), blk(256);
#define KV8_LAUNCH(SRC_, F16_) \
    hipLaunchKernelGGL((attn_decode_kv8_wave_kernel<SRC_, F16_>), grid, blk, 0, st, qkv, ld_qkv, kc, vc, step, out, S, H, T, src, out16)
    if (src) { if (f16) KV8_LAUNCH(true, true); else KV8_LAUNCH(true, false); }
    else { if (f16) KV8_LAUNCH(false, true); else KV8_LAUNCH(false, false); }
#undef KV8_LAUNCH
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

}  // namespace rgrg
