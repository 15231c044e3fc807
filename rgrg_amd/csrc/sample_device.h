// Device helpers of the row kernels that hold a whole logits row in registers and filter it by temperature, top-k and top-p: the
// token sampler (sample.hip) and the beam-sampling ranking (beam_sample.hip).  One 1024-thread workgroup per row.
//
// * Every logit is read from memory once, with 16-byte loads, and stays in registers: wave w owns the contiguous vocabulary
//   segment [3328 w, 3328 (w + 1)), a lane holds 13 vectors of 4 (vector lane + 64 u of the segment), so a wave-load is 1 KiB
//   contiguous and "vocabulary order" is wave -> vector u -> lane -> element.
// * Both filters are one routine.  With keys that order the logits DESCENDING (flipped IEEE bits, exact), "keep the tokens
//   whose weight of strictly greater logits is <= P" is: delta = max{d : W(d) <= P}, W(d) = weight of the keys < d, keep
//   key <= delta.  Top-k: weight 1, P = k - 1 (the k-th largest logit and everything tied with it).  Top-p: weight = the
//   token's probability mass among the top-k set, P = top_p x total.  delta is found by a radix descent, 8 bits per pass,
//   over a 256-bin histogram in LDS; a thread adds a RUN of equal digits with one atomic, so a peaked row, whose keys share
//   their leading bits, does not serialise 50 000 adds on one bin.
// * DETERMINISM: there is no floating-point atomic and no floating-point sum whose order could vary.  A token's mass is the
//   64-bit fixed-point integer floor(2^40 exp(z - z_max)) (z_max has mass 2^40 exactly, a row's total stays below 2^56), and
//   every accumulation of masses - histogram bins, wave and row totals, running sums - is an integer add: integer adds commute,
//   so the result does not depend on the order in which waves or atomics arrive.  exp is evaluated by the same expression on
//   the same input wherever a mass is needed again, which is what lets the masses stay out of registers.
#pragma once
#include "common.h"

namespace rgrg {

constexpr int SM_THREADS = 1024, SM_WAVES = 16, SM_NV = 13;
constexpr int SM_SEG = 64 * SM_NV * 4;   // vocabulary entries per wave
constexpr float SM_FIX = 1099511627776.0f;   // 2^40

struct SampleParams {   // the device-side block a captured step reads: one graph serves every seed and parameter set
    unsigned long long seed;
    float inv_T;
    int top_k;     // 0: off
    float top_p;   // 1: off
    int pad_;
};

typedef unsigned long long u64;

__device__ __forceinline__ unsigned desc_key(float x) {   // ascending key <=> descending logit; -0 == +0
    const unsigned b = __float_as_uint(x + 0.0f);
    return (b & 0x80000000u) ? b : (b ^ 0x7fffffffu);
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 wave_scan_u64(u64 v, int lane) {   // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    return v;
}

__device__ __forceinline__ float key_logit(unsigned k) {   // the inverse of desc_key
    return __uint_as_float((k & 0x80000000u) ? k : (k ^ 0x7fffffffu));
}
constexpr unsigned SM_NO_TOKEN = 0xffffffffu;   // key of the slots behind the vocabulary (no finite or infinite logit maps to it)
constexpr unsigned SM_KEEP_ALL = 0xfffffffeu;   // "no filter": every key but that one

// z = fp32(x * inv_T), the contract's product: formed with __fmul_rn so that it is never contracted into the subtraction below
__device__ __forceinline__ float token_z(unsigned k, float inv_T) { return __fmul_rn(key_logit(k), inv_T); }
// Fixed-point mass of the token with key k: floor(2^40 exp(z - z_max)).  The ONE definition, called wherever a mass is needed
// (histogram weights, wave totals, vector sums, the element walk): equal inputs give equal bits, which DETERMINISM above and
// the agreement of the vector sums with the element walk rest on.
__device__ __forceinline__ u64 token_mass(unsigned k, float inv_T, float zmax) {
    asm volatile("" : "+v"(k));   // evaluated where it is used: the compiler otherwise keeps all 52 masses of a thread live from
                                  // one use to the next (104 registers) and spills
    const float z = token_z(k, inv_T);
    const float ev = (z == zmax) ? 1.0f : expf(__fsub_rn(z, zmax));
    return (u64)(ev * SM_FIX);
}

// A thread's 52 logits, held as their keys: the filters compare keys, and a logit is two instructions away from its key
struct RowRegs {
    unsigned k[SM_NV][4];
    int base;   // vocabulary index of k[0][0]; k[u][e] is base + 256 u + e
    float inv_T, zmax;
    __device__ __forceinline__ u64 mass(int u, int e) const { return token_mass(k[u][e], inv_T, zmax); }
};

// delta = max{d : W(d) <= P} (see the head of the file); w(u, e) is the weight of a token that takes part, called only for
// tokens with key <= limit
template <class WF>
__device__ __forceinline__ unsigned radix_threshold(const RowRegs& r, unsigned limit, u64 P, WF&& w, u64* hist, u64* sh_a,
                                                    unsigned* sh_prefix) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0;
    u64 A = 0;   // weight of the keys below the prefix
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned himask = pass ? (0xffffffffu << (shift + 8)) : 0u;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        unsigned lim = limit;
        asm volatile("" : "+v"(lim));   // opaque per pass: hoisting the 52 pass-invariant compares out of the loop spills their masks
        int cur = 0;
        u64 acc = 0;
#pragma unroll
        for (int u = 0; u < SM_NV; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned k = r.k[u][e];
                if (k <= lim && (k & himask) == prefix) {
                    const int b = (int)((k >> shift) & 255u);
                    if (b != cur) {
                        if (acc) atomicAdd(&hist[cur], acc);
                        cur = b;
                        acc = 0;
                    }
                    acc += w(u, e);
                }
            }
        if (acc) atomicAdd(&hist[cur], acc);
        __syncthreads();
        if (wave == 0) {   // the largest bin b with A + (weight of the bins below b) <= P; bin 0 always qualifies
            const u64 h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const u64 s = (h0 + h1) + (h2 + h3);
            const u64 below = A + (wave_scan_u64(s, lane) - s);
            const u64 m = __ballot(below <= P);
            const int L = 63 - __clzll((long long)m);
            if (lane == L) {
                u64 a = below;
                int b = 4 * lane;
                if (a + h0 <= P) { a += h0; ++b;
                    if (a + h1 <= P) { a += h1; ++b;
                        if (a + h2 <= P) { a += h2; ++b; } } }
                *sh_a = a;
                *sh_prefix = prefix | ((unsigned)b << shift);
            }
        }
        __syncthreads();
        A = *sh_a;
        prefix = *sh_prefix;
    }
    return prefix;
}

}  // namespace rgrg
