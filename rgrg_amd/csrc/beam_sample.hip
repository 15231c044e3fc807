// Beam-search sampling: the ranking behind a beam step that DRAWS its K = 2 num_beams candidates per item without replacement from
// the joint distribution over the item's num_beams x V continuations (contract: include/rgrg_hip.h "Beam-search sampling";
// DESIGN.md 7.12).  Gumbel top-k: independent Gumbel noise g on every kept continuation's score s, the K largest keys s + g ARE K
// sequential draws without replacement from softmax(s) (Plackett-Luce) - one pass over the logits, no loop of dependent draws.
//
// beam_sample_row_kernel, one 1024-thread workgroup per beam row: the row in registers and the two filters as in the token sampler
// (sample_device.h); then every held logit is replaced IN PLACE by its key (a filtered one by -inf) and K rounds of a workgroup
// arg-max pop the row's K largest keys.  A thread keeps the arg-max of its own 52 values between rounds: only the winner's wave
// rescans its registers, the others bring their cached head to the butterfly.  Nothing is accumulated in an order that could vary
// (the fp32 sums run per thread, per wave butterfly, then over the 16 waves in wave order), so equal inputs give equal bits.
// beam_sample_item_kernel, one workgroup per item: the K largest keys of the item's num_beams x K row candidates, ordered by s.
#include "decoder_internal.h"
#include "sample_device.h"

namespace rgrg {

constexpr unsigned BS_FINITE_KEYS = 0xff7fffffu;   // desc_key(-FLT_MAX): every key above it is -inf, NaN or a slot behind V
constexpr unsigned BS_NEG_INF = 0xff800000u;       // the float -inf

// s of a kept token (the contract's expression, every operation rounded once): beam_score + ((x - max) - logsum) * inv_T.  The ONE
// definition: the key is formed from it and the winner's s is recomputed by it, so a candidate's key is its s plus its noise.
__device__ __forceinline__ float beam_sample_score(float x, float m, float logsum, float inv_T, float beam_score) {
    return __fadd_rn(beam_score, __fmul_rn(__fsub_rn(__fsub_rn(x, m), logsum), inv_T));
}
// g = -log(-log u), u = (n + 0.5) 2^-24 for the 24-bit n.  u is never rounded: below one half it is an fp32 number, above it
// 1 - u = (2^24 - n - 0.5) 2^-24 is, and -log u = -log1p(-(1 - u)) - rounding u itself would make the largest n draw u = 1, g = +inf.
__device__ __forceinline__ float gumbel_noise(unsigned word) {
    const unsigned n = word >> 8;
    const float a = n < 0x800000u ? -logf(((float)n + 0.5f) * 0x1p-24f) : -log1pf(-(((float)(0xffffffu - n) + 0.5f) * 0x1p-24f));
    return -logf(a);
}

// the arg-max of a thread's registers read as floats (value descending, ties to the lower token: the scan ascends)
__device__ __forceinline__ void thread_head(const RowRegs& r, float& bv, int& bi) {
    bv = -INFINITY;
    int slot = -1;   // 256 u + e: constants, where base + 256 u + e would be 52 loop-invariant registers to the compiler
#pragma unroll
    for (int u = 0; u < SM_NV; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = __uint_as_float(r.k[u][e]);
            if (v > bv) { bv = v; slot = 256 * u + e; }
        }
    bi = slot < 0 ? 0x7fffffff : r.base + slot;
}

// logits [rows][ld]; prm_dev (or, when null, prm_val) = the parameters; t = *step_dev (a decode step) or step.  Row `row` draws its
// noise from the Philox counter (row0 + row, t, token >> 2, 1).  -> row_key / row_s / row_tok [rows][BEAM_K]: the K largest keys of
// the row, key descending (ties to the lower token), with their s and token; a row with fewer than K kept tokens ends in
// (-inf, -inf, 0) entries.
template <bool VEC>
__global__ __launch_bounds__(SM_THREADS) void beam_sample_row_kernel(const float* __restrict__ logits, size_t ld, int V, int K,
                                                                     const float* __restrict__ beam_scores,
                                                                     const SampleParams* __restrict__ prm_dev, SampleParams prm_val,
                                                                     const int* __restrict__ step_dev, int step, int row0,
                                                                     float* __restrict__ row_key, float* __restrict__ row_s,
                                                                     int* __restrict__ row_tok) {
    __shared__ u64 hist[256];
    __shared__ u64 sh_w[SM_WAVES];
    __shared__ unsigned sh_k[SM_WAVES];
    __shared__ float sh_f[SM_WAVES];
    __shared__ u64 sh_a;
    __shared__ unsigned sh_prefix;
    __shared__ float wv[2][SM_WAVES];
    __shared__ int wi[2][SM_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SampleParams prm = prm_dev ? *prm_dev : prm_val;
    const int t = step_dev ? *step_dev : step;
    const float* __restrict__ x = logits + (size_t)row * ld;
    const float bscore = beam_scores[row];

    RowRegs r;
    r.base = wave * SM_SEG + lane * 4;
    r.inv_T = prm.inv_T;
#pragma unroll
    for (int u = 0; u < SM_NV; ++u) {
        const int i = r.base + 256 * u;
        if (VEC && i + 3 < V) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) r.k[u][e] = desc_key(v[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) r.k[u][e] = (i + e < V) ? desc_key(x[i + e]) : SM_NO_TOKEN;
        }
    }
    // row maximum = the smallest key (exact, any order)
    unsigned kmin = SM_NO_TOKEN;
#pragma unroll
    for (int u = 0; u < SM_NV; ++u) kmin = min(min(kmin, min(r.k[u][0], r.k[u][1])), min(r.k[u][2], r.k[u][3]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, 64));
    if (lane == 0) sh_k[wave] = kmin;
    __syncthreads();
    kmin = sh_k[0];
#pragma unroll
    for (int w = 1; w < SM_WAVES; ++w) kmin = min(kmin, sh_k[w]);
    kmin = __builtin_amdgcn_readfirstlane(kmin);   // row-uniform values read back from LDS go to scalar registers: the vector ones are all taken
    r.zmax = token_z(kmin, r.inv_T);
    const float m = key_logit(kmin);

    // log of the row's sum of exp(x - max): per thread in register order, per wave by butterfly, the 16 waves in wave order
    float ssum = 0.f;
#pragma unroll
    for (int u = 0; u < SM_NV; ++u) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (r.k[u][e] != SM_NO_TOKEN) ssum += expf(key_logit(r.k[u][e]) - m);
        asm volatile("" : "+v"(ssum));   // one vector after the other: 52 exponentials in flight at once spill
    }
    ssum = wave_sum(ssum);
    if (lane == 0) sh_f[wave] = ssum;
    __syncthreads();
    ssum = sh_f[0];
#pragma unroll
    for (int w = 1; w < SM_WAVES; ++w) ssum += sh_f[w];
    const float logsum = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(logf(ssum))));

    // the kept set: the sampler's top-k, then top-p, with min_tokens_to_keep = 2; a -inf logit is never kept
    const auto count = [](int, int) -> u64 { return 1; };
    const int top_k = prm.top_k == 1 ? 2 : prm.top_k;
    unsigned limit = BS_FINITE_KEYS;
    if (top_k > 1 && top_k < V) limit = min(limit, radix_threshold(r, limit, (u64)(top_k - 1), count, hist, &sh_a, &sh_prefix));
    if (prm.top_p < 1.0f) {   // top-p on the distribution re-normalised over the top-k set; the two largest logits (and the ties of the second) stay
        u64 total = 0;   // masses of the top-k set: integer adds, any order
#pragma unroll
        for (int u = 0; u < SM_NV; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (r.k[u][e] <= limit) total += r.mass(u, e);
        total = wave_sum_u64(total);
        if (lane == 0) sh_w[wave] = total;
        __syncthreads();
        total = 0;
#pragma unroll
        for (int w = 0; w < SM_WAVES; ++w) total += sh_w[w];
        const u64 P = (u64)((double)total * (double)prm.top_p);
        const unsigned dp = radix_threshold(r, limit, P, [&](int u, int e) -> u64 { return r.mass(u, e); }, hist, &sh_a, &sh_prefix);
        const unsigned two = top_k == 2 ? limit : radix_threshold(r, limit, (u64)1, count, hist, &sh_a, &sh_prefix);
        limit = min(limit, max(dp, two));
    }
    limit = __builtin_amdgcn_readfirstlane(limit);

    // every held value becomes its key s + g (one Philox call per four tokens), a filtered one -inf
    const unsigned rr = (unsigned)(row0 + row);
#pragma unroll
    for (int u = 0; u < SM_NV; ++u) {
        asm volatile("" : "+v"(r.k[u][0]), "+v"(r.k[u][1]), "+v"(r.k[u][2]), "+v"(r.k[u][3]));   // one vector after the other, as above
        const bool any = r.k[u][0] <= limit || r.k[u][1] <= limit || r.k[u][2] <= limit || r.k[u][3] <= limit;
        if (any) {
            const Philox4 w = philox4x32_10(rr, (unsigned)t, (unsigned)((r.base + 256 * u) >> 2), 1u, (unsigned)prm.seed,
                                            (unsigned)(prm.seed >> 32));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned k = r.k[u][e];
                const float s = beam_sample_score(key_logit(k), m, logsum, r.inv_T, bscore);
                r.k[u][e] = k <= limit ? __float_as_uint(__fadd_rn(s, gumbel_noise(w.w[e]))) : BS_NEG_INF;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) r.k[u][e] = BS_NEG_INF;
        }
    }

    // K rounds: workgroup arg-max over the threads' heads (key descending, ties to the lower token); the winner's thread writes the
    // entry, drops the value and rescans.  wv / wi alternate between rounds: one barrier per round.
    float hv;
    int hi;
    thread_head(r, hv, hi);
    for (int round = 0; round < K; ++round) {
        float bv = hv;
        int bi = hi;
        int self = lane;
        asm volatile("" : "+v"(self));   // the six partner addresses are formed per round: shared with the butterflies in front of
                                         // the filters they stay live through them, and that costs the registers the filters need
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int partner = (self ^ o) << 2;
            const float ov = __int_as_float(__builtin_amdgcn_ds_bpermute(partner, __float_as_int(bv)));
            const int oi = __builtin_amdgcn_ds_bpermute(partner, bi);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        const int p = round & 1;
        if (lane == 0) { wv[p][wave] = bv; wi[p][wave] = bi; }
        __syncthreads();
        bv = wv[p][0]; bi = wi[p][0];
#pragma unroll
        for (int w = 1; w < SM_WAVES; ++w)
            if (wv[p][w] > bv || (wv[p][w] == bv && wi[p][w] < bi)) { bv = wv[p][w]; bi = wi[p][w]; }
        const size_t o = (size_t)row * BEAM_K + round;
        if (bv == -INFINITY) {   // the kept set is exhausted (every thread sees it)
            if (tid == 0) { row_key[o] = -INFINITY; row_s[o] = -INFINITY; row_tok[o] = 0; }
        } else if (hi == bi) {   // tokens are distinct: the one thread that holds the winner
            row_key[o] = bv;
            row_s[o] = beam_sample_score(x[bi], m, logsum, r.inv_T, bscore);
            row_tok[o] = bi;
            const int slot = bi - r.base;
#pragma unroll
            for (int u = 0; u < SM_NV; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (slot == 256 * u + e) r.k[u][e] = BS_NEG_INF;
            thread_head(r, hv, hi);
        }
    }
}

// Per item: the nb * K row candidates (row lists BEAM_K wide, as the row kernel leaves them), one thread each, ranked against all
// others through LDS: the K largest keys (ties: lower flat index beam * V + token), written in the order s descending (ties: lower
// flat index) -> out_score (= s) / out_tok / out_beam [item][K], the buffers BeamSearchScorer.process reads.  An exhausted entry
// (-inf) ranks behind every finite key; an item holds >= K finite ones, since every row keeps two tokens.
__global__ __launch_bounds__(BEAM_K * BEAM_K / 2) void beam_sample_item_kernel(const float* __restrict__ row_key, const float* __restrict__ row_s,
                                                                               const int* __restrict__ row_tok, int nb, int K, int V,
                                                                               float* __restrict__ out_score, int* __restrict__ out_tok,
                                                                               int* __restrict__ out_beam) {
    constexpr int N = BEAM_K * BEAM_K / 2;   // nb * 2 nb <= 512 for nb <= 16
    __shared__ float skey[N];
    __shared__ float ssc[N];
    __shared__ long long sflat[N];
    const int item = blockIdx.x, tid = threadIdx.x;
    const int n = nb * K;
    float key = -INFINITY, sc = -INFINITY;
    long long flat = 0x7fffffffffffLL;
    int tok = 0, b = 0;
    if (tid < n) {
        b = tid / K;
        const size_t o = (size_t)(item * nb + b) * BEAM_K + (tid - b * K);
        key = row_key[o];
        sc = row_s[o];
        tok = row_tok[o];
        if (key > -INFINITY) flat = (long long)b * V + tok;
    }
    skey[tid] = key;
    sflat[tid] = flat;
    __syncthreads();
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const float oj = skey[j];
        const long long fj = sflat[j];
        if (oj > key || (oj == key && fj < flat)) ++rank;
    }
    const bool chosen = tid < n && rank < K;
    ssc[tid] = chosen ? sc : -INFINITY;
    if (!chosen) flat = 0x7fffffffffffLL;
    __syncthreads();   // every thread has read the flat indices it ranks its key by
    sflat[tid] = flat;
    __syncthreads();
    if (!chosen) return;
    int pos = 0;   // among the chosen: the others hold -inf and the largest flat index
    for (int j = 0; j < n; ++j) {
        const float oj = ssc[j];
        const long long fj = sflat[j];
        if (oj > sc || (oj == sc && fj < flat)) ++pos;
    }
    if (pos < K) {   // always, for K chosen entries with distinct (s, flat); kept as the bound of the three stores
        out_score[item * K + pos] = sc;
        out_tok[item * K + pos] = tok;
        out_beam[item * K + pos] = b;
    }
}

// The two launches of the beam-sampling ranking, shared by beam_search_run and the test hook.  t = *step_dev, or `step` when null.
int launch_beam_sample_rank(const float* logits, size_t ld, int V, int S, int nb, const float* beam_scores, const void* prm_dev,
                            const void* prm_val, const int* step_dev, int step, int row0, float* row_key, float* row_s, int* row_tok,
                            float* out_score, int* out_tok, int* out_beam, hipStream_t st) {
    RGRG_CHECK_ARG(logits && beam_scores && (prm_dev || prm_val) && row_key && row_s && row_tok && out_score && out_tok && out_beam);
    RGRG_CHECK_ARG(S > 0 && nb >= 1 && nb <= BEAM_K / 2 && V >= 2 && V <= SM_WAVES * SM_SEG && ld >= (size_t)V);
    const int K = 2 * nb, rows = S * nb;
    const SampleParams pv = prm_val ? *static_cast<const SampleParams*>(prm_val) : SampleParams{};
    const SampleParams* pd = static_cast<const SampleParams*>(prm_dev);
    const bool vec = (ld % 4 == 0) && (reinterpret_cast<uintptr_t>(logits) % 16 == 0);
    if (vec)
        hipLaunchKernelGGL(beam_sample_row_kernel<true>, dim3(rows), dim3(SM_THREADS), 0, st, logits, ld, V, K, beam_scores, pd, pv, step_dev,
                           step, row0, row_key, row_s, row_tok);
    else
        hipLaunchKernelGGL(beam_sample_row_kernel<false>, dim3(rows), dim3(SM_THREADS), 0, st, logits, ld, V, K, beam_scores, pd, pv, step_dev,
                           step, row0, row_key, row_s, row_tok);
    RGRG_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_sample_item_kernel, dim3(S), dim3(BEAM_K * BEAM_K / 2), 0, st, row_key, row_s, row_tok, nb, K, V, out_score,
                       out_tok, out_beam);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

}  // namespace rgrg

using namespace rgrg;

extern "C" int rgrg_debug_beam_sample_rank(const float* logits, int64_t ld, int V, int S, int nb, const float* beam_scores, float temperature,
                                           int top_k, float top_p, uint64_t seed, int step, int row0, float* out_score, int* out_tok,
                                           int* out_beam, float* row_key, float* row_s, int* row_tok, void* stream) {
    RGRG_CHECK_ARG(ld > 0 && step >= 0 && row0 >= 0 && S > 0 && S <= 65535 && nb >= 1 && nb <= BEAM_K / 2);
    RGRG_CHECK_ARG(temperature > 0.f && top_k >= 0 && top_p > 0.f && top_p <= 1.0f);
    RGRG_CHECK_ARG((row_key != nullptr) == (row_s != nullptr) && (row_key != nullptr) == (row_tok != nullptr));
    hipStream_t st = as_stream(stream);
    const size_t n = (size_t)S * nb * BEAM_K;
    float* own = nullptr;   // the row lists, when the caller does not ask for them
    if (!row_key) {
        RGRG_HIP(hipMalloc((void**)&own, n * 3 * sizeof(float)));
        row_key = own; row_s = own + n; row_tok = reinterpret_cast<int*>(own + 2 * n);
    }
    const SampleParams v{seed, 1.0f / temperature, top_k, top_p, 0};
    int rc = launch_beam_sample_rank(logits, (size_t)ld, V, S, nb, beam_scores, nullptr, &v, nullptr, step, row0, row_key, row_s, row_tok,
                                     out_score, out_tok, out_beam, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (own) (void)hipFree(own);
    if (!rc && e != hipSuccess) { set_error("rgrg_debug_beam_sample_rank: %s", hipGetErrorString(e)); rc = RGRG_EHIP; }
    return rc;
}
