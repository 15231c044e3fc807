// Token sampling on the device: temperature, top-k, top-p, one inverse-CDF draw and its log-probability per logits row, in
// ONE launch (contract: include/rgrg_hip.h "Sampling").  One 1024-thread workgroup per row.  The row in registers,
// the two filters and the fixed-point masses that make the result deterministic are in sample_device.h (shared with the
// beam-sampling ranking, beam_sample.hip); here: the draw (sample_row), for the rows of a lock-step decode step or of caller-provided logits
// (sample_kernel) and for the rows of rolling-batch sampling (roll_sample_kernel).  "Vocabulary order" is wave -> vector u -> lane -> element, so the
// inverse-CDF scan needs one wave's prefix only.  The draw compares integers: running sum > floor(w24 x total / 2^24),
// u = w24 2^-24.
#include "decoder_internal.h"
#include "sample_device.h"

namespace rgrg {

// The draw of one logits row x[0..V) by its workgroup of SM_THREADS threads, every thread of which calls this: filters, masses and
// the inverse-CDF scan under the Philox counter (rr, t).  -> true in the ONE lane that holds the result (*tok, *logq); every other
// thread returns false.  The body of sample_kernel and of roll_sample_kernel.
template <bool VEC>
__device__ __forceinline__ bool sample_row(const float* __restrict__ x, int V, const SampleParams& prm, unsigned rr, unsigned t,
                                           int* tok_out, float* logq_out) {
    __shared__ u64 hist[256];
    __shared__ u64 sh_w[SM_WAVES];
    __shared__ unsigned sh_k[SM_WAVES];
    __shared__ u64 sh_a;
    __shared__ unsigned sh_prefix;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

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
    r.zmax = token_z(kmin, r.inv_T);

    // top-k: the k-th largest logit and its ties
    unsigned limit = SM_KEEP_ALL;
    if (prm.top_k == 1) limit = kmin;
    else if (prm.top_k > 1 && prm.top_k < V)
        limit = min(limit, radix_threshold(r, limit, (u64)(prm.top_k - 1), [](int, int) -> u64 { return 1; }, hist, &sh_a, &sh_prefix));

    // masses of the kept tokens per wave -> row total
    auto wave_totals = [&](unsigned lim) -> u64 {
        u64 s = 0;
#pragma unroll
        for (int u = 0; u < SM_NV; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (r.k[u][e] <= lim) s += r.mass(u, e);
        s = wave_sum_u64(s);
        __syncthreads();   // the previous readers of sh_w are done
        if (lane == 0) sh_w[wave] = s;
        __syncthreads();
        u64 tot = 0;
#pragma unroll
        for (int w = 0; w < SM_WAVES; ++w) tot += sh_w[w];
        return tot;
    };
    u64 total = wave_totals(limit);
    if (prm.top_p < 1.0f) {   // top-p on the distribution re-normalised over the top-k set
        const u64 P = (u64)((double)total * (double)prm.top_p);
        const unsigned dp = radix_threshold(r, limit, P, [&](int u, int e) -> u64 { return r.mass(u, e); }, hist, &sh_a, &sh_prefix);
        limit = dp < limit ? dp : limit;
        total = wave_totals(limit);
    }

    // the draw: first kept token, in vocabulary order, whose running mass exceeds u x total.  top_k == 1: the first kept token
    // (first-occurrence arg-max, what greedy returns)
    const unsigned w24 = prm.top_k == 1 ? 0u : philox4x32_10_first(rr, t, 0u, 0u, (unsigned)prm.seed, (unsigned)(prm.seed >> 32)) >> 8;
    const u64 T = (__umul64hi(total, (u64)w24) << 40) | ((total * (u64)w24) >> 24);   // floor(w24 total / 2^24) < total
    u64 run = 0;
    int wsel = 0;
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w) {
        const bool before = run + sh_w[w] <= T;   // the crossing is behind wave w
        if (before && wsel == w) { run += sh_w[w]; wsel = w + 1; }
    }
    if (wave != wsel) return false;   // (wsel < SM_WAVES: the running mass reaches total > T)
    u64 s[SM_NV];
#pragma unroll
    for (int u = 0; u < SM_NV; ++u) {
        s[u] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (r.k[u][e] <= limit) s[u] += r.mass(u, e);
    }
    int usel = 0;
    u64 lane_s = 0;
    bool open = true;
#pragma unroll
    for (int u = 0; u < SM_NV; ++u) {
        const u64 c = wave_sum_u64(s[u]);
        if (open) {
            if (run + c <= T) run += c;
            else { open = false; usel = u; lane_s = s[u]; }
        }
    }
    const u64 incl = run + wave_scan_u64(lane_s, lane);
    const u64 hit = __ballot(incl > T);
    const int L = __ffsll((long long)hit) - 1;
    if (lane != L) return false;
    u64 c = incl - lane_s;
    unsigned kv[4];
#pragma unroll
    for (int u = 0; u < SM_NV; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (u == 0 || u == usel) kv[e] = r.k[u][e];
    // The lane's kept tokens sum to lane_s (token_mass both times) and c + lane_s = incl > T, so the walk crosses T at one of
    // them; should it ever not, the lane's LAST kept token is taken - a kept token, never an index outside the kept set.
    int tok = 0;
    unsigned ksel = SM_NO_TOKEN;
    bool found = false;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (!found && kv[e] <= limit) {
            c += token_mass(kv[e], r.inv_T, r.zmax);
            tok = r.base + 256 * usel + e;
            ksel = kv[e];
            found = c > T;
        }
    const float z = token_z(ksel, r.inv_T);
    // log q(token) under the distribution it was drawn from
    // (one lane, once per row: in double, so that the fp32 result carries one rounding and not those of z - z_max, of the
    // conversion of the total and of logf - together 2 ulp, measured against the float64 reference)
    const double logq_d = ((z == r.zmax) ? 0.0 : ((double)z - (double)r.zmax)) - (log((double)total) - 40.0 * 0.6931471805599453);
    *tok_out = tok;
    *logq_out = (float)logq_d;
    return true;
}

// logits [S][ld]; prm_dev (or, when null, prm_val) = the parameters; the Philox counter is (row0 + row, t) with t = *bk.step in
// a decode step (bk.ids != null: the token and its log-prob go through record_step_token into ids / lp[row][t + 1]) and
// t = step otherwise (out_tok / out_lp [S]).
template <bool VEC>
__global__ __launch_bounds__(SM_THREADS) void sample_kernel(const float* __restrict__ logits, size_t ld, int V,
                                                            const SampleParams* __restrict__ prm_dev, SampleParams prm_val, int step,
                                                            int row0, int* __restrict__ out_tok, float* __restrict__ out_lp,
                                                            StepBook bk, float* __restrict__ lp, int ld_lp) {
    const int row = blockIdx.x;
    const SampleParams prm = prm_dev ? *prm_dev : prm_val;
    const int t = bk.ids ? *bk.step : step;
    int tok;
    float logq;
    if (!sample_row<VEC>(logits + (size_t)row * ld, V, prm, (unsigned)(row0 + row), (unsigned)t, &tok, &logq)) return;
    if (bk.ids) {
        bool was_finished;
        record_step_token(bk, row, t, tok, &was_finished);
        if (lp) lp[(size_t)row * ld_lp + t + 1] = was_finished ? 0.0f : logq;
    } else {
        out_tok[row] = tok;
        if (out_lp) out_lp[row] = logq;
    }
}

// The rolling sampler (rolling-batch sampling, decoder_roll.hip): row r holds sequence row_seq[r] at row_len[r] tokens and draws the
// token of column len under the counter (sequence, len - 1) - the counter of sample_kernel for row = sequence at step len - 1, so
// neither the decoder row nor the step of the call enters the draw.  The token goes to arg[r] (roll_retire_kernel appends it), the
// log-prob to the sequence's own output row.  An idle row (sequence < 0) leaves as a whole workgroup before the first barrier.
template <bool VEC>
__global__ __launch_bounds__(SM_THREADS) void roll_sample_kernel(const float* __restrict__ logits, size_t ld, int V,
                                                                 const SampleParams* __restrict__ prm_dev, const int* __restrict__ row_seq,
                                                                 const int* __restrict__ row_len, const RollCall* __restrict__ call,
                                                                 int* __restrict__ arg) {
    const int row = blockIdx.x;
    const int seq = row_seq[row];
    if (seq < 0) return;
    const int len = row_len[row];
    const int slot = seq % call->C;   // the sequence's ring row (a one-shot call: C = S, the row itself)
    // A session: the parameters and the counter row seq - q0 are those of the sequence's request; else the step's block
    SampleParams prm;
    unsigned rr = (unsigned)seq;
    if (const RollReq* ring = call->req) {
        const RollReq q = ring[slot];
        prm = SampleParams{q.seed, q.inv_T, q.top_k, q.top_p, 0};
        rr = (unsigned)(seq - q.q0);
    } else {
        prm = *prm_dev;
    }
    int tok;
    float logq;
    if (!sample_row<VEC>(logits + (size_t)row * ld, V, prm, rr, (unsigned)(len - 1), &tok, &logq)) return;
    arg[row] = tok;
    float* lp = call->lp;
    if (lp) lp[(size_t)slot * call->ld + len] = logq;
}

static int launch_sample(const float* logits, size_t ld, int S, int V, const SampleParams* prm_dev, SampleParams prm_val, int step,
                         int row0, int* out_tok, float* out_lp, StepBook bk, float* lp, int ld_lp, hipStream_t st) {
    RGRG_CHECK_ARG(logits && S > 0 && V > 0 && V <= SM_WAVES * SM_SEG && ld >= (size_t)V);
    const bool vec = (ld % 4 == 0) && (reinterpret_cast<uintptr_t>(logits) % 16 == 0);
    if (vec)
        hipLaunchKernelGGL(sample_kernel<true>, dim3(S), dim3(SM_THREADS), 0, st, logits, ld, V, prm_dev, prm_val, step, row0, out_tok,
                           out_lp, bk, lp, ld_lp);
    else
        hipLaunchKernelGGL(sample_kernel<false>, dim3(S), dim3(SM_THREADS), 0, st, logits, ld, V, prm_dev, prm_val, step, row0, out_tok,
                           out_lp, bk, lp, ld_lp);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

int launch_roll_sample(const float* logits, size_t ld, int R, int V, const void* prm_dev, const int* row_seq, const int* row_len,
                       const RollCall* call, int* arg, hipStream_t st) {
    RGRG_CHECK_ARG(logits && R > 0 && V > 0 && V <= SM_WAVES * SM_SEG && ld >= (size_t)V && prm_dev && row_seq && row_len && call && arg);
    const SampleParams* prm = static_cast<const SampleParams*>(prm_dev);
    const bool vec = (ld % 4 == 0) && (reinterpret_cast<uintptr_t>(logits) % 16 == 0);
    if (vec) hipLaunchKernelGGL(roll_sample_kernel<true>, dim3(R), dim3(SM_THREADS), 0, st, logits, ld, V, prm, row_seq, row_len, call, arg);
    else hipLaunchKernelGGL(roll_sample_kernel<false>, dim3(R), dim3(SM_THREADS), 0, st, logits, ld, V, prm, row_seq, row_len, call, arg);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

__global__ void sample_set_params_kernel(SampleParams* dst, SampleParams v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v;
}

static int check_sample_args(float temperature, int top_k, float top_p) {
    RGRG_CHECK_ARG(temperature > 0.f && top_k >= 0 && top_p > 0.f && top_p <= 1.0f);
    return RGRG_OK;
}

size_t sample_params_bytes() { return sizeof(SampleParams); }

int enqueue_sample_params(void* prm_dev, float temperature, int top_k, float top_p, unsigned long long seed, hipStream_t st) {
    int rc = check_sample_args(temperature, top_k, top_p);
    if (rc) return rc;
    const SampleParams v{seed, 1.0f / temperature, top_k, top_p, 0};
    hipLaunchKernelGGL(sample_set_params_kernel, dim3(1), dim3(64), 0, st, static_cast<SampleParams*>(prm_dev), v);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

int launch_sample_step(const float* logits, int ld, int S, int V, const void* prm_dev, long long* ids, int ld_ids, int* finished,
                       int* step, int* done_len, int* sync, float* lp, int ld_lp, hipStream_t st) {
    RGRG_CHECK_ARG(prm_dev && ids && finished && step && done_len && sync);
    const StepBook bk{ids, ld_ids, finished, step, done_len, sync, S};
    return launch_sample(logits, (size_t)ld, S, V, static_cast<const SampleParams*>(prm_dev), SampleParams{}, 0, 0, nullptr, nullptr, bk,
                         lp, ld_lp, st);
}

}  // namespace rgrg

using namespace rgrg;

extern "C" int rgrg_sample_logits_f32(const float* logits, int64_t ld, int S, int V, float temperature, int top_k, float top_p,
                                      uint64_t seed, int step, int row0, int* out_tok, float* out_logprob, void* stream) {
    RGRG_CHECK_ARG(out_tok && ld > 0 && step >= 0 && row0 >= 0);
    int rc = check_sample_args(temperature, top_k, top_p);
    if (rc) return rc;
    const SampleParams v{seed, 1.0f / temperature, top_k, top_p, 0};
    return launch_sample(logits, (size_t)ld, S, V, nullptr, v, step, row0, out_tok, out_logprob, StepBook{}, nullptr, 0, as_stream(stream));
}
