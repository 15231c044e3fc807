// Beam search of the RGRG decoder (LanguageModel.generate with num_beams > 1 -> beam_search of ttanida/rgrg):
// the ranking / merge / ancestor-table kernels and the host-side restatement of transformers' BeamSearchScorer.
// A beam step is the decode step of decoder.hip (enqueue_step) whose StepSpec names the beam tokens, the ancestor table and
// STEP_BEAM; the ranking behind it is captured into the step's graph (step_graph).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "decoder_internal.h"

namespace rgrg {

// ------------------------------------------------------------------ beam search kernels
// Per beam row: max, log-sum-exp and the top-K (value desc, token asc on ties) logits.
// log_softmax is monotonic within a row, so the row's best continuations are its top logits.
// Round 6: 1024 threads per row and candidate lists of LIST = 8 / 16 / 32 >= K entries (the scripts' 4 beams need 8): the round-5
// kernel - 256 threads, lists of 32 - took 204 us per step at 116 beam rows (11 % of the step): a wave runs the whole 31-step
// insertion chain whenever ONE of its lanes inserts, i.e. for nearly every one of its 196 elements per lane.
constexpr int BEAM_ROW_THREADS = 1024;
// max and sum of exp(x - max) of a row, the same value in every thread (fixed order: strided per thread, butterflies per wave, the 16
// wave sums in wave order)
template <int THREADS>
__device__ __forceinline__ void beam_row_max_sumexp(const float* __restrict__ x, int V, float* sh, float& m_out, float& ssum_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m = -INFINITY;
    for (int i = tid; i < V; i += THREADS) m = fmaxf(m, x[i]);
    m = wave_max(m);
    if (lane == 0) sh[wave] = m;
    __syncthreads();
    m = sh[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) m = fmaxf(m, sh[w]);
    __syncthreads();
    float ssum = 0.f;
    for (int i = tid; i < V; i += THREADS) ssum += expf(x[i] - m);
    ssum = wave_sum(ssum);
    if (lane == 0) sh[wave] = ssum;
    __syncthreads();
    ssum = sh[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) ssum += sh[w];
    __syncthreads();
    m_out = m; ssum_out = ssum;
}
template <int LIST, int THREADS>   // (8, 1024), (16, 1024), (32, 512): 1024 threads x 32 entries spill
__global__ __launch_bounds__(THREADS) void beam_row_topk_kernel(const float* __restrict__ logits, int ld, int V, int K,
                                                                         float* __restrict__ row_max, float* __restrict__ row_logsum,
                                                                         float* __restrict__ top_val, int* __restrict__ top_tok) {
    constexpr int NW = THREADS / 64;
    __shared__ float sh[NW];
    __shared__ float wv[NW];
    __shared__ int wi[NW];
    __shared__ int winner;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + (size_t)row * ld;
    // ONE pass over the row: the thread's running maximum with the sum of exp(x - maximum) rescaled whenever the maximum moves, and its
    // local top-LIST, sorted (value desc, index asc).  (Three passes - maximum, sum, candidates - took 50 us per step at the scripts'
    // 116 beam rows, this form 44: what is left is the insertion chain, which a wave runs whenever one of its lanes inserts, and the
    // exponentials, on 116 of the 256 CUs - profiles/r06_kernel_trace_summary_beam4_fp16.md.)
    float tm = -INFINITY, ts = 0.f;
    float lv[LIST];
    int li[LIST];
#pragma unroll
    for (int k = 0; k < LIST; ++k) { lv[k] = -INFINITY; li[k] = 0x7fffffff; }
    // (8 loads in flight per thread)
    for (int i0 = tid; i0 < V; i0 += 8 * THREADS) {
        float vb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) vb[u] = x[min(i0 + u * THREADS, V - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * THREADS;
            if (i >= V) break;
            const float v = vb[u];
            if (v > tm) { ts = ts * expf(tm - v) + 1.0f; tm = v; }   // (first element: 0 * exp(-inf) + 1)
            else if (v > -INFINITY) ts += expf(v - tm);   // -inf is zero mass; while tm is still -inf, exp(-inf - -inf) would be NaN
            if (v > lv[LIST - 1]) {  // strided indices ascend, so an equal value never displaces an earlier one
                lv[LIST - 1] = v; li[LIST - 1] = i;
#pragma unroll
                for (int k = LIST - 1; k > 0; --k) {
                    if (lv[k] > lv[k - 1]) {
                        const float tv = lv[k]; lv[k] = lv[k - 1]; lv[k - 1] = tv;
                        const int ti = li[k]; li[k] = li[k - 1]; li[k - 1] = ti;
                    }
                }
            }
        }
    }
    // row maximum, then every thread's sum brought to it; fixed order (butterflies per wave, the wave sums in wave order)
    float m = wave_max(tm);
    if (lane == 0) sh[wave] = m;
    __syncthreads();
    m = sh[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, sh[w]);
    __syncthreads();
    float ssum = wave_sum(tm == -INFINITY ? 0.f : ts * expf(tm - m));
    if (lane == 0) sh[wave] = ssum;
    __syncthreads();
    ssum = sh[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) ssum += sh[w];
    // K rounds: block-wide arg-max over the threads' current heads; the winner pops its head
    for (int round = 0; round < K; ++round) {
        float bv = lv[0];
        int bi = li[0];
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NW; ++w)
                if (wv[w] > bv || (wv[w] == bv && wi[w] < bi)) { bv = wv[w]; bi = wi[w]; }
            top_val[(size_t)row * BEAM_K + round] = bv;
            top_tok[(size_t)row * BEAM_K + round] = bi;
            winner = bi;
        }
        __syncthreads();
        if (li[0] == winner) {
#pragma unroll
            for (int k = 0; k < LIST - 1; ++k) { lv[k] = lv[k + 1]; li[k] = li[k + 1]; }
            lv[LIST - 1] = -INFINITY; li[LIST - 1] = 0x7fffffff;
        }
    }
    if (tid == 0) { row_max[row] = m; row_logsum[row] = logf(ssum); }
}

// Per batch item: log_softmax + beam score for the nb*K row candidates, then the top K = 2*nb
// of the item (score desc; ties: lower flat index beam*V + token first) - language_model.py:545-561.
constexpr int BEAM_MERGE_THREADS = BEAM_K * BEAM_K / 2;  // one thread per candidate: nb * 2 nb <= 512
__global__ __launch_bounds__(BEAM_MERGE_THREADS) void beam_merge_kernel(const float* __restrict__ row_max, const float* __restrict__ row_logsum,
                                                         const float* __restrict__ top_val, const int* __restrict__ top_tok,
                                                         const float* __restrict__ beam_scores, int nb, int K, int V,
                                                         float* __restrict__ out_score, int* __restrict__ out_tok,
                                                         int* __restrict__ out_beam) {
    // n = nb * 2 nb candidates (<= 512 for nb <= 16): one thread each, ranked against all others through LDS
    __shared__ float ssc[BEAM_MERGE_THREADS];
    __shared__ long long sflat[BEAM_MERGE_THREADS];
    const int item = blockIdx.x, tid = threadIdx.x;
    const int n = nb * K;
    float sc = -INFINITY;
    long long flat = 0x7fffffffffffLL;
    int tok = 0, b = 0;
    if (tid < n) {
        b = tid / K;
        const int row = item * nb + b;
        const float v = top_val[(size_t)row * BEAM_K + (tid - b * K)];
        tok = top_tok[(size_t)row * BEAM_K + (tid - b * K)];
        sc = ((v - row_max[row]) - row_logsum[row]) + beam_scores[row];
        flat = (long long)b * V + tok;
    }
    ssc[tid] = sc;
    sflat[tid] = flat;
    __syncthreads();
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const float oj = ssc[j];
        const long long fj = sflat[j];
        if (oj > sc || (oj == sc && fj < flat)) ++rank;
    }
    if (tid < n && rank < K) {
        out_score[item * K + rank] = sc;
        out_tok[item * K + rank] = tok;
        out_beam[item * K + rank] = b;
    }
}

// Diverse (grouped) beam search, transformers 4.19.2 group_beam_search with its HammingDiversityLogitsProcessor: one workgroup per
// item runs the G groups of num_beams / G rows IN ORDER - group g's candidates are penalised by the tokens groups 0 .. g-1 took in
// this very step - behind the same beam_row_topk_kernel (K = 2 nb candidates per row).  Per group: one thread per candidate of the
// gs * K row candidates, score by the contract of include/rgrg_hip.h ("Diverse beam search": every operation rounded once, the
// multiply NOT contracted into the subtract), ranked against all others through LDS (score desc; ties: lower flat index
// beam_in_group * V + token), top 2 gs -> columns g * 2 gs .. of the item's K = G * 2 gs candidate slots (`beam` = the row within
// the item), and the first gs non-EOS tokens in rank order - what BeamSearchScorer.process hands back as the group's next tokens -
// join the LDS list the later groups count their penalty from.  The row lists are enough: at most nb - gs tokens are penalised and
// a penalty only lowers a value, so a row's list keeps >= nb + gs >= 2 gs unpenalised entries, each of which beats every unlisted
// token of the row.  A finished item needs no special case: the host ignores its candidates.  *penalty is read from device memory,
// so one captured step serves every penalty.
__global__ __launch_bounds__(BEAM_MERGE_THREADS) void beam_group_merge_kernel(const float* __restrict__ row_max, const float* __restrict__ row_logsum,
                                                               const float* __restrict__ top_val, const int* __restrict__ top_tok,
                                                               const float* __restrict__ beam_scores, int nb, int G,
                                                               const float* __restrict__ penalty, int V, float* __restrict__ out_score,
                                                               int* __restrict__ out_tok, int* __restrict__ out_beam) {
#pragma clang fp contract(off)
    __shared__ float ssc[BEAM_MERGE_THREADS];
    __shared__ long long sflat[BEAM_MERGE_THREADS];
    __shared__ int chosen[BEAM_K / 2];   // tokens taken by the groups so far: <= nb - gs when the last group reads it
    __shared__ int rtok[BEAM_K];         // the current group's ranked tokens
    __shared__ int nchosen;
    const int item = blockIdx.x, tid = threadIdx.x;
    const int gs = nb / G, K = 2 * nb, n = gs * K, top = 2 * gs;   // n <= 512 for nb <= 16
    const float lam = *penalty;
    if (tid == 0) nchosen = 0;
    for (int g = 0; g < G; ++g) {
        __syncthreads();   // the list of the groups before this one is complete; ssc / sflat / rtok are free again
        float sc = -INFINITY;
        long long flat = 0x7fffffffffffLL;
        int tok = 0, b = 0;
        if (tid < n) {
            const int bi = tid / K;
            b = g * gs + bi;
            const int row = item * nb + b;
            const float v = top_val[(size_t)row * BEAM_K + (tid - bi * K)];
            tok = top_tok[(size_t)row * BEAM_K + (tid - bi * K)];
            int freq = 0;
            for (int j = 0; j < nchosen; ++j) freq += (chosen[j] == tok) ? 1 : 0;
            const float logp = __fsub_rn(__fsub_rn(v, row_max[row]), row_logsum[row]);
            float pen = __fmul_rn(lam, (float)freq);
            asm volatile("" : "+v"(pen));   // the product stays a rounded value of its own: __fmul_rn is a plain multiply in this
                                            // toolchain and hipcc contracts it into the subtract once inlined, the pragma notwithstanding
            sc = __fadd_rn(__fsub_rn(logp, pen), beam_scores[row]);
            flat = (long long)bi * V + tok;
        }
        ssc[tid] = sc;
        sflat[tid] = flat;
        __syncthreads();
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float oj = ssc[j];
            const long long fj = sflat[j];
            if (oj > sc || (oj == sc && fj < flat)) ++rank;
        }
        if (tid < n && rank < top) {
            out_score[item * K + g * top + rank] = sc;
            out_tok[item * K + g * top + rank] = tok;
            out_beam[item * K + g * top + rank] = b;
            rtok[rank] = tok;   // n = gs * 2 nb >= 2 gs candidates with distinct (score, flat): every rank below top is written
        }
        __syncthreads();
        if (tid == 0) {
            int c = nchosen;
            for (int r = 0, picked = 0; r < top && picked < gs; ++r)
                if (rtok[r] != EOS_ID) { chosen[c++] = rtok[r]; ++picked; }
            nchosen = c;
        }
    }
}

// ---- more than 16 beams (round 6: the reference's loop has no bound, language_model.py:450-475).  The per-thread sorted lists of the
// kernels above hold 32 candidates in registers; wider beams take K = 2 num_beams rounds of a block-wide arg-max over the elements
// that come AFTER the previous winner in the same total order (value desc, index asc) - K scans of the row from L2 instead of one,
// the same winners.  top_val / top_tok rows are K wide here (ldk).
template <int NW>
__device__ __forceinline__ void beam_block_argmax(float& bv, long long& bi, float* wv, long long* wi, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const long long oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
    __syncthreads();
    bv = wv[0]; bi = wi[0];
    for (int w = 1; w < NW; ++w)
        if (wv[w] > bv || (wv[w] == bv && wi[w] < bi)) { bv = wv[w]; bi = wi[w]; }
    __syncthreads();
}
__global__ __launch_bounds__(BEAM_ROW_THREADS) void beam_row_topk_wide_kernel(const float* __restrict__ logits, int ld, int V, int K,
                                                                              float* __restrict__ row_max, float* __restrict__ row_logsum,
                                                                              float* __restrict__ top_val, int* __restrict__ top_tok) {
    constexpr int NW = BEAM_ROW_THREADS / 64;
    __shared__ float sh[NW];
    __shared__ float wv[NW];
    __shared__ long long wi[NW];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (size_t)row * ld;
    float m, ssum;
    beam_row_max_sumexp<BEAM_ROW_THREADS>(x, V, sh, m, ssum);
    float pv = INFINITY;
    long long pi = -1;
    for (int round = 0; round < K; ++round) {
        float bv = -INFINITY;
        long long bi = 0x7fffffffLL;
        for (int i = tid; i < V; i += BEAM_ROW_THREADS) {
            const float v = x[i];
            if ((v < pv || (v == pv && i > pi)) && v > bv) { bv = v; bi = i; }   // strided indices ascend: the first of equal values stays
        }
        beam_block_argmax<NW>(bv, bi, wv, wi, tid);
        if (tid == 0) {
            top_val[(size_t)row * K + round] = bv;
            top_tok[(size_t)row * K + round] = (int)bi;
        }
        pv = bv; pi = bi;
    }
    if (tid == 0) { row_max[row] = m; row_logsum[row] = logf(ssum); }
}
// Per batch item: the nb * K candidate scores (same expression as beam_merge_kernel) into `score` [item][nb * K], then the item's
// top K in the order (score desc, flat index beam * V + token asc), again by K rounds over what follows the previous winner.
__global__ __launch_bounds__(256) void beam_merge_wide_kernel(const float* __restrict__ row_max, const float* __restrict__ row_logsum,
                                                              const float* __restrict__ top_val, const int* __restrict__ top_tok,
                                                              const float* __restrict__ beam_scores, int nb, int K, int V,
                                                              float* __restrict__ score, float* __restrict__ out_score,
                                                              int* __restrict__ out_tok, int* __restrict__ out_beam) {
    __shared__ float wv[4];
    __shared__ long long wi[4];
    const int item = blockIdx.x, tid = threadIdx.x;
    const int n = nb * K;
    float* sc = score + (size_t)item * n;
    for (int c = tid; c < n; c += 256) {
        const int b = c / K, row = item * nb + b;
        sc[c] = ((top_val[(size_t)row * K + (c - b * K)] - row_max[row]) - row_logsum[row]) + beam_scores[row];
    }
    __syncthreads();
    float pv = INFINITY;
    long long pf = -1;
    for (int round = 0; round < K; ++round) {
        float bv = -INFINITY;
        long long bf = 0x7fffffffffffLL;
        for (int c = tid; c < n; c += 256) {
            const int b = c / K;
            const float v = sc[c];
            const long long flat = (long long)b * V + top_tok[(size_t)(item * nb + b) * K + (c - b * K)];
            if ((v < pv || (v == pv && flat > pf)) && (v > bv || (v == bv && flat < bf))) { bv = v; bf = flat; }
        }
        beam_block_argmax<4>(bv, bf, wv, wi, tid);
        if (tid == 0) {
            out_score[item * K + round] = bv;
            out_tok[item * K + round] = (int)(bf % V);
            out_beam[item * K + round] = (int)(bf / V);
        }
        pv = bv; pf = bf;
    }
}

// New ancestor table after the host picked the surviving beams: row r continues beam parent[r];
// slots 0..t come from the parent's table, slot t+1 (written this step) lives in the parent's row.
__global__ __launch_bounds__(256) void beam_advance_kernel(const int* __restrict__ src_old, int* __restrict__ src_new,
                                                           const int* __restrict__ parent, int* __restrict__ step, int T,
                                                           int R) {
    const int r = blockIdx.x, t = *step;
    const int p = parent[r];
    for (int j = threadIdx.x; j <= t; j += 256) src_new[(size_t)r * T + j] = src_old[(size_t)p * T + j];
    if (threadIdx.x == 0) src_new[(size_t)r * T + t + 1] = p;
    __syncthreads();
    (void)R;
}
__global__ void beam_step_inc_kernel(int* __restrict__ step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *step += 1;
}
__global__ __launch_bounds__(256) void beam_init_kernel(int* __restrict__ src, int T, int nb, int R, int* __restrict__ step) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < R) src[(size_t)r * T] = (r / nb) * nb;  // slot 0 (image key/value) is stored once per item, in its first beam row
    if (r == 0) *step = 0;
}
// the two launches on raw pointers, shared by beam_search_run and the test hooks (rgrg_debug_beam_init / _advance)
int launch_beam_init(int* src, int T, int nb, int R, int* step, hipStream_t st) {
    hipLaunchKernelGGL(beam_init_kernel, dim3((R + 255) / 256), dim3(256), 0, st, src, T, nb, R, step);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
int launch_beam_advance(const int* src_old, int* src_new, const int* parent, int* step, int T, int R, hipStream_t st) {
    hipLaunchKernelGGL(beam_advance_kernel, dim3(R), dim3(256), 0, st, src_old, src_new, parent, step, T, R);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// The two launches of a plain ranking, shared by beam_search_run and the test hooks (rgrg_debug_beam_row_topk / _merge), and the
// one place that chooses the kernel.  More than 16 beams (K > BEAM_K): the K-round kernels on candidate rows K wide; up to 16: the
// register lists, LIST >= K, on rows BEAM_K wide.  force_wide (the hooks only): the K-round kernels at any K.
bool beam_wide(int K, bool force_wide) { return force_wide || K > BEAM_K; }
// Row ranking of `rows` logits rows, K = 2 num_beams candidates each.
void launch_beam_row_topk(const float* logits, int ld, int V, int rows, int K, float* row_max, float* row_logsum, float* top_val,
                                 int* top_tok, bool force_wide, hipStream_t st) {
    if (beam_wide(K, force_wide)) {
        hipLaunchKernelGGL(beam_row_topk_wide_kernel, dim3(rows), dim3(BEAM_ROW_THREADS), 0, st, logits, ld, V, K, row_max, row_logsum,
                           top_val, top_tok);
        return;
    }
#define BEAM_TOPK(LIST_, THREADS_) hipLaunchKernelGGL((beam_row_topk_kernel<LIST_, THREADS_>), dim3(rows), dim3(THREADS_), 0, st, logits, ld, V, K, \
                                              row_max, row_logsum, top_val, top_tok)
    if (K <= 8) BEAM_TOPK(8, 1024); else if (K <= 16) BEAM_TOPK(16, 1024); else BEAM_TOPK(32, 512);
#undef BEAM_TOPK
}
// Item merge of S items with nb rows of K = 2 nb candidates (rows as launch_beam_row_topk left them); `score` [S][nb * K] is the
// wide form's scratch.
void launch_beam_merge(const float* row_max, const float* row_logsum, const float* top_val, const int* top_tok,
                              const float* beam_scores, int S, int nb, int V, float* score, float* out_score, int* out_tok, int* out_beam,
                              bool force_wide, hipStream_t st) {
    const int K = 2 * nb;
    if (beam_wide(K, force_wide))
        hipLaunchKernelGGL(beam_merge_wide_kernel, dim3(S), dim3(256), 0, st, row_max, row_logsum, top_val, top_tok, beam_scores, nb, K, V,
                           score, out_score, out_tok, out_beam);
    else
        hipLaunchKernelGGL(beam_merge_kernel, dim3(S), dim3(BEAM_MERGE_THREADS), 0, st, row_max, row_logsum, top_val, top_tok, beam_scores,
                           nb, K, V, out_score, out_tok, out_beam);
}

}  // namespace rgrg

using namespace rgrg;

// ------------------------------------------------------------------ beam search (host side)
// BeamHypotheses / BeamSearchScorer of transformers 4.19.2 (used by language_model.py:457-464, :570-578,
// :597-605), restated on the host: hypothesis scores, worst_score and the is_done test are double arithmetic
// (HF does them on Python floats obtained through .item()), beam scores stay float32.
namespace rgrg {
void BeamHyps::add(const std::vector<long long>& toks, double sum_logprobs, int nb, double lp) {
    const double score = sum_logprobs / std::pow((double)toks.size(), lp);
    if ((int)beams.size() < nb || score > worst) {
        beams.push_back({score, toks});
        if ((int)beams.size() > nb) {
            int i0 = 0;  // sorted([(score, idx)]): smallest (score, idx) is dropped, worst = the next one
            for (int i = 1; i < (int)beams.size(); ++i)
                if (beams[i].score < beams[i0].score) i0 = i;
            beams.erase(beams.begin() + i0);
            double w = beams[0].score;
            for (auto& h : beams) w = h.score < w ? h.score : w;
            worst = w;
        } else {
            worst = score < worst ? score : worst;
        }
    }
}
bool BeamHyps::is_done(double best_sum_logprobs, int cur_len, bool early, int nb, double lp) const {
    if ((int)beams.size() < nb) return false;
    if (early) return true;
    return worst >= best_sum_logprobs / std::pow((double)cur_len, lp);
}

// BeamSearchScorer.process for ONE group of gs rows of one item (plain beam search: the item's one group of nb rows), shared by the
// lock-step loop below and the rolling loop (decoder_beam_roll.hip).  sc / tok / beam: the group's 2 gs ranked candidates (beam = the
// row within the item); item_row0: the item's first row in `ids`; nscore / ntok / nidx: the next score, token and parent row of the
// group's gs rows.  The heap (capacity nb) and `done` belong to the ITEM: a finished item takes PAD.
int beam_process_group(BeamHyps& hyps, char& done, const float* sc, const int* tok, const int* beam, int gs, int nb, int item_row0,
                       const std::vector<std::vector<long long>>& ids, int cur_len, bool early, double lp, float* nscore, int* ntok,
                       int* nidx) {
    if (done) {
        for (int j = 0; j < gs; ++j) { nscore[j] = 0.f; ntok[j] = PAD_ID; nidx[j] = 0; }
        return RGRG_OK;
    }
    int beam_idx = 0;
    for (int rank = 0; rank < 2 * gs; ++rank) {
        const int row = item_row0 + beam[rank];
        if (tok[rank] == EOS_ID) {
            if (rank >= gs) continue;
            hyps.add(ids[row], (double)sc[rank], nb, lp);
        } else {
            nscore[beam_idx] = sc[rank]; ntok[beam_idx] = tok[rank]; nidx[beam_idx] = row;
            ++beam_idx;
        }
        if (beam_idx == gs) break;
    }
    if (beam_idx < gs) { set_error("beam search: fewer than num_beams non-EOS candidates"); return RGRG_ESTATE; }
    done = done || hyps.is_done((double)sc[0], cur_len, early, nb, lp);
    return RGRG_OK;
}

// BeamSearchScorer.finalize for one item: an item that is not done adds its nb open beams (rows: ids / scores of its first row on)
void beam_finalize_item(BeamHyps& hyps, bool done, const std::vector<long long>* rows, const float* scores, int nb, double lp) {
    if (done) return;
    for (int j = 0; j < nb; ++j) hyps.add(rows[j], (double)scores[j], nb, lp);
}

// ... and its output: the `keep` best hypotheses per item, padded to the width L over ALL items -> out_ids [S * keep][out_ld], *out_len = L
int beam_write_best(const std::vector<BeamHyps>& hyps, int keep, int max_length, int64_t* out_ids, int out_ld, int* out_len, hipStream_t st) {
    // num_beam_hyps_to_keep best hypotheses per item: sorted(beams, key=score) is stable and pop() takes the last, i.e.
    // descending score and, among equal scores, the LATER-added hypothesis first
    const int S = (int)hyps.size(), NR = S * keep;
    std::vector<const std::vector<long long>*> best(NR);
    int max_sent = 0;
    for (int b = 0; b < S; ++b) {
        const int nh = (int)hyps[b].beams.size();
        if (nh < keep) { set_error("beam search: item %d has %d finished hypotheses, %d requested", b, nh, keep); return RGRG_ESTATE; }
        std::vector<int> order(nh);
        for (int j = 0; j < nh; ++j) order[j] = j;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return hyps[b].beams[x].score < hyps[b].beams[y].score; });
        for (int j = 0; j < keep; ++j) {
            best[b * keep + j] = &hyps[b].beams[order[nh - 1 - j]].toks;
            const int len = (int)best[b * keep + j]->size();
            max_sent = len > max_sent ? len : max_sent;
        }
    }
    const int L = (max_sent + 1 < max_length) ? max_sent + 1 : max_length;
    std::vector<long long> dec((size_t)NR * L, PAD_ID);
    for (int b = 0; b < NR; ++b) {
        const int len = (int)best[b]->size();
        for (int j = 0; j < len && j < L; ++j) dec[(size_t)b * L + j] = (*best[b])[j];
        if (len < max_length) dec[(size_t)b * L + len] = EOS_ID;
    }
    RGRG_HIP(hipMemcpy2DAsync(out_ids, (size_t)out_ld * sizeof(int64_t), dec.data(), (size_t)L * sizeof(long long),
                              (size_t)L * sizeof(long long), NR, hipMemcpyHostToDevice, st));
    RGRG_HIP(hipStreamSynchronize(st));
    *out_len = L;
    return RGRG_OK;
}

// more than 16 beams: the K-wide candidate rows of the wide ranking kernels for R rows, grown on demand
int beam_reserve_wide(rgrg_decoder* d, int R, int K) {
    if (d->wide_cap >= (size_t)R * K) return RGRG_OK;
    RGRG_HIP(hipStreamSynchronize(d->stream));
    for (auto& g : d->graphs) (void)hipGraphExecDestroy(g.exec);   // (captured beam steps bake the buffers in)
    d->graphs.clear();
    for (void** q : {(void**)&d->wide_val, (void**)&d->wide_tok, (void**)&d->wide_score}) {   // grown: the smaller buffers go
        if (!*q) continue;
        auto it = std::find(d->allocs.begin(), d->allocs.end(), *q);
        if (it != d->allocs.end()) d->allocs.erase(it);
        (void)hipFree(*q);
        *q = nullptr;
    }
    d->wide_cap = 0;
    int r;
    if ((r = dmalloc(d, (void**)&d->wide_val, (size_t)R * K * 4, true)) || (r = dmalloc(d, (void**)&d->wide_tok, (size_t)R * K * 4, true)) ||
        (r = dmalloc(d, (void**)&d->wide_score, (size_t)R * K * 4, true)))
        return r;
    d->wide_cap = (size_t)R * K;
    return RGRG_OK;
}
}  // namespace rgrg

// prompt == NULL: the BOS start of rgrg_decoder_beam_search.  With a prompt (rgrg_decoder_beam_search_prompted, decoder_prompt.hip)
// the first iteration ranks the logits of the prompt's last position instead of running a step - the reference's first iteration
// on nb identical rows - and ids / cur_len start at the prompt.
// sample != NULL (never with groups): beam-search sampling (rgrg_decoder_beam_sample[_prompted]; the caller has checked the
// parameters and nb <= 16) - the ranking is the Gumbel top-2nb draw of beam_sample.hip under its own StepEnd, everything behind it
// (process / finalize below) is plain beam search's.
// groups != NULL: diverse beam search (rgrg_decoder_group_beam_search[_prompted]; the caller has checked G and the penalty) - G
// groups of gs = nb / G rows per item, ranked by beam_group_merge_kernel; BeamSearchScorer.process runs per item and group with
// group_size gs on the item's shared heap and `done` flag.  groups == NULL is G = 1 on beam_merge_kernel: plain beam search.
int rgrg::beam_search_run(rgrg_decoder* d, const float* feats, int S, int num_beams, int max_length, int early_stopping,
                          float length_penalty, int num_return_sequences, int64_t* out_ids, int out_ld, int* out_len, void* stream,
                          const BeamPrompt* prompt, const BeamGroups* groups, const BeamSample* sample) {
    RGRG_CHECK_ARG(d && feats && out_ids && out_len && S > 0 && num_beams > 1 && num_beams <= (1 << 14));
    RGRG_CHECK_ARG(!(groups && sample) && (!sample || num_beams <= BEAM_K / 2));
    RGRG_CHECK_ARG(num_return_sequences >= 1 && num_return_sequences <= num_beams);
    const int nb = num_beams, K = 2 * nb, R = S * nb;
    const int G = groups ? groups->G : 1, gs = nb / G;   // K = G * 2 gs candidate slots per item either way
    RGRG_CHECK_ARG(R <= d->max_seqs && max_length >= 2 && max_length <= d->max_len && out_ld >= max_length);
    hipStream_t st = d->stream;
    const bool wide = beam_wide(K);   // more than 16 beams: the K-round ranking kernels on K-wide candidate rows
    if (wide) {
        int r = beam_reserve_wide(d, R, K);
        if (r) return r;
    }
    if (groups && !d->group_penalty) {
        int r = dmalloc(d, (void**)&d->group_penalty, sizeof(float), true);
        if (r) return r;
    }
    if (sample) {
        int r;
        if (!d->sample_prm && (r = dmalloc(d, &d->sample_prm, sample_params_bytes(), true))) return r;
        if (!d->bsample_s && (r = dmalloc(d, (void**)&d->bsample_s, (size_t)d->rows * BEAM_K * sizeof(float), true))) return r;
    }
    ++d->epoch;   // the cache rows are rewritten: an open rolling session is stale
    RGRG_HIP(hipEventRecord(d->ev_in, as_stream(stream)));
    RGRG_HIP(hipStreamWaitEvent(st, d->ev_in, 0));
    // ... and the sampling step its seed and parameters from this block: the graph of a spec serves every seed and parameter set
    if (sample) {
        int r = enqueue_sample_params(d->sample_prm, sample->temperature, sample->top_k, sample->top_p, sample->seed, st);
        if (r) return r;
    }
    // the captured group step reads the penalty from this word: the graph of a spec serves every penalty
    if (groups) RGRG_HIP(hipMemcpyAsync(d->group_penalty, &groups->penalty, sizeof(float), hipMemcpyHostToDevice, st));
    // prefill for the S image features; the image key/value of item s is stored in cache row s*nb (slot 0)
    int rc = enqueue_prefill(d, feats, S, nb);
    if (rc) return rc;
    bool padded = false;
    std::vector<long long> prompt_ids;
    if (prompt) {
        if ((rc = enqueue_beam_prompt(d, *prompt, S, nb, &padded, &prompt_ids))) return rc;
    } else {
        if ((rc = launch_beam_init(d->src_a, d->T, nb, R, d->step, st))) return rc;
    }

    std::vector<std::vector<long long>> ids(R, std::vector<long long>(1, BOS_ID));
    if (prompt)
        for (int r = 0; r < R; ++r) ids[r].assign(prompt_ids.begin() + (size_t)(r / nb) * prompt->T, prompt_ids.begin() + (size_t)(r / nb + 1) * prompt->T);
    std::vector<float> beam_scores(R, 0.f), h_score((size_t)S * K);
    std::vector<int> beam_tok(R, BOS_ID), parent(R, 0), h_tok((size_t)S * K), h_beam((size_t)S * K);
    for (int r = 0; r < R; ++r) beam_scores[r] = (r % nb % gs == 0) ? 0.f : -1e9f;   // beam_scores[:, ::gs] = 0
    std::vector<BeamHyps> hyps(S);
    std::vector<char> done(S, 0);
    const double lp = (double)length_penalty;
    int* src_cur = d->src_a;
    int* src_nxt = d->src_b;
    int cur_len = prompt ? prompt->T : 1;
    bool first_ranking = prompt != nullptr;
    // the ranking of d->logits behind a step (captured with it) or behind the prompt's last position
    auto enqueue_ranking = [&]() -> int {
        if (sample)   // t = *d->step: the step word, T - 1 for the first ranking behind a prompt of T tokens
            return launch_beam_sample_rank(d->logits, (size_t)d->ld_logits, d->V, S, nb, d->beam_scores, d->sample_prm, nullptr, d->step, 0, 0,
                                           d->top_val, d->bsample_s, d->top_tok, d->cand_score, d->cand_tok, d->cand_beam, st);
        launch_beam_row_topk(d->logits, d->ld_logits, d->V, R, K, d->row_max, d->row_logsum, wide ? d->wide_val : d->top_val,
                             wide ? d->wide_tok : d->top_tok, false, st);
        if (groups)
            hipLaunchKernelGGL(beam_group_merge_kernel, dim3(S), dim3(BEAM_MERGE_THREADS), 0, st, d->row_max, d->row_logsum, d->top_val,
                               d->top_tok, d->beam_scores, nb, G, d->group_penalty, d->V, d->cand_score, d->cand_tok, d->cand_beam);
        else
            launch_beam_merge(d->row_max, d->row_logsum, wide ? d->wide_val : d->top_val, wide ? d->wide_tok : d->top_tok, d->beam_scores,
                              S, nb, d->V, d->wide_score, d->cand_score, d->cand_tok, d->cand_beam, false, st);
        return RGRG_OK;
    };
    std::vector<float> nscore(R);
    std::vector<int> ntok(R), nidx(R);
    d->logits_stale_rows = 0;   // beam steps write d->logits
    d->logits_valid = false;
    while (true) {
        RGRG_HIP(hipMemcpyAsync(d->beam_tok, beam_tok.data(), R * sizeof(int), hipMemcpyHostToDevice, st));
        RGRG_HIP(hipMemcpyAsync(d->beam_scores, beam_scores.data(), R * sizeof(float), hipMemcpyHostToDevice, st));
        if (first_ranking) {   // the prompt pass left the ln_f row of every item's last position in its nb rows: head, ranking, no step
            if ((rc = enqueue_head_logits(d, R))) return rc;
            if ((rc = enqueue_ranking())) return rc;
            RGRG_LAUNCH_CHECK();
        } else {
            // the step (embed .. lm_head .. ranking) is captured once per spec - the ancestor table it reads is part of it - and
            // replayed; behind a left-padded prompt it carries per-row positions and the padded slots of every row
            StepSpec step;
            step.rows = R; step.tok = d->beam_tok; step.src = src_cur; step.end = sample ? STEP_BEAM_SAMPLE : STEP_BEAM; step.nb = nb; step.G = groups ? G : 0;
            if (padded) step = padded_step_spec(d, step, d->beam_pad);
            hipGraphExec_t exec = nullptr;
            rc = step_graph(d, step, [&]() -> int {
                int r = padded ? enqueue_beam_row_pos(d, R) : RGRG_OK;
                if (!r && !(r = enqueue_step(d, step, false))) r = enqueue_ranking();
                return r;
            }, &exec);
            if (rc) return rc;
            RGRG_HIP(hipGraphLaunch(exec, st));
        }
        RGRG_HIP(hipMemcpyAsync(h_score.data(), d->cand_score, (size_t)S * K * sizeof(float), hipMemcpyDeviceToHost, st));
        RGRG_HIP(hipMemcpyAsync(h_tok.data(), d->cand_tok, (size_t)S * K * sizeof(int), hipMemcpyDeviceToHost, st));
        RGRG_HIP(hipMemcpyAsync(h_beam.data(), d->cand_beam, (size_t)S * K * sizeof(int), hipMemcpyDeviceToHost, st));
        RGRG_HIP(hipStreamSynchronize(st));
        // BeamSearchScorer.process, per item and - in group order - per group of gs rows (plain beam search: one group of nb): the
        // heap (capacity nb) and `done` belong to the ITEM, so `done` may flip between two groups of a step, and the later groups
        // of that item then take PAD like a finished item (HF's behaviour, kept); items are independent, so item-major order is HF's
        for (int b = 0; b < S; ++b) {
            for (int g = 0; g < G; ++g) {
                const int r0 = b * nb + g * gs;            // the group's first row
                const size_t c0 = (size_t)b * K + (size_t)g * 2 * gs;   // ... and first candidate slot
                if ((rc = beam_process_group(hyps[b], done[b], h_score.data() + c0, h_tok.data() + c0, h_beam.data() + c0, gs, nb, b * nb, ids,
                                             cur_len, early_stopping != 0, lp, nscore.data() + r0, ntok.data() + r0, nidx.data() + r0)))
                    return rc;
            }
        }
        // input_ids = cat(input_ids[beam_idx], tokens); cache "re-order" = new ancestor table
        std::vector<std::vector<long long>> nids(R);
        for (int r = 0; r < R; ++r) { nids[r] = ids[nidx[r]]; nids[r].push_back(ntok[r]); }
        ids.swap(nids);
        beam_scores = nscore;
        for (int r = 0; r < R; ++r) { beam_tok[r] = ntok[r]; parent[r] = nidx[r]; }
        ++cur_len;
        bool all_done = true;
        for (int b = 0; b < S; ++b) all_done = all_done && done[b];
        if (all_done || cur_len >= max_length) break;
        if (first_ranking) {
            // no slot was written: slots 0 .. T of every beam live in row s * nb whatever its parent, and the prompt pass
            // pointed BOTH tables there - the advance kernel would point slot T at the parent's row
            first_ranking = false;
        } else {
            RGRG_HIP(hipMemcpyAsync(d->beam_parent, parent.data(), R * sizeof(int), hipMemcpyHostToDevice, st));
            if ((rc = launch_beam_advance(src_cur, src_nxt, d->beam_parent, d->step, d->T, R, st))) return rc;
        }
        hipLaunchKernelGGL(beam_step_inc_kernel, dim3(1), dim3(64), 0, st, d->step);
        RGRG_LAUNCH_CHECK();
        int* tmp = src_cur; src_cur = src_nxt; src_nxt = tmp;
    }
    // BeamSearchScorer.finalize (num_beam_hyps_to_keep = 1)
    for (int b = 0; b < S; ++b) beam_finalize_item(hyps[b], done[b] != 0, &ids[(size_t)b * nb], &beam_scores[(size_t)b * nb], nb, lp);
    if ((rc = beam_write_best(hyps, num_return_sequences, max_length, out_ids, out_ld, out_len, st))) return rc;
    d->logits_valid = true;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_beam_search(rgrg_decoder* d, const float* feats, int S, int num_beams, int max_length,
                                        int early_stopping, float length_penalty, int num_return_sequences, int64_t* out_ids,
                                        int out_ld, int* out_len, void* stream) {
    return beam_search_run(d, feats, S, num_beams, max_length, early_stopping, length_penalty, num_return_sequences, out_ids, out_ld,
                           out_len, stream, nullptr);
}

// the refusals the two beam-sampling entries share, each with a message
int rgrg::check_beam_sample(const char* who, int num_beams, int num_return_sequences, float temperature, int top_k, float top_p) {
    const int nb = num_beams;
    if (nb < 2) { set_error("%s: num_beams %d: beam sampling needs more than one beam", who, nb); return RGRG_EINVAL; }
    if (nb > BEAM_K / 2) {
        set_error("%s: num_beams %d: beam sampling ranks at most %d beams (the row candidate lists hold %d entries)", who, nb, BEAM_K / 2, BEAM_K);
        return RGRG_EINVAL;
    }
    if (num_return_sequences < 1 || num_return_sequences > nb) {
        set_error("%s: num_return_sequences %d outside 1 .. num_beams %d", who, num_return_sequences, nb);
        return RGRG_EINVAL;
    }
    if (!(temperature > 0.f) || !std::isfinite(temperature)) { set_error("%s: temperature has to be a finite float > 0, but is %g", who, (double)temperature); return RGRG_EINVAL; }
    if (top_k < 0) { set_error("%s: top_k has to be >= 0 (0 = off), but is %d", who, top_k); return RGRG_EINVAL; }
    if (!(top_p > 0.f && top_p <= 1.0f)) { set_error("%s: top_p has to be in (0, 1], but is %g", who, (double)top_p); return RGRG_EINVAL; }
    return RGRG_OK;
}

extern "C" int rgrg_decoder_beam_sample(rgrg_decoder* d, const float* feats, int S, int num_beams, int max_length, int early_stopping,
                                        float length_penalty, int num_return_sequences, float temperature, int top_k, float top_p,
                                        uint64_t seed, int64_t* out_ids, int out_ld, int* out_len, void* stream) {
    int rc;
    if ((rc = check_beam_sample("rgrg_decoder_beam_sample", num_beams, num_return_sequences, temperature, top_k, top_p))) return rc;
    const BeamSample smp{temperature, top_k, top_p, seed};
    return beam_search_run(d, feats, S, num_beams, max_length, early_stopping, length_penalty, num_return_sequences, out_ids, out_ld,
                           out_len, stream, nullptr, nullptr, &smp);
}

// the refusals the two diverse entries share, each with a message
int rgrg::check_beam_groups(const char* who, int num_beams, int num_beam_groups, float diversity_penalty, int num_return_sequences) {
    const int nb = num_beams, G = num_beam_groups;
    if (nb < 2 || G < 1) { set_error("%s: num_beams %d (> 1) and num_beam_groups %d (>= 1) are required", who, nb, G); return RGRG_EINVAL; }
    if (nb > BEAM_K / 2) {
        set_error("%s: num_beams %d: diverse beam search ranks at most %d beams (the wide ranking kernels have no group form)", who, nb, BEAM_K / 2);
        return RGRG_EINVAL;
    }
    if (G > nb) { set_error("%s: num_beam_groups %d has to be smaller or equal to num_beams %d", who, G, nb); return RGRG_EINVAL; }
    if (nb % G != 0) { set_error("%s: num_beams %d has to be divisible by num_beam_groups %d", who, nb, G); return RGRG_EINVAL; }
    if (G > 1 && !(diversity_penalty > 0.f && std::isfinite(diversity_penalty))) {
        set_error("%s: diversity_penalty has to be a float > 0 with num_beam_groups %d > 1, but is %g", who, G, (double)diversity_penalty);
        return RGRG_EINVAL;
    }
    if (num_return_sequences < 1 || num_return_sequences > nb) {
        set_error("%s: num_return_sequences %d outside 1 .. num_beams %d", who, num_return_sequences, nb);
        return RGRG_EINVAL;
    }
    return RGRG_OK;
}

extern "C" int rgrg_decoder_group_beam_search(rgrg_decoder* d, const float* feats, int S, int num_beams, int num_beam_groups,
                                              float diversity_penalty, int max_length, int early_stopping, float length_penalty,
                                              int num_return_sequences, int64_t* out_ids, int out_ld, int* out_len, void* stream) {
    int rc;
    if ((rc = check_beam_groups("rgrg_decoder_group_beam_search", num_beams, num_beam_groups, diversity_penalty, num_return_sequences))) return rc;
    const BeamGroups grp{num_beam_groups, num_beam_groups > 1 ? diversity_penalty : 0.f};
    return beam_search_run(d, feats, S, num_beams, max_length, early_stopping, length_penalty, num_return_sequences, out_ids, out_ld,
                           out_len, stream, nullptr, &grp);
}

// Test hook: beam_group_merge_kernel alone on caller buffers (top_val / top_tok rows BEAM_K wide, as in the decoder)
extern "C" int rgrg_debug_beam_group_merge(const float* row_max, const float* row_logsum, const float* top_val, const int* top_tok,
                                           const float* beam_scores, int S, int nb, int G, float penalty, int V, float* out_score,
                                           int* out_tok, int* out_beam, void* stream) {
    RGRG_CHECK_ARG(row_max && row_logsum && top_val && top_tok && beam_scores && out_score && out_tok && out_beam);
    RGRG_CHECK_ARG(S > 0 && V > 0 && nb >= 1 && nb <= BEAM_K / 2 && G >= 1 && G <= nb && nb % G == 0);
    float* pen = nullptr;
    RGRG_HIP(hipMalloc((void**)&pen, sizeof(float)));
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemcpyAsync(pen, &penalty, sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(beam_group_merge_kernel, dim3(S), dim3(BEAM_MERGE_THREADS), 0, st, row_max, row_logsum, top_val, top_tok, beam_scores,
                           nb, G, pen, V, out_score, out_tok, out_beam);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(st);   // the penalty word is the call's own: it must outlive the launch
    (void)hipFree(pen);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { set_error("rgrg_debug_beam_group_merge: %s", hipGetErrorString(e)); return RGRG_EHIP; }
    return RGRG_OK;
}

// Test hooks: the plain ranking's two launches alone on caller buffers, through launch_beam_row_topk / launch_beam_merge - the
// decoder's own choice of kernel.  RGRG_DEBUG_BEAM_WIDE=1 (read per call, by the hooks only) takes the wide form at K <= 32 too.
static bool debug_force_wide() {
    const char* e = getenv("RGRG_DEBUG_BEAM_WIDE");
    return e && e[0] == '1';
}
static int debug_sync(const char* who, hipStream_t st) {
    hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(e)); return RGRG_EHIP; }
    return RGRG_OK;
}
extern "C" int rgrg_debug_beam_row_topk(const float* logits, int ld, int V, int rows, int K, float* row_max, float* row_logsum,
                                        float* top_val, int* top_tok, void* stream) {
    RGRG_CHECK_ARG(logits && row_max && row_logsum && top_val && top_tok);
    RGRG_CHECK_ARG(V >= 1 && ld >= V && rows >= 1 && K >= 2 && K % 2 == 0 && K <= V);
    hipStream_t st = as_stream(stream);
    launch_beam_row_topk(logits, ld, V, rows, K, row_max, row_logsum, top_val, top_tok, debug_force_wide(), st);
    return debug_sync("rgrg_debug_beam_row_topk", st);
}
extern "C" int rgrg_debug_beam_merge(const float* row_max, const float* row_logsum, const float* top_val, const int* top_tok,
                                     const float* beam_scores, int S, int nb, int V, float* score_scratch, float* out_score, int* out_tok,
                                     int* out_beam, void* stream) {
    RGRG_CHECK_ARG(row_max && row_logsum && top_val && top_tok && beam_scores && score_scratch && out_score && out_tok && out_beam);
    RGRG_CHECK_ARG(S >= 1 && S <= 65535 && nb >= 1 && nb <= (1 << 14) && V >= 2 * nb);
    hipStream_t st = as_stream(stream);
    launch_beam_merge(row_max, row_logsum, top_val, top_tok, beam_scores, S, nb, V, score_scratch, out_score, out_tok, out_beam,
                      debug_force_wide(), st);
    return debug_sync("rgrg_debug_beam_merge", st);
}

// Test hooks: the two ancestor-table kernels of the plain loop alone (tests/test_gpu_step_rows.py).  rgrg_debug_beam_advance reads
// *step and parent [R] back first (one synchronisation): 0 <= *step <= T - 2 and 0 <= parent[r] < R, or nothing is launched.
extern "C" int rgrg_debug_beam_init(int* src, int T, int nb, int R, int* step, void* stream) {
    RGRG_CHECK_ARG(src && step && T >= 1 && nb >= 1 && R >= 1);
    return launch_beam_init(src, T, nb, R, step, as_stream(stream));
}

extern "C" int rgrg_debug_beam_advance(const int* src_old, int* src_new, const int* parent, int* step, int T, int R, void* stream) {
    RGRG_CHECK_ARG(src_old && src_new && src_old != src_new && parent && step && T >= 2 && R >= 1);
    hipStream_t st = as_stream(stream);
    std::vector<int> host(R + 1);
    RGRG_HIP(hipStreamSynchronize(st));
    RGRG_HIP(hipMemcpy(host.data(), parent, (size_t)R * sizeof(int), hipMemcpyDeviceToHost));
    RGRG_HIP(hipMemcpy(&host[R], step, sizeof(int), hipMemcpyDeviceToHost));
    if (host[R] < 0 || host[R] > T - 2) {
        set_error("rgrg_debug_beam_advance: *step = %d, a table of %d slots takes 0 .. %d", host[R], T, T - 2);
        return RGRG_EINVAL;
    }
    for (int r = 0; r < R; ++r)
        if (host[r] < 0 || host[r] >= R) {
            set_error("rgrg_debug_beam_advance: parent[%d] = %d, the table has rows 0 .. %d", r, host[r], R - 1);
            return RGRG_EINVAL;
        }
    return launch_beam_advance(src_old, src_new, parent, step, T, R, st);
}
