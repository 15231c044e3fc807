// What the decoder's translation units (decoder.hip: the decode step and the object; attn_decode.hip: the decode attention; decoder_beam.hip: beam search;
// decoder_beam_roll.hip: rolling-batch beam search; decoder_lm.hip: the teacher-forced and training passes; decoder_roll.hip: rolling-batch decoding, greedy and sampled) share: the rgrg_decoder object, its constants and the few host
// helpers that are called across those files.  Everything else is static in the file that uses it.
#pragma once
#include <deque>
#include <functional>
#include <vector>

#include "internal.h"

namespace rgrg {

constexpr int MAX_CHAINS = 4;   // row ranges of the many-sequence decode step (enqueue_step)
constexpr int PAD_ROWS = 32;
constexpr int SKINNY_MAX_ROWS = 128;  // 4 row tiles of 32 sequences per weight-streaming launch (RGRG_SKINNY_MAX_ROWS)
constexpr int BOS_ID = 50256, EOS_ID = 50256, PAD_ID = 50256;
constexpr int BEAM_K = 32;  // max 2*num_beams candidates per row (num_beams <= 16)
// What a decode step keeps its K/V cache in (rgrg_decoder_kv_format_in_use returns these values): fp32, the 16-bit type of the
// precision mode, or - opt-in, wherever the 16-bit cache would be used - OCP e4m3fn bytes (attn_kv8.hip)
enum KvFormat { KV_F32 = 0, KV_BF16 = 1, KV_F16 = 2, KV_E4M3 = 3 };
constexpr int KV8_CHUNK_KEYS = 144;   // keys of a full chunk of attn_decode_kv8_wave_kernel (9 loads x 16 groups)

// The bookkeeping of one greedy_search step (:629-650) for one row, run by ONE thread of the row's workgroup: a finished row
// takes PAD, the token goes to ids[row][t + 1], EOS finishes the row, and the LAST row to arrive records the first length
// at which every row is finished and advances the step counter.  Arrival and "this row is still unfinished" travel in ONE
// packed atomic (low 16 bits: tickets, high 16 bits: unfinished rows; S < 65536), so no fence and no second atomic order
// the two - the integer ticket keeps the result deterministic.  sync[0] = the packed word.  Shared by argmax_update_kernel
// (decoder.hip) and sample_kernel (sample.hip).  -> the token written; *was_finished: the row had finished before this step.
struct StepBook {
    long long* ids;   // [S][ld_ids]
    int ld_ids;
    int *finished, *step, *done_len, *sync;
    int S;
};
#ifdef __HIPCC__
__device__ __forceinline__ int record_step_token(const StepBook& bk, int row, int t, int tok, bool* was_finished = nullptr) {
    int fin = bk.finished[row];
    if (was_finished) *was_finished = fin != 0;
    if (fin) tok = PAD_ID;
    bk.ids[(size_t)row * bk.ld_ids + t + 1] = tok;
    if (tok == EOS_ID) fin = 1;
    bk.finished[row] = fin;
    const unsigned mine = fin ? 0u : 0x10000u;
    const unsigned old = atomicAdd(reinterpret_cast<unsigned*>(bk.sync), 1u + mine);
    if ((old & 0xffffu) == (unsigned)(bk.S - 1)) {  // every row has been recorded
        const unsigned unfinished = (old >> 16) + (mine >> 16);
        if (unfinished == 0 && *bk.done_len == 0) *bk.done_len = t + 2;
        *bk.step = t + 1;
        bk.sync[0] = 0;
    }
    return tok;
}

// First-occurrence arg-max of one row of NT (value, column) candidates by the row's workgroup of 256 threads (bv / bi: 4 words of
// LDS each): a thread requests its (up to 13) candidates up front with clamped indices - one memory latency instead of one per
// loop trip.  -> the column in thread 0 (0x7fffffff for a row without any comparable value: the callers take token 0); shared by argmax_update_kernel (decoder.hip)
// and roll_argmax_kernel (decoder_roll.hip).
constexpr int ARGMAX_U = 13;
__device__ __forceinline__ int argmax_candidates_row(const float* __restrict__ cv, const int* __restrict__ cx, int NT, float* bv, int* bi) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float v[ARGMAX_U];
    int ci[ARGMAX_U];
#pragma unroll
    for (int u = 0; u < ARGMAX_U; ++u) {
        const int i = min(tid + 256 * u, NT - 1);
        v[u] = cv[i];
        ci[u] = cx[i];
    }
    float best = -INFINITY;
    int idx = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < ARGMAX_U; ++u)
        if (tid + 256 * u < NT && (v[u] > best || (v[u] == best && ci[u] < idx))) { best = v[u]; idx = ci[u]; }
    for (int i = tid + 256 * ARGMAX_U; i < NT; i += 256) {   // more than 3328 candidates per row: not a shape of this model
        const float w = cv[i];
        const int wi = cx[i];
        if (w > best || (w == best && wi < idx)) { best = w; idx = wi; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = idx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
    }
    return idx;
}
#endif

struct Lin {
    const float* w = nullptr;  // [N,K]
    const float* b = nullptr;  // [N]
    float* packed = nullptr;   // skinny layout
    void* wb = nullptr;        // bf16 copy of w (opt-in many-sequence path)
    float* wT = nullptr;       // [K][Np] transposed copy, Np = N rounded up to 256 (backward pass: dX = dY W)
    void* wTb = nullptr;       // 16-bit copy of wT (training under autocast)
    int wb_f16 = 0, wTb_f16 = 0;   // the 16-bit type wb / wTb currently hold (0 bf16, 1 fp16)
    // 16-bit many-sequence decode with the LayerNorm in front of this GEMM folded in (enqueue_step): wb_ln[n][k] =
    // round16(gain[k] w[n][k]), cs16[n] = sum_k wb_ln[n][k] (of the ROUNDED values), c2_16[n] = b[n] + sum_k beta[k] w[n][k]
    void* wb_ln = nullptr;
    float *cs16 = nullptr, *c2_16 = nullptr;
    int wb_ln_f16 = -1;
    int N = 0, K = 0, NT = 0, KS = 1, ntile = 32;
    // fused decode plan (skinny_direct.inc): `packed` holds 16-column fragments, pre-scaled by the LayerNorm weight of
    // the LayerNorm this GEMM consumes when lnf is set; c1 / c2 are the folded vectors of that LayerNorm
    bool direct = false, lnf = false;
    float *c1 = nullptr, *c2 = nullptr;
    // 16-bit-weight variant of the fused plan (33-128 rows under autocast, round 6): `packed` rounded to the autocast type, and
    // the column sums of those ROUNDED values (lnf)
    void* packed16 = nullptr;
    float* c1_16 = nullptr;
    int packed16_f16 = -1;
};

struct LayerW {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    Lin c_attn, attn_proj, c_fc, mlp_proj;
};

// Everything that shapes the launches of one decode step (enqueue_step).  The pointers are buffers of the decoder; a captured step
// bakes them in, so two steps may share a graph exactly when their specs are equal (step_graph).
enum StepEnd {
    STEP_ARGMAX,   // arg-max and the bookkeeping of record_step_token
    STEP_LOGITS,   // d->logits, nothing else (forward(use_cache=True))
    STEP_SAMPLE,   // d->logits, then the sampler and its bookkeeping (enqueue_sampler)
    STEP_BEAM,     // d->logits, then the ranking of nb beams per item in G groups, which the caller enqueues behind the step (G = 0: plain)
    STEP_BEAM_SAMPLE,  // d->logits, then the beam-sampling ranking of nb beams per item (beam_sample.hip), enqueued by the caller likewise
    STEP_ROLL,         // arg-max into d->roll.arg, then the retire-and-refill kernels of rolling-batch decoding (decoder_roll.hip enqueue_roll_end)
    STEP_ROLL_SAMPLE   // d->logits, then the rolling sampler into d->roll.arg and the same two kernels (decoder_roll.hip enqueue_roll_sample_end)
};
struct StepSpec {
    int rows = 0;                      // sequences, or beam rows
    const int* tok = nullptr;          // [rows] the tokens to embed; NULL: the id buffer at *d->step
    const int* src = nullptr;          // [rows][T] ancestor table: the cache row that holds each slot of a beam row; NULL: the row itself
    const int* row_pos = nullptr;      // [rows] embedding positions; NULL: *d->step
    const int* kv_first = nullptr;     // [rows] 16-bit cache: the attention skips slots 1 .. kv_first[r] (padding in front of a prompt)
    const float* key_mask = nullptr;   // [rows][T] fp32 cache: added to the scores of the slots
    const int* row_step = nullptr;     // [rows] every row at a step of its own: key count t + 2 and slot t + 1 per row; NULL: *d->step for all
    StepEnd end = STEP_ARGMAX;
    int nb = 0, G = 0;                 // STEP_BEAM (nb, G), STEP_BEAM_SAMPLE (nb)
    bool roll_prompt = false;          // STEP_ROLL / STEP_ROLL_SAMPLE: the prompt refill behind the refill (a session with max_prompt_length > 0)
    bool operator==(const StepSpec& o) const {
        return rows == o.rows && tok == o.tok && src == o.src && row_pos == o.row_pos && kv_first == o.kv_first && key_mask == o.key_mask &&
               row_step == o.row_step && end == o.end && nb == o.nb && G == o.G && roll_prompt == o.roll_prompt;
    }
};

// What changes from call to call of rolling-batch decoding (decoder_roll.hip): the kernels of a captured step read it from a device
// block.  A call decodes S sequences, n per feature row: sequence q belongs to feature row q / n.
struct RollReq;
struct RollCall {
    long long* ids;       // [S][ld] the caller's output: column 0 BOS, PAD behind a sequence's last token
    int* len;             // [S] tokens of every sequence, BOS included (0 until it has ended)
    const float* ukv;     // [S / n][ld_ukv] image key / value rows of every layer (the ukv GEMM's output), one per FEATURE row
    int ld, S, max_length, ld_ukv;
    float* lp;            // [S][ld] log-probs of the drawn tokens (rolling sampling), or NULL
    int n;                // sequences (hypotheses) per feature row
    // Only the STORAGE is a ring (a rolling session): sequence q writes row q % C of ids / lp / len and reads row
    // (q / n) % Cf of ukv.  A one-shot call passes C = S and Cf = S / n: q % C == q, the caller's buffers as they are.
    int C, Cf;
    // The request ring of a rolling session: entry q % C holds what sequence q asked for.  NULL - the one-shot calls,
    // rolling beam search, the test hooks without a ring - is the call's max_length, EOS alone and the parameter block of the step.
    const RollReq* req;
    // The prompt rings of a rolling session opened with max_prompt_length = MP > 0, one row per FEATURE row, row
    // (q / n) % Cf like ukv: ptok [Cf][MP] the prompt's tokens, plen [Cf] its length P (1 = BOS alone, a submit without a prompt),
    // pkv the prompt's keys / values in the cache's element format, planes [layer][2][Cf][H][MP][64] of which slots 1 .. P - 1 are
    // written (the last prompt token runs through the row's decode step).  NULL / 0: no prompts.
    const int* ptok;
    const int* plen;
    const void* pkv;
    int MP;
};

// What one sequence of a rolling session asked for (include/rgrg_hip.h "Request ring" states the layout for the test hooks): 40 bytes,
// written by roll_submit_kernel for every new sequence, read by roll_retire_kernel and roll_sample_kernel for the sequence a row holds.
// A greedy session uses max_length, stop and flags only.
constexpr unsigned ROLL_REQ_CANCEL = 1u;      // flags: rgrg_decoder_roll_cancel has reached the sequence
constexpr unsigned short ROLL_NO_STOP = 0xffffu;
constexpr int ROLL_MAX_STOPS = 4;
struct RollReq {
    unsigned long long seed;    // the Philox key of the sequence's draws
    float inv_T;                // 1 / temperature
    int top_k;
    float top_p;
    int max_length;             // the sequence's own limit, 2 .. the session's
    int q0;                     // the counter row of the draws is q - q0 (0: the session's numbering)
    unsigned short stop[ROLL_MAX_STOPS];   // token ids that end the sequence as EOS does; ROLL_NO_STOP = unused
    unsigned flags;
};
static_assert(sizeof(RollReq) == 40, "RollReq is 40 bytes (include/rgrg_hip.h)");

// BeamHypotheses of transformers 4.19.2 restated on the host (decoder_beam.hip): hypothesis scores, worst_score and the is_done test are
// double arithmetic (HF does them on Python floats obtained through .item()), beam scores stay float32
struct BeamHyp { double score; std::vector<long long> toks; };
struct BeamHyps {
    std::vector<BeamHyp> beams;
    double worst = 1e9;
    void add(const std::vector<long long>& toks, double sum_logprobs, int nb, double lp);
    bool is_done(double best_sum_logprobs, int cur_len, bool early, int nb, double lp) const;
};

// The host state of the rolling beam loop (decoder_beam_roll.hip), which the one-shot call keeps for a call and the session
//  between its calls.  Per row of the Ru = G * nb rows: the hypothesis so far, and what the next step is fed - token,
// beam score, turn (the parent row, TURN_FRESH or TURN_IDLE).  Per slot: the region it holds (-1 = idle), that region's cur_len and
// `done` flag.  refill: the (first row, region) pairs of the slots seated for the next step.  src_cur / src_nxt: the ancestor tables.
struct BeamRollState {
    int nb = 0, G = 0, Ru = 0, max_length = 0, early = 0, use_graph = 0, nrefill = 0, occupied = 0;
    bool wide = false;
    double lp = 1.0;
    std::vector<std::vector<long long>> ids, nids;
    std::vector<float> beam_scores, nscore, h_score;
    std::vector<int> beam_tok, turn, ntok, nidx, h_tok, h_beam, refill, cur_len;
    std::vector<long long> region;
    std::vector<char> done;
    int *src_cur = nullptr, *src_nxt = nullptr;
};

struct GraphEntry {
    StepSpec spec;   // the step the graph was captured for
    hipGraphExec_t exec;
};

}  // namespace rgrg

struct rgrg_decoder {
    int n_layer, D, H, V, max_seqs, rows, T, max_len;
    const float* wte;
    const float *lnf_g, *lnf_b;
    rgrg::Lin fst0, fst2, ukv, lm_head;
    std::vector<rgrg::LayerW> layers;
    // workspace
    float *feats, *h1, *img, *ukv_out, *x, *x2, *xn, *qkv, *att, *ff, *logits, *part, *kv, *cand_val, *gemm_ws;
    size_t gemm_ws_floats;
    int* cand_idx;
    size_t kv_layer_stride, kv_kv_stride;
    int ld_logits, ld_ukv;
    long long* ids;
    int *next, *finished, *step, *done_len, *sync;
    // beam search
    int *src_a, *src_b, *beam_tok, *beam_parent, *cand_tok, *cand_beam, *top_tok;
    float *beam_scores, *row_max, *row_logsum, *top_val, *cand_score;
    float *wide_val = nullptr, *wide_score = nullptr;   // more than 16 beams: [rows][K] row candidates, [items][num_beams * K] scores
    int* wide_tok = nullptr;
    size_t wide_cap = 0;                                 // rows * K the wide buffers were sized for
    float* group_penalty = nullptr;                      // diverse beam search: the device word the captured group step reads its penalty from
    // sampling (decoder_sample.hip): device-side parameter block the captured step reads, log-probs [rows][max_len]
    void* sample_prm = nullptr;
    float* sample_lp = nullptr;
    float* bsample_s = nullptr;   // beam sampling: s of the row candidates [rows][BEAM_K], next to their keys (top_val) and tokens (top_tok)
    int* h_done;  // pinned: [0] final read, [1..2] the two in-flight "all finished" polls of the greedy loop
    hipEvent_t ev_poll[2] = {nullptr, nullptr};
    // Token-id validation of the teacher-forced passes, without a host round trip.  id_error[0]: raised by the CURRENT
    // pass (embedding / cross-entropy kernels) when an id is outside [0, vocab), cleared when a pass starts - it poisons
    // THAT pass's loss and gradients (NaN).  id_error[1]: sticky "some pass failed and has not been reported yet",
    // folded from [0] at the end of every pass and copied to the pinned mirror; the next call that finds the mirror set
    // reports torch.nn.Embedding's IndexError and clears both.
    int* id_error = nullptr;
    int* h_id_error = nullptr;
    hipStream_t stream;
    hipEvent_t ev_in;
    std::vector<rgrg::GraphEntry> graphs;
    std::vector<void*> allocs;
    size_t gemm_bytes_per_step = 0;
    double gemm_flops_per_step = 0.0;
    // teacher-forced pass workspace (grown on demand, rgrg_decoder_lm_forward; decoder_lm.hip tf_reserve)
    struct TfWork {
        float *x = nullptr, *xn = nullptr, *qkv = nullptr, *att = nullptr, *ff = nullptr, *logits = nullptr, *ws = nullptr,
              *row_loss = nullptr;
        int* row_valid = nullptr;
        size_t rows = 0, ws_floats = 0;
        const long long* pos = nullptr;   // position_ids of the NEXT teacher-forced pass (rgrg_decoder_set_lm_positions), [pos_rows] int64
        int pos_rows = 1;
        void free() {
            float** fs[] = {&x, &xn, &qkv, &att, &ff, &logits, &ws, &row_loss};
            for (float** f : fs) { if (*f) (void)hipFree(*f); *f = nullptr; }
            if (row_valid) (void)hipFree(row_valid);
            row_valid = nullptr;
            rows = 0;
            ws_floats = 0;
        }
    } tf;
    // training pass (rgrg_decoder_lm_loss_grad; decoder_lm.hip tr_reserve): saved activations and gradient work space, grown on demand
    struct TrWork {
        float *xs = nullptr, *qkv = nullptr, *ffpre = nullptr, *ff = nullptr, *dx = nullptr, *dbig = nullptr, *dxn = nullptr,
              *logits = nullptr, *dukv = nullptr, *t1 = nullptr, *t2 = nullptr, *dimg = nullptr, *dh1 = nullptr, *row_lse = nullptr,
              *att = nullptr, *lse = nullptr, *delta = nullptr;
        int* count = nullptr;
        size_t rows = 0, seqs = 0;
        // 16-bit activation flow of the training pass (autocast, > 128 token rows; round 5): every GEMM input is written as 16 bit
        // by its producer - LayerNorm outputs, attention outputs, gelu outputs + the saved c_fc pre-activations of every layer,
        // masked gradients, d(c_fc output), d(qkv), d(logits) of the chunk
        unsigned short *xn16 = nullptr, *att16 = nullptr, *ff16 = nullptr, *ffpre16 = nullptr, *dx16 = nullptr, *dff16 = nullptr,
                       *dqkv16 = nullptr, *dl16 = nullptr;
        // ... and, for T + 1 <= 128 keys, the 16-bit attention kernels (attn_train16.hip): q / k / v and the attention output of
        // every layer kept as 16 bit, d(attention output) and the image key / value of slot 0 as 16 bit
        unsigned short *qkv16 = nullptr, *datt16 = nullptr, *ukv16 = nullptr;
        bool a16 = false;
        bool h16 = false;       // what the current training work space was reserved for
        size_t chunk = 0;       // token rows per lm_head / cross-entropy chunk of that reservation
        bool seen_a16 = false, seen_a32 = false, seen_h16 = false, seen_h32 = false, seen_h16_a32 = false;   // tr_reserve: modes seen
        bool have_wT = false;
        void* a16_scratch = nullptr;   // bf16 copy of an fp32 GEMM input (teacher-forced / training passes under autocast); outlives free()
        size_t a16_bytes = 0;
        void free() {   // the work space of tr_reserve (not the weight copies, not a16_scratch)
            float** fs[] = {&xs, &qkv, &ffpre, &ff, &dx, &dbig, &dxn, &logits, &dukv, &t1, &t2, &dimg, &dh1, &row_lse, &att, &lse, &delta};
            for (float** f : fs) { if (*f) (void)hipFree(*f); *f = nullptr; }
            if (count) (void)hipFree(count);
            count = nullptr;
            unsigned short** hs[] = {&xn16, &att16, &ff16, &ffpre16, &dx16, &dff16, &dqkv16, &dl16, &qkv16, &datt16, &ukv16};
            for (unsigned short** h : hs) { if (*h) (void)hipFree(*h); *h = nullptr; }
            rows = seqs = 0;
            chunk = 0;
        }
    } tr;
    int bf16_gemms = 0;  // 1 (bf16) / 2 (fp16): 16-bit-weight MFMA GEMMs on the many-sequence path (not bit-exact; opt-in)
    int f16() const { return bf16_gemms == 2 ? 1 : 0; }   // the 16-bit type of that mode
    unsigned short *xn16 = nullptr, *att16 = nullptr, *ff16 = nullptr;  // bf16 activations of that path (GEMM inputs)
    float* sk_ws = nullptr;     // split-K work space of the N = 1024 projections of the many-sequence decode step (gemm_bf16.hip)
    unsigned* sk_cnt = nullptr;
    int sk_attn = 0, sk_mlp = 0; // K slices of attn_proj / mlp_proj there (RGRG_SK_ATTN / RGRG_SK_MLP; 1 = off; -1 = automatic: 2 / 4 slices for a
                                 // step of <= 256 rows - 32-64 output tiles for 256 CUs - and none above)
    int step_rows = 0;           // token rows of the many-sequence step being enqueued (all row ranges together)
    float* ln_stat = nullptr;   // [rows][16][2]: per-row (sum, sum of squares) slots (one per 64 columns) of the residual stream (folded LayerNorm)
    bool ln_fold = true;        // 16-bit path: LayerNorms folded into the GEMMs around them; RGRG_LN_FOLD=0: ln_rows launches (A/B)
    float* key_mask = nullptr;             // [rows][T] additive padding mask of the cache slots (forward(use_cache=True) with padding, padded prompts)
    // rgrg_decoder_trace_step: one hipEvent after every launch of an eagerly enqueued step, on the stream it was launched on
    struct TraceMark { hipEvent_t ev; int r0; int tag; };
    std::vector<TraceMark>* trace = nullptr;
    bool w16_fused = true;      // under autocast 33-128 rows run the fused plan on 16-bit weights (skinny_direct.inc W16); RGRG_W16_FUSED=0: the
                                // many-sequence 16-bit path from 33 rows on (A/B)
    bool qkv_cache = true;      // plain 16-bit many-sequence steps: c_attn stores k / v into cache slot t + 1, the attention reads q only
                                // (decoder.hip step_qkv_cache); RGRG_QKV_CACHE=0: the fp32 q | k | v row and the attention's own cache store (A/B)
    int kp_gemms = 2;           // ... and run on the K-parity ping-pong kernel (gemm_kp.inc, round 6): RGRG_GEMM_KP = 0 none (the LDS-DMA kernel), 1 all four,
                                // 2 (default) the producers only (attn_proj / mlp_proj, N = 1024), 3 the consumers only (c_attn / c_fc, 128 x 128 row-split kernel).
                                // Measured per mode: profiles/r06_step_trace_v3.log
    int gemm_launches_per_step = 0;
    int* row_pos = nullptr;                  // [rows] per-row embedding positions (StepSpec::row_pos of forward(use_cache=True) and padded prompts)
    // a left-padded prompt (decoder_prompt.hip): padded prompt slots of every row - on the 16-bit cache also StepSpec::kv_first of the
    // steps behind it, whose kernel skips cache slots 1 .. prompt_pad[s] instead of adding a mask - and the prompt's position ids
    int* prompt_pad = nullptr;               // [rows]
    long long* prompt_pos = nullptr;         // [rows][max_len]
    int* beam_pad = nullptr;                 // [rows] rgrg_decoder_beam_search_prompted: prompt_pad of every beam row's item
    // > 0: the last greedy generate ran the lm_head with the arg-max epilogue for this many rows - d->logits was not written;
    // rgrg_decoder_copy_last_logits recomputes it from the retained ln_f output (xn16) before copying
    int logits_stale_rows = 0;
    bool logits_valid = false;   // d->logits / the retained ln_f rows belong to the last step of a completed generate / beam / cached call (ADVICE r05:
                                 // the timing hooks and a precision change overwrite them - rgrg_decoder_copy_last_logits then refuses)
    // enqueue_step: extra streams + fork / join events of the multi-range many-sequence step (RGRG_DECODE_CHAINS)
    hipStream_t streams_x[rgrg::MAX_CHAINS - 1] = {};
    hipEvent_t ev_fork = nullptr, ev_join[rgrg::MAX_CHAINS - 1] = {};
    int kv8 = 0;      // rgrg_decoder_set_kv_format: 1 = the many-sequence 16-bit step keeps its K/V cache as e4m3 bytes (attn_kv8.hip); survives
                      // precision changes and has no effect where the cache is fp32 (fp32 mode, the fused plans, forward_cached)
    // rolling-batch decoding, greedy and sampled (decoder_roll.hip).  Per decoder row [rows]: the sequence it holds (-1 = idle), that sequence's
    // length so far (BOS included), the token and the embedding position of its next step, its step (= the key count - 2), the arg-max
    // - or the drawn token - of the step just run; list[2 k], list[2 k + 1] = row and sequence of the k-th refill of the step; shared[0] = the next pending
    // sequence, [1] = unfinished sequences, [2] = refills of the step, [3] = steps that had an active row.  call: the device block of
    // RollCall the captured kernels read what changes from call to call from; ukv [ukv_seqs][ld_ukv]: the image key / value rows of
    // every feature row of the call (grown on demand, freed with the decoder)
    struct RollWork {
        int *seq = nullptr, *len = nullptr, *tok = nullptr, *pos = nullptr, *step = nullptr, *arg = nullptr, *list = nullptr, *shared = nullptr;
        void* call = nullptr;
        float* ukv = nullptr;
        size_t ukv_seqs = 0;
        int host_refills = 0;   // enqueue_roll_refill_list: the host word the refill count is copied from
    } roll;
    // Every decode entry that rewrites the cache rows, the step plan or the rolling state bumps the epoch (decode_begin and the
    // entries that wait for the caller's stream themselves); an open rolling session remembers the one it was opened in.
    unsigned long long epoch = 0;
    // The rolling session (decoder_roll.hip): one per decoder.  ids / lp / len are the output rings the decoder owns
    // ([C][max_length], [C]); h_len (pinned) mirrors len as of the last synchronisation, with 0 for every sequence submitted since.
    struct RollSession {
        bool open = false;
        unsigned long long epoch = 0;
        rgrg::RollCall call{};          // the host's copy of the device block (S = sequences submitted so far)
        int R = 0, use_graph = 0;
        rgrg::StepEnd end = rgrg::STEP_ROLL;
        long long watermark = 0;        // the lowest sequence number not yet released
        long long unfinished = 0;       // as of the last synchronisation, plus what was submitted since
        bool drained = true;            // the last poll said 0 and no submit has come since: advance launches nothing
        bool counted = false;           // the first eager step has been counted into the GEMM statistics
        int steps = 0;                  // the device's count of steps that had an active row, as of the last synchronisation
        long long* ids = nullptr;
        float* lp = nullptr;
        int* len = nullptr;
        int* h_len = nullptr;
        // the request ring [C] and what a submit without a request writes into it: the session's own parameters
        rgrg::RollReq* req = nullptr;
        rgrg::RollReq defaults{};
        // the prompt rings (max_prompt_length = call.MP > 0 only): device ptok / plen / pkv as RollCall states them,
        // h_ptok / h_plen their pinned sources (a ring row is rewritten only after its sequences have been released), pids the
        // int64 [prompt_chunk] token rows of one teacher-forced pass, prompt_chunk the token rows the work space was reserved for
        int *ptok = nullptr, *plen = nullptr, *h_ptok = nullptr, *h_plen = nullptr;
        void* pkv = nullptr;
        long long* pids = nullptr;
        int prompt_chunk = 0;
    } sess;
    // The rolling beam session (decoder_beam_roll.hip): one per decoder, and never next to `sess`.  Regions are numbered
    // over the life of the session; `next` is the lowest one not yet seated (pending: next .. submitted - 1), hyps / finalized hold
    // regions watermark .. submitted - 1.  The image key / value ring is roll.ukv [capacity][ld_ukv], row q % capacity.
    struct BeamRollSession {
        bool open = false;
        unsigned long long epoch = 0;
        rgrg::RollCall call{};          // what the device block holds: ukv, ld_ukv, n = 1, Cf = capacity
        rgrg::BeamRollState st;
        int capacity = 0, keep = 0, steps = 0;
        long long submitted = 0, watermark = 0, next = 0;
        std::deque<rgrg::BeamHyps> hyps;
        std::deque<char> finalized;
    } bsess;
    int chains = 4;   // round 5 (LDS-DMA kernel everywhere): 1 -> 81.6, 2 -> 82.8, 3 -> 85.4, 4 -> 85.1 images/s at BASELINE configs[2]
                      // (profiles/r05_decode_row_ranges_ab.log); round 6, attn_proj / mlp_proj on the K-parity kernel: ms per decode step
                      // 2.89 (3 ranges, round-5 kernels), 2.83 (3), 2.785 (4) - profiles/r06_step_trace_v3.log
};

namespace rgrg {

inline int pad256(int n) { return (n + 255) / 256 * 256; }  // K granularity of the bf16 GEMM pipeline

// decoder.hip
int dmalloc(rgrg_decoder* d, void** p, size_t bytes, bool zero);
int skinny_max_rows();
int linear(rgrg_decoder* d, const Lin& l, const float* X, const float* R, float* Y, int M, int ldy, int act,
           bool count, const unsigned short* X16 = nullptr, unsigned short* Y16 = nullptr, const GemmLnFold* ln = nullptr);
int launch_ln_rows(const float* x, const float* g, const float* b, float* xn, int D, unsigned short* xn16, int f16, int rows,
                   hipStream_t st);   // ln_rows_kernel, one wave per row
int enqueue_step(rgrg_decoder* d, const StepSpec& s, bool count);
// the graph of step `s`: captured on d->stream the first time the spec is seen - body() enqueues the step and whatever belongs to
// it (rows prepared in front, a ranking behind) -, found by equality afterwards
int step_graph(rgrg_decoder* d, const StepSpec& s, const std::function<int()>& body, hipGraphExec_t* exec);
// the step behind a left-padded prompt whose padded slots per row are in `pad`: positions from d->row_pos (the caller's kernel fills
// them in front of every step), the padded slots out of the attention through the slot mask (fp32 cache) or `pad` itself (16 bit)
StepSpec padded_step_spec(rgrg_decoder* d, StepSpec s, const int* pad);
int enqueue_prefill(rgrg_decoder* d, const float* feats, int S, int row_mul = 1);
int decode_begin(rgrg_decoder* d, void* stream);
// attn_decode.hip.  One decode-attention launch on plain device pointers: the variant and grid rules of the product path.
// launch_attention (decoder.hip) fills it from the decoder object, the test hooks rgrg_debug_attn_decode* from their arguments - the
// rules exist once, in launch_attn_decode.
struct AttnDecodeLaunch {
    const float* qkv; int ld_qkv;          // [S][ld_qkv]: q | k | v of the current token, D floats each
    void *kc, *vc;                         // K / V plane [rows][H][T][64]: fp32, 16 bit or e4m3 bytes (fmt)
    size_t plane_elems;                    // elements of one plane (16 bit / e4m3: bounds the 32-bit byte offsets of the buffer loads)
    const int* step;
    float* out; unsigned short* out16;
    int S, H, T;
    const int* src;                        // beam search: [S][T] ancestor table, or NULL
    const float* kmask;                    // [S][T] additive padding mask of the cache slots, or NULL (fp32 kernel only)
    KvFormat fmt;                          // KV_F32, KV_BF16 / KV_F16 (one kernel; the type is f16), KV_E4M3
    int f16;                               // the 16-bit type of a 16-bit cache and of out16 (0 bf16, 1 fp16)
    int ni;                                // fp32 kernel: 9 / 2 keys per group and chunk; 0 = S * H <= 4096 ? 9 : 2
    int frag_out;
    int max_wgs;                           // wave kernels (16 bit, e4m3): > 0 caps the grid, each wave then walks several (sequence, head) items
    hipStream_t st;
    bool q_only = false;                   // 16-bit cache without src: slot t + 1 already holds the new k / v (c_attn's K/V-cache epilogue) -
                                           // the kernel reads q only and stores nothing to the cache
    const int* first = nullptr;            // 16-bit cache: [S] padded prompt slots, cache slots 1 .. first[s] are left out (with src: not q_only)
    const int* row_step = nullptr;         // fp32 / 16-bit cache: [S] the step of every row on its own, instead of the one word *step (rolling-batch
                                           // decoding); plain or with src (rolling beam search) - no mask, no padded slots, not q_only
};
int launch_attn_decode(const AttnDecodeLaunch& a);
// attn_kv8.hip: attn_decode_kv8_wave_kernel on `workgroups` workgroups of 4 waves (grid and argument rules: launch_attn_decode)
int launch_attn_decode_kv8(const float* qkv, int ld_qkv, uint8_t* kc, uint8_t* vc, const int* step, float* out, unsigned short* out16,
                           int S, int H, int T, const int* src, int f16, int workgroups, hipStream_t st);
// prologue: work enqueued between the prefill and the first step that already produced the tokens of steps 0 .. steps_done - 1
// (a prompt pass, decoder_prompt.hip); the loop then runs the remaining limit - 1 - steps_done steps
struct DecodePrologue { int (*fn)(rgrg_decoder*, int S, const void* arg); const void* arg; int steps_done; };
// step: STEP_ARGMAX or STEP_SAMPLE; prepare (or NULL): enqueued in front of every step (the rows of a padded prompt)
int run_decode_loop(rgrg_decoder* d, const float* feats, const StepSpec& step, int (*prepare)(rgrg_decoder*, int S), int limit,
                    int use_graph, int64_t* out_ids, int out_ld, float* out_logprobs, int* out_len,
                    const DecodePrologue* prologue = nullptr);
bool lm_head_cand_path(const rgrg_decoder* d, int S);   // greedy many-sequence 16-bit step: the lm_head leaves arg-max candidates, no logits
// the end of a greedy step on its own: lm_head over the ln_f rows in d->xn (and d->xn16 where the step plan of S rows reads 16-bit
// activations), arg-max, record_step_token at *d->step
int enqueue_head_argmax(rgrg_decoder* d, int S);
// ... and in its logits-leaving form (the form beam search and sampling rank): d->logits rows [0, S), nothing else
int enqueue_head_logits(rgrg_decoder* d, int S);
// additive slot mask [R][T] of beam rows behind a left-padded prompt: -1e4 on slots 1 .. first[r], 0 elsewhere
int launch_beam_first_mask(const int* first, int R, int T, float* kmask, hipStream_t st);

// decoder_lm.hip: embedding .. ln_f of the teacher-forced pass over S x T token rows; leaves the ln_f rows in d->tf.xn (the image
// key / value of every layer must be in d->ukv_out, the work space reserved with tf_reserve).  after_qkv (or NULL) runs behind
// every layer's c_attn with that layer's q | k | v rows [S*T][3D] (fp32).
// decoder_prompt.hip: the prompt of rgrg_decoder_beam_search_prompted, one per ITEM.  enqueue_beam_prompt runs between the prefill
// and the first ranking: mask scan and refusals (one read-back), the teacher-forced pass over the S x T prompt rows with keys /
// values into slots 1 .. T of cache row s * nb, both ancestor tables pointing slots 0 .. T of every beam row there, *step = T - 1,
// and the ln_f row of every item's last prompt position in the lm_head input of its nb rows.  -> *padded, host_ids [S][T].
struct BeamPrompt { const long long* ids; const float* am; int T; };
int enqueue_beam_prompt(rgrg_decoder* d, const BeamPrompt& p, int S, int nb, bool* padded, std::vector<long long>* host_ids);
// in front of every beam step behind a left-padded prompt: the rows' embedding positions (beam_row_pos_kernel)
int enqueue_beam_row_pos(rgrg_decoder* d, int R);
// decoder_beam.hip: rgrg_decoder_beam_search, from a prompt when one is given
// groups (or NULL = plain beam search): num_beam_groups and the Hamming diversity penalty of rgrg_decoder_group_beam_search
struct BeamGroups { int G; float penalty; };
// sample (or NULL; never together with groups): beam-search sampling - the ranking of beam_sample.hip under these parameters (the
// caller has checked them and num_beams <= BEAM_K / 2)
struct BeamSample { float temperature; int top_k; float top_p; unsigned long long seed; };
int beam_search_run(rgrg_decoder* d, const float* feats, int S, int num_beams, int max_length, int early_stopping, float length_penalty,
                    int num_return_sequences, int64_t* out_ids, int out_ld, int* out_len, void* stream, const BeamPrompt* prompt,
                    const BeamGroups* groups = nullptr, const BeamSample* sample = nullptr);
// the refusals the two beam-sampling entries share, each with a message
int check_beam_sample(const char* who, int num_beams, int num_return_sequences, float temperature, int top_k, float top_p);
// beam_sample.hip: the row and item launches of the beam-sampling ranking over S items of nb <= BEAM_K / 2 rows of logits [S * nb][ld];
// parameters from the device block prm_dev or, when null, from *prm_val (both SampleParams); t = *step_dev or, when null, step;
// row lists [S * nb][BEAM_K] -> out_score / out_tok / out_beam [S][2 nb]
int launch_beam_sample_rank(const float* logits, size_t ld, int V, int S, int nb, const float* beam_scores, const void* prm_dev,
                            const void* prm_val, const int* step_dev, int step, int row0, float* row_key, float* row_s, int* row_tok,
                            float* out_score, int* out_tok, int* out_beam, hipStream_t st);
int check_beam_groups(const char* who, int num_beams, int num_beam_groups, float diversity_penalty, int num_return_sequences);
// decoder_beam.hip, shared with the rolling loop (decoder_beam_roll.hip): the plain ranking's two launches and the one place that chooses
// their kernel (K = 2 num_beams > BEAM_K: the K-round kernels on candidate rows K wide), the wide buffers for R rows, and the ONE
// restatement of BeamSearchScorer - process (one item, one group's candidate list), finalize (one item), the padded output
bool beam_wide(int K, bool force_wide = false);
void launch_beam_row_topk(const float* logits, int ld, int V, int rows, int K, float* row_max, float* row_logsum, float* top_val,
                          int* top_tok, bool force_wide, hipStream_t st);
void launch_beam_merge(const float* row_max, const float* row_logsum, const float* top_val, const int* top_tok, const float* beam_scores,
                       int S, int nb, int V, float* score, float* out_score, int* out_tok, int* out_beam, bool force_wide, hipStream_t st);
int beam_reserve_wide(rgrg_decoder* d, int R, int K);
int beam_process_group(BeamHyps& hyps, char& done, const float* sc, const int* tok, const int* beam, int gs, int nb, int item_row0,
                       const std::vector<std::vector<long long>>& ids, int cur_len, bool early, double lp, float* nscore, int* ntok,
                       int* nidx);
void beam_finalize_item(BeamHyps& hyps, bool done, const std::vector<long long>* rows, const float* scores, int nb, double lp);
int beam_write_best(const std::vector<BeamHyps>& hyps, int keep, int max_length, int64_t* out_ids, int out_ld, int* out_len, hipStream_t st);
// decoder_sample.hip: the sampler behind the logits of S rows (the end of a STEP_SAMPLE step) and the start of every sampling entry
int enqueue_sampler(rgrg_decoder* d, int S);
int sample_begin(rgrg_decoder* d, int S, float temperature, int top_k, float top_p, uint64_t seed, void* stream);
// decoder_roll.hip: the end of a STEP_ROLL step - the arg-max of R rows over their NT candidates, retire, refill
// (prompt: StepSpec::roll_prompt - the prompt refill behind the refill)
int enqueue_roll_end(rgrg_decoder* d, int R, int NT, bool prompt = false);
// ... and of a STEP_ROLL_SAMPLE step: the rolling sampler over the R logits rows, retire, refill
int enqueue_roll_sample_end(rgrg_decoder* d, int R, bool prompt = false);
// ... and what rolling beam search (decoder_beam_roll.hip) shares with them: the work space for S feature rows, the refusals (R rows,
// max_length, the e4m3 cache), feature_space_transformation_nn and the uk / uv GEMM of the S feature rows -> roll.ukv, and
// roll_refill_kernel alone over a HOST-written refill list: n (row, feature row) pairs -> roll.list / roll.shared, then the launch
int roll_reserve(rgrg_decoder* d, int S);
int roll_check(rgrg_decoder* d, const char* who, int R, int max_length);
int enqueue_roll_prefill(rgrg_decoder* d, const float* feats, int S, size_t ukv_row0 = 0);   // -> roll.ukv rows ukv_row0 .. + S - 1
void roll_session_free(rgrg_decoder* d);   // the session's rings (rgrg_decoder_destroy, close)
int enqueue_roll_refill_list(rgrg_decoder* d, const int* pairs, int n, int R);
// sample.hip: the rolling sampler - row r of logits [R][ld] holds sequence row_seq[r] (< 0: idle, nothing is written) at row_len[r]
// tokens; an active row draws with the Philox counter (sequence, len - 1), the token -> arg[r], its log-prob ->
// call->lp[sequence][len] (pitch call->ld; a NULL call->lp: no log-probs).  Parameters from the device block prm_dev - or, with a request ring (call->req), from
// the sequence's entry, the counter then being (sequence - q0, len - 1).
int launch_roll_sample(const float* logits, size_t ld, int R, int V, const void* prm_dev, const int* row_seq, const int* row_len,
                       const RollCall* call, int* arg, hipStream_t st);
int tf_reserve(rgrg_decoder* d, size_t rows);
// ... and the 16-bit copy of a GEMM input of `rows` token rows that a pass under autocast makes: reserved up front, the pass never waits
int tf_reserve_a16(rgrg_decoder* d, size_t rows);
// ukv (or NULL = d->ukv_out): the S image key / value rows [S][ld_ukv] the pass attends to in slot 0.
// kv_only (the prompt passes of a rolling session, which want every layer's q | k | v and nothing else): the pass ends behind the
// last layer's after_qkv - d->tf.xn is NOT the ln_f rows then - and its fp32 GEMMs take no split-K: every output element is one K
// loop in a fixed order, whatever the row count.
int tf_hidden_pass(rgrg_decoder* d, const long long* ids, const float* attention_mask, const long long* pos, int pos_rows, int S, int T,
                   int (*after_qkv)(rgrg_decoder*, int layer, const float* qkv, const void* arg) = nullptr, const void* arg = nullptr,
                   const float* ukv = nullptr, bool kv_only = false);
// decoder_prompt.hip: q | k | v rows [S*T][3D] (fp32) of one layer -> slots 1 .. T of the planes [rows][H][slots][64] (prompt_kv_store_kernel)
int launch_prompt_kv_store(const float* qkv, void* kplane, void* vplane, int S, int H, int T, int slots, int row_mul, bool kv16, int f16,
                           hipStream_t st);

}  // namespace rgrg
