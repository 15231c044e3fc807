// Rolling-batch decoding - greedy (rgrg_decoder_generate_rolling) and sampled (rgrg_decoder_sample_rolling): R decoder rows through which any number of sequences flow.  A row
// whose sequence has ended - EOS, or max_length tokens - takes the next pending sequence in the same step, so the work follows the
// sum of the sequence lengths instead of sequences x the longest one, and the K/V cache is sized by R.
//
// The step is the decode step of every other mode (enqueue_step) with per-row tokens, positions and - new - per-row steps
// (StepSpec::row_step: every attention item reads its own key count).  Its end (STEP_ROLL) is three launches:
//   roll_argmax_kernel   the row's arg-max over the step's candidates -> roll.arg[r]
//   roll_retire_kernel   ONE workgroup: append, retire, hand pending sequences to the free rows in ascending row order (a prefix
//                        scan, no atomics: which row gets which sequence is a function of the tokens alone)
//   roll_refill_kernel   the image key / value of every sequence handed out -> slot 0 of its row's cache, all layers
//   (a session with prompts, DESIGN.md 7.19, adds roll_prompt_refill_kernel: the prompt's keys / values from a ring -> slots 1 .. P - 1)
// What changes from call to call (output buffers, sequence count, max_length) is read from a device block, so one captured graph
// per (R, plan) serves every call.
//
// Rolling sampling (STEP_ROLL_SAMPLE) is the same step with logits left and roll_sample_kernel (sample.hip) in
// place of the arg-max: sequence q draws the token of column c under the Philox counter (q, c - 1), whichever row holds it.  A call
// decodes n sequences per feature row; they share that row's image key / value (ukv row q / n).
#include <algorithm>
#include <vector>

#include "decoder_internal.h"

namespace rgrg {

struct RollRows {
    int *seq, *len, *tok, *pos, *step, *list, *shared;
};
constexpr int ROLL_NEXT = 0, ROLL_UNFINISHED = 1, ROLL_REFILLS = 2, ROLL_STEPS = 3;

// a length word of the prompt ring, kept inside 1 .. MP whatever the ring holds (the host has checked it: no kernel indexes by trust)
__device__ __forceinline__ int roll_prompt_len(int P, int MP) { return min(max(P, 1), MP); }

__global__ __launch_bounds__(256) void roll_argmax_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_idx, int NT,
                                                          int* __restrict__ arg) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int row = blockIdx.x;
    const int idx = argmax_candidates_row(cand_val + (size_t)row * NT, cand_idx + (size_t)row * NT, NT, bv, bi);
    if (threadIdx.x == 0) arg[row] = idx == 0x7fffffff ? 0 : idx;
}

// The start of a call: the call block, every row idle, nothing handed out, and the output in its final form for a sequence that
// never runs a step (BOS, then PAD; log-probs 0).  One launch of roll_retire_kernel behind it hands out the first min(S, R) sequences.
__global__ __launch_bounds__(256) void roll_begin_kernel(const RollCall c, RollCall* __restrict__ call, const RollRows st, int R) {
    const size_t total = (size_t)c.S * c.max_length;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        c.ids[(i / c.max_length) * c.ld + (i % c.max_length)] = (i % c.max_length) == 0 ? BOS_ID : PAD_ID;
    if (c.lp)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
            c.lp[(i / c.max_length) * c.ld + (i % c.max_length)] = 0.f;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < c.S; s += gridDim.x * blockDim.x) c.len[s] = 0;
    if (blockIdx.x == 0) {
        for (int r = threadIdx.x; r < R; r += 256) {
            st.seq[r] = -1; st.len[r] = 0; st.tok[r] = BOS_ID; st.pos[r] = 0; st.step[r] = 0;
        }
        if (threadIdx.x == 0) {
            *call = c;
            st.shared[ROLL_NEXT] = 0; st.shared[ROLL_UNFINISHED] = c.S; st.shared[ROLL_REFILLS] = 0; st.shared[ROLL_STEPS] = 0;
        }
    }
}

// Retire and refill, one workgroup of 256 threads over the R rows in passes of 256 (tests/rolling_reference.py is the model):
//   an ACTIVE row (seq >= 0) appends arg[r] at ids[seq][len]; on EOS, or when that was the max_length-th token, the sequence's
//   length is recorded and the row is free; otherwise the token, len - 1 as position and step are the row's next input.
//   FREE rows - just retired, or idle - take the pending sequences next, next + 1, ... in ascending row order as long as there
//   are any: BOS, position 0, step 0 - behind a prompt of P tokens (call->plen): its last token, position and step P - 1, length P -,
//   and (row, sequence) goes to the refill list.  A free row without a sequence is idle: it
//   keeps the BOS state, runs along and writes nothing.
// `next` advances by the sequences handed out, not by the free rows.  Sequence q writes ring row q % C of the output.
// handout_only (the first hand-out of a call, a submit of a session): a row that holds a sequence is not touched - no append, no
// retire, arg is not read - and the pass is not a step; idle rows take pending sequences as above.
// With a request ring (call->req; tests/rolling_request_reference.py is the model) the limit is the sequence's own, its
// stop tokens end it like EOS (appended, the last token), and a sequence whose cancel flag is set is CUT: nothing is appended, its
// length is recorded NEGATIVE (-len, len >= 1 tokens kept) and the row is free like a retired one.  The flag is looked at for rows that
// hold a sequence on entry only: a pending sequence takes a row as usual and is cut in that row's next pass, as BOS alone.
__global__ __launch_bounds__(256) void roll_retire_kernel(const RollRows st, const int* __restrict__ arg, const RollCall* __restrict__ call,
                                                          int R, int handout_only) {
    __shared__ int wave_free[4];
    const RollCall c = *call;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int next0 = st.shared[ROLL_NEXT];
    int base_rank = 0;      // free rows in front of this pass
    int active_in = 0;      // this thread's rows that were active on entry
    for (int r0 = 0; r0 < R; r0 += 256) {
        const int r = r0 + tid;
        bool is_free = false;
        if (r < R) {
            const int seq = st.seq[r];
            is_free = seq < 0;
            if (seq >= 0 && !handout_only) {
                ++active_in;
                const int tok = arg[r];
                int len = st.len[r];
                const int slot = seq % c.C;
                int limit = c.max_length;
                bool stop = tok == EOS_ID, cut = false;
                if (c.req) {   // the sequence's own request (a session): its limit, its stop tokens, the cancel flag
                    const RollReq q = c.req[slot];
                    limit = min(q.max_length, c.max_length);   // (never beyond the row's width, whatever the entry says)
                    cut = (q.flags & ROLL_REQ_CANCEL) != 0u;
#pragma unroll
                    for (int i = 0; i < ROLL_MAX_STOPS; ++i) stop |= q.stop[i] != ROLL_NO_STOP && tok == (int)q.stop[i];
                }
                if (cut) {   // cancelled: the token of this step is not appended; the negative length tells the cut from an end
                    c.len[slot] = -len;
                    is_free = true;
                } else {
                    c.ids[(size_t)slot * c.ld + len] = tok;
                    ++len;
                    if (stop || len >= limit) {
                        c.len[slot] = len;
                        is_free = true;
                    } else {
                        st.len[r] = len; st.tok[r] = tok; st.pos[r] = len - 1; st.step[r] = len - 1;
                    }
                }
            }
        }
        // exclusive prefix count of the free rows of this pass: inside the wave from the ballot, across the 4 waves through LDS
        const unsigned long long b = __ballot(is_free);
        const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wave_free[wave] = __popcll(b);
        __syncthreads();
        int before = 0, pass_free = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wave_free[w];
            pass_free += wave_free[w];
        }
        if (is_free) {
            const int k = base_rank + before + in_wave;
            const int seq = next0 + k;
            const bool given = seq < c.S;
            // with prompt rings the sequence starts behind its prompt of P tokens: the last prompt token is the row's
            // next input, at position and step P - 1 (without rings: P = 1 and BOS)
            int P = 1, tok = BOS_ID;
            if (given && c.plen) {
                const int f = seq / c.n % c.Cf;
                P = roll_prompt_len(c.plen[f], c.MP);
                tok = c.ptok[(size_t)f * c.MP + P - 1];
            }
            st.seq[r] = given ? seq : -1;
            st.len[r] = given ? P : 0;
            st.tok[r] = tok; st.pos[r] = P - 1; st.step[r] = P - 1;
            if (given) { st.list[2 * k] = r; st.list[2 * k + 1] = seq; }
        }
        base_rank += pass_free;
        __syncthreads();   // wave_free is rewritten by the next pass
    }
    // base_rank = free rows of the step (the same in every thread)
    const int given = min(base_rank, c.S - next0);
    const unsigned long long any = __ballot(active_in > 0);
    if (lane == 0) wave_free[wave] = any != 0ull;
    __syncthreads();
    if (tid == 0) {
        st.shared[ROLL_NEXT] = next0 + given;
        st.shared[ROLL_REFILLS] = given;
        st.shared[ROLL_UNFINISHED] = (c.S - (next0 + given)) + (R - (base_rank - given));   // pending + rows that hold a sequence now
        if (wave_free[0] | wave_free[1] | wave_free[2] | wave_free[3]) st.shared[ROLL_STEPS] += 1;
    }
}

// The image key / value of every sequence handed out in this step (the refill list; ukv ring row (sequence / n) % Cf) -> cache slot 0 of its row, every layer, with
// kv_slot0_kernel's rounding for the cache format (16 bit: to16_rt; fp32: the value).  Grid (layers * 2, ROLL_REFILL_ROWS): workgroup
// (x, y) copies the D values of plane x for list entries y, y + gridDim.y, ...; a step without refills costs the empty launch.
constexpr int ROLL_REFILL_ROWS = 32;
constexpr int ROLL_PROMPT_CHUNK = 512;   // token rows of one teacher-forced pass over the prompts of a submit (the work space a session reserves)
template <typename KV>
__global__ __launch_bounds__(256) void roll_refill_kernel(const int* __restrict__ list, const int* __restrict__ shared,
                                                          const RollCall* __restrict__ call, KV* __restrict__ kv_all, size_t layer_stride,
                                                          size_t kv_stride, int H, int T, int f16) {
    const int n = shared[ROLL_REFILLS];
    const int l = blockIdx.x >> 1, kv = blockIdx.x & 1, D = H * 64;
    const float* ukv = call->ukv;
    const int ld = call->ld_ukv, per_row = call->n, Cf = call->Cf;
    for (int k = blockIdx.y; k < n; k += gridDim.y) {
        const int r = list[2 * k], seq = list[2 * k + 1] / per_row % Cf;
        for (int d = threadIdx.x; d < D; d += 256) {
            const int hd = d >> 6, e = d & 63;
            const float val = ukv[(size_t)seq * ld + ((size_t)l * 2 + kv) * D + d];
            const size_t o = (size_t)l * layer_stride + (size_t)kv * kv_stride + (((size_t)r * H + hd) * T) * 64 + e;
            if constexpr (sizeof(KV) == 2) kv_all[o] = (KV)to16_rt(val, f16);
            else kv_all[o] = val;
        }
    }
}

// The prompt's keys / values of every sequence handed out in this step (a session with prompt rings): slots 1 .. P - 1
// of ring row (sequence / n) % Cf of call->pkv -> the same slots of its row's cache, every layer.  Ring and cache hold the same element
// format, so these are bytes: per (row, head) the (P - 1) * 64 elements are contiguous on both sides, a lane moves 16 bytes
// (prompt_kv_store_kernel's piece), consecutive lanes consecutive pieces.  Grid as roll_refill_kernel: workgroup (x, y) serves plane x
// of list entries y, y + gridDim.y, ...; a prompt of one token (a submit without a prompt) has nothing to copy.
template <typename KV>
__global__ __launch_bounds__(256) void roll_prompt_refill_kernel(const int* __restrict__ list, const int* __restrict__ shared,
                                                                 const RollCall* __restrict__ call, KV* __restrict__ kv_all, size_t layer_stride,
                                                                 size_t kv_stride, int H, int T) {
    constexpr int PER = 16 / sizeof(KV);      // elements per lane
    constexpr int LANES = 64 / PER;           // lanes per slot of a head
    const int n = shared[ROLL_REFILLS];
    const int l = blockIdx.x >> 1, kv = blockIdx.x & 1;
    const int per_row = call->n, Cf = call->Cf, MP = call->MP;
    const int* plen = call->plen;
    const KV* ring = static_cast<const KV*>(call->pkv) + ((size_t)l * 2 + kv) * Cf * H * MP * 64;
    KV* plane = kv_all + (size_t)l * layer_stride + (size_t)kv * kv_stride;
    for (int k = blockIdx.y; k < n; k += gridDim.y) {
        const int r = list[2 * k], f = list[2 * k + 1] / per_row % Cf;
        const int per_head = (roll_prompt_len(plen[f], MP) - 1) * LANES;   // 16-byte pieces of one head
        for (int i = threadIdx.x; i < H * per_head; i += 256) {
            const int hd = i / per_head, j = i - hd * per_head;
            const KV* src = ring + (((size_t)f * H + hd) * MP + 1) * 64 + (size_t)j * PER;
            KV* dst = plane + (((size_t)r * H + hd) * T + 1) * 64 + (size_t)j * PER;
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        }
    }
}

// One thread per token of the M x T prompt rows of a teacher-forced pass: ptok rows (pitch MP) -> ids [M][T] int64
__global__ __launch_bounds__(256) void roll_prompt_ids_kernel(const int* __restrict__ ptok, int MP, int T, int M, long long* __restrict__ ids) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < M * T) ids[i] = ptok[(size_t)(i / T) * MP + (i % T)];
}

namespace {

// prompt: the call block holds prompt rings - roll_prompt_refill_kernel behind the refill
int launch_retire_refill(const RollRows& st, const int* arg, const RollCall* call, int R, void* kv, size_t layer_stride, size_t kv_stride,
                         int H, int T, int n_layer, KvFormat fmt, int f16, hipStream_t s, int handout_only = 0, bool prompt = false) {
    hipLaunchKernelGGL(roll_retire_kernel, dim3(1), dim3(256), 0, s, st, arg, call, R, handout_only);
    RGRG_LAUNCH_CHECK();
    const dim3 grid(n_layer * 2, std::min(R, ROLL_REFILL_ROWS));
    if (fmt == KV_F32)
        hipLaunchKernelGGL(roll_refill_kernel<float>, grid, dim3(256), 0, s, st.list, st.shared, call, static_cast<float*>(kv), layer_stride,
                           kv_stride, H, T, 0);
    else
        hipLaunchKernelGGL(roll_refill_kernel<unsigned short>, grid, dim3(256), 0, s, st.list, st.shared, call,
                           static_cast<unsigned short*>(kv), layer_stride, kv_stride, H, T, f16);
    RGRG_LAUNCH_CHECK();
    if (!prompt) return RGRG_OK;
    if (fmt == KV_F32)
        hipLaunchKernelGGL(roll_prompt_refill_kernel<float>, grid, dim3(256), 0, s, st.list, st.shared, call, static_cast<float*>(kv),
                           layer_stride, kv_stride, H, T);
    else
        hipLaunchKernelGGL(roll_prompt_refill_kernel<unsigned short>, grid, dim3(256), 0, s, st.list, st.shared, call,
                           static_cast<unsigned short*>(kv), layer_stride, kv_stride, H, T);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

RollRows roll_rows(const rgrg_decoder* d) {
    const rgrg_decoder::RollWork& w = d->roll;
    return RollRows{w.seq, w.len, w.tok, w.pos, w.step, w.list, w.shared};
}

}  // namespace

int roll_reserve(rgrg_decoder* d, int S) {
    rgrg_decoder::RollWork& w = d->roll;
    int rc;
    if (!w.seq) {
        const size_t R = d->rows;
        int** rows[] = {&w.seq, &w.len, &w.tok, &w.pos, &w.step, &w.arg};
        for (int** p : rows)
            if ((rc = dmalloc(d, (void**)p, R * sizeof(int), true))) return rc;
        if ((rc = dmalloc(d, (void**)&w.list, 2 * R * sizeof(int), true))) return rc;
        if ((rc = dmalloc(d, (void**)&w.shared, 4 * sizeof(int), true))) return rc;
        if ((rc = dmalloc(d, &w.call, sizeof(RollCall), true))) return rc;
    }
    if ((size_t)S > w.ukv_seqs) {
        RGRG_HIP(hipStreamSynchronize(d->stream));
        if (w.ukv) (void)hipFree(w.ukv);
        w.ukv = nullptr; w.ukv_seqs = 0;
        RGRG_HIP(hipMalloc((void**)&w.ukv, (size_t)S * d->ld_ukv * sizeof(float)));
        w.ukv_seqs = S;
    }
    return RGRG_OK;
}

// feature_space_transformation_nn and the uk / uv GEMM of all S feature rows (enqueue_prefill's, in passes of up to max_seqs rows
// through its work space; S <= max_seqs is one pass, the GEMM calls of rgrg_decoder_generate for S rows) -> roll.ukv
int enqueue_roll_prefill(rgrg_decoder* d, const float* feats, int S, size_t ukv_row0) {
    const int D = d->D;
    int rc;
    for (int s0 = 0; s0 < S; s0 += d->max_seqs) {
        const int M = std::min(d->max_seqs, S - s0);
        RGRG_HIP(hipMemcpyAsync(d->feats, feats + (size_t)s0 * D, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, d->stream));
        if ((rc = linear(d, d->fst0, d->feats, nullptr, d->h1, M, D, RGRG_ACT_RELU, false))) return rc;
        if ((rc = linear(d, d->fst2, d->h1, nullptr, d->img, M, D, RGRG_ACT_NONE, false))) return rc;
        if ((rc = linear(d, d->ukv, d->img, nullptr, d->roll.ukv + (ukv_row0 + s0) * d->ld_ukv, M, d->ld_ukv, RGRG_ACT_NONE, false))) return rc;
    }
    return RGRG_OK;
}

// roll_refill_kernel alone, for a scheduler that lives on the host (rolling beam search): the n (row, feature row) pairs of `pairs` -
// host memory that stays valid until the stream has passed this point - go to roll.list, n to the refill count.  The device block
// (roll.call) must hold the call's ukv / ld_ukv with n = 1.  n = 0 enqueues nothing.
int enqueue_roll_refill_list(rgrg_decoder* d, const int* pairs, int n, int R) {
    if (n <= 0) return RGRG_OK;
    hipStream_t st = d->stream;
    RGRG_HIP(hipMemcpyAsync(d->roll.list, pairs, 2 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    d->roll.host_refills = n;   // (outlives the call, like `pairs`)
    RGRG_HIP(hipMemcpyAsync(d->roll.shared + ROLL_REFILLS, &d->roll.host_refills, sizeof(int), hipMemcpyHostToDevice, st));
    const KvFormat fmt = (KvFormat)rgrg_decoder_kv_format_in_use(d, R);
    const dim3 grid(d->n_layer * 2, std::min(n, ROLL_REFILL_ROWS));
    const RollCall* call = static_cast<const RollCall*>(d->roll.call);
    if (fmt == KV_F32)
        hipLaunchKernelGGL(roll_refill_kernel<float>, grid, dim3(256), 0, st, d->roll.list, d->roll.shared, call, d->kv, d->kv_layer_stride,
                           d->kv_kv_stride, d->H, d->T, 0);
    else
        hipLaunchKernelGGL(roll_refill_kernel<unsigned short>, grid, dim3(256), 0, st, d->roll.list, d->roll.shared, call,
                           reinterpret_cast<unsigned short*>(d->kv), d->kv_layer_stride, d->kv_kv_stride, d->H, d->T, d->f16());
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

static int roll_retire_refill(rgrg_decoder* d, int R, int handout_only = 0, bool prompt = false) {
    const KvFormat fmt = (KvFormat)rgrg_decoder_kv_format_in_use(d, R);
    return launch_retire_refill(roll_rows(d), d->roll.arg, static_cast<const RollCall*>(d->roll.call), R, d->kv, d->kv_layer_stride,
                                d->kv_kv_stride, d->H, d->T, d->n_layer, fmt, d->f16(), d->stream, handout_only, prompt);
}

int enqueue_roll_end(rgrg_decoder* d, int R, int NT, bool prompt) {
    hipLaunchKernelGGL(roll_argmax_kernel, dim3(R), dim3(256), 0, d->stream, d->cand_val, d->cand_idx, NT, d->roll.arg);
    RGRG_LAUNCH_CHECK();
    return roll_retire_refill(d, R, 0, prompt);
}

int enqueue_roll_sample_end(rgrg_decoder* d, int R, bool prompt) {
    const int rc = launch_roll_sample(d->logits, (size_t)d->ld_logits, R, d->V, d->sample_prm, d->roll.seq, d->roll.len,
                                      static_cast<const RollCall*>(d->roll.call), d->roll.arg, d->stream);
    return rc ? rc : roll_retire_refill(d, R, 0, prompt);
}

namespace {

// What the two rolling entries share behind decode_begin: the S sequences - n per row of feats [S / n][1024] - through R rows with
// steps that end in `end` (STEP_ROLL, or STEP_ROLL_SAMPLE with the parameter block already enqueued).
int roll_run(rgrg_decoder* d, const char* who, const float* feats, int S, int n, int R, int max_length, StepEnd end, int64_t* ids_out,
             float* lp_out, int* lens_out, int* steps_out, int use_graph) {
    int rc;
    if ((rc = roll_reserve(d, S / n))) return rc;
    if ((rc = enqueue_roll_prefill(d, feats, S / n))) return rc;
    hipStream_t st = d->stream;
    const KvFormat fmt = (KvFormat)rgrg_decoder_kv_format_in_use(d, R);
    const RollRows rows = roll_rows(d);
    const RollCall call{reinterpret_cast<long long*>(ids_out), lens_out, d->roll.ukv, max_length, S, max_length, d->ld_ukv, lp_out, n, S, S / n};
    RollCall* dcall = static_cast<RollCall*>(d->roll.call);
    hipLaunchKernelGGL(roll_begin_kernel, dim3(64), dim3(256), 0, st, call, dcall, rows, R);
    RGRG_LAUNCH_CHECK();
    // every row is idle: the hand-out-only pass gives the first min(S, R) sequences to rows 0, 1, ... and fills their slot 0
    if ((rc = launch_retire_refill(rows, d->roll.arg, dcall, R, d->kv, d->kv_layer_stride, d->kv_kv_stride, d->H, d->T, d->n_layer, fmt,
                                   d->f16(), st, 1)))
        return rc;

    StepSpec step;
    step.rows = R; step.tok = d->roll.tok; step.row_pos = d->roll.pos; step.row_step = d->roll.step; step.end = end;
    hipGraphExec_t exec = nullptr;
    if (use_graph && (rc = step_graph(d, step, [&] { return enqueue_step(d, step, true); }, &exec))) return rc;
    // A sequence takes at most max_length - 1 steps and a free row never waits while a sequence is pending (list scheduling): all S
    // are done within ceil(S / R) (max_length - 1) steps of full rows plus one more sequence's worth.  The loop cannot run past that,
    // whatever the device words say.
    const long long bound = ((long long)(S + R - 1) / R + 1) * (max_length - 1);
    // "nothing unfinished" is polled like the greedy loop polls its length word (run_decode_loop): every 16 steps, waiting for the copy
    // queued 16 steps earlier; the up to 32 steps behind the last retirement run idle rows only
    int polls = 0;
    d->h_done[1] = d->h_done[2] = 1;
    for (long long t = 0; t < bound; ++t) {
        if (exec) RGRG_HIP(hipGraphLaunch(exec, st));
        else if ((rc = enqueue_step(d, step, t == 0))) return rc;
        if ((t & 15) == 15 && t + 1 < bound) {
            if (polls > 0) {
                const int prev = (polls - 1) & 1;
                RGRG_HIP(hipEventSynchronize(d->ev_poll[prev]));
                if (d->h_done[1 + prev] == 0) break;
            }
            const int cur = polls & 1;
            RGRG_HIP(hipMemcpyAsync(d->h_done + 1 + cur, d->roll.shared + ROLL_UNFINISHED, sizeof(int), hipMemcpyDeviceToHost, st));
            RGRG_HIP(hipEventRecord(d->ev_poll[cur], st));
            ++polls;
        }
    }
    RGRG_HIP(hipMemcpyAsync(d->h_done, d->roll.shared + ROLL_UNFINISHED, sizeof(int), hipMemcpyDeviceToHost, st));
    RGRG_HIP(hipMemcpyAsync(d->h_done + 1, d->roll.shared + ROLL_STEPS, sizeof(int), hipMemcpyDeviceToHost, st));
    RGRG_HIP(hipStreamSynchronize(st));
    d->logits_stale_rows = 0;   // (logits_valid stays false: the last step's rows are idle ones)
    if (d->h_done[0] != 0) {
        set_error("%s: %d of %d sequences unfinished after the bound of %lld steps on %d rows", who, d->h_done[0], S, bound, R);
        return RGRG_EHIP;
    }
    if (steps_out) *steps_out = d->h_done[1];
    return RGRG_OK;
}

}  // namespace

// the refusals the rolling entries share, each with a message
int roll_check(rgrg_decoder* d, const char* who, int R, int max_length) {
    if (R < 1 || R > d->max_seqs) {
        set_error("%s: %d decoder rows, the cache of this decoder holds 1 .. %d", who, R, d->max_seqs);
        return RGRG_EINVAL;
    }
    if (max_length < 2 || max_length > d->max_len) {
        set_error("%s: max_length %d, 2 .. %d (the cache) are possible", who, max_length, d->max_len);
        return RGRG_EINVAL;
    }
    if ((KvFormat)rgrg_decoder_kv_format_in_use(d, R) == KV_E4M3) {
        set_error("%s: the e4m3 K/V cache has no per-row step: call rgrg_decoder_set_kv_format(d, 0) first", who);
        return RGRG_EINVAL;
    }
    return RGRG_OK;
}

}  // namespace rgrg

using namespace rgrg;

extern "C" int rgrg_decoder_generate_rolling(rgrg_decoder* d, const float* feats, int S, int R, int max_length, int64_t* ids_out,
                                             int* lens_out, int* steps_out, int use_graph, void* stream) {
    RGRG_CHECK_ARG(d && feats && ids_out && lens_out && S > 0);
    int rc;
    if ((rc = roll_check(d, "rgrg_decoder_generate_rolling", R, max_length))) return rc;
    if ((rc = decode_begin(d, stream))) return rc;
    return roll_run(d, "rgrg_decoder_generate_rolling", feats, S, 1, R, max_length, STEP_ROLL, ids_out, nullptr, lens_out, steps_out,
                    use_graph);
}

extern "C" int rgrg_decoder_sample_rolling(rgrg_decoder* d, const float* feats, int S, int n, int R, int max_length, float temperature,
                                           int top_k, float top_p, uint64_t seed, int64_t* ids_out, float* logprobs_out, int* lens_out,
                                           int* steps_out, int use_graph, void* stream) {
    RGRG_CHECK_ARG(d && feats && ids_out && lens_out && S > 0 && n > 0 && (long long)S * n < 0x7fffffffLL / 1024);
    int rc;
    if ((rc = roll_check(d, "rgrg_decoder_sample_rolling", R, max_length))) return rc;
    if (!d->sample_prm && (rc = dmalloc(d, &d->sample_prm, sample_params_bytes(), true))) return rc;
    if ((rc = decode_begin(d, stream))) return rc;
    // the parameter block lives in device memory: the captured step serves every seed and parameter set
    if ((rc = enqueue_sample_params(d->sample_prm, temperature, top_k, top_p, seed, d->stream))) return rc;
    return roll_run(d, "rgrg_decoder_sample_rolling", feats, S * n, n, R, max_length, STEP_ROLL_SAMPLE, ids_out, logprobs_out, lens_out,
                    steps_out, use_graph);
}

// Test hook: ONE retire-and-refill step (roll_retire_kernel, roll_refill_kernel as the product launches them) on the caller's state.
// Device int32: row_seq / row_len / row_tok / row_pos / row_step / arg [R], shared [4] = {next pending, unfinished, refills, steps};
// ids int64 [S][ld_ids], lens [S].  ukv f32 [S][ld_ukv] and the cache kv [n_layer][2][R][H][T_slots][64] (fp32, or 16 bit with kv16 /
// fp16; layer_stride / kv_stride in elements) may be NULL together: no refill launch.  Synchronises `stream`.
extern "C" int rgrg_debug_roll_step(int* row_seq, int* row_len, int* row_tok, int* row_pos, int* row_step, int* shared, const int* arg,
                                    int64_t* ids, int ld_ids, int* lens, int S, int R, int max_length, const float* ukv, int ld_ukv,
                                    void* kv, size_t layer_stride, size_t kv_stride, int H, int T_slots, int n_layer, int kv16, int fp16,
                                    void* stream) {
    RGRG_CHECK_ARG(row_seq && row_len && row_tok && row_pos && row_step && shared && arg && ids && lens);
    RGRG_CHECK_ARG(S > 0 && R > 0 && R < 65536 && max_length >= 2 && ld_ids >= max_length);
    RGRG_CHECK_ARG((ukv == nullptr) == (kv == nullptr));
    RGRG_CHECK_ARG(!kv || (H > 0 && T_slots >= 2 && n_layer > 0 && ld_ukv >= n_layer * 2 * H * 64 && kv_stride >= (size_t)R * H * T_slots * 64 &&
                           layer_stride >= 2 * kv_stride));
    hipStream_t st = as_stream(stream);
    int* list = nullptr;
    RollCall* dcall = nullptr;
    RGRG_HIP(hipMalloc((void**)&list, 2 * (size_t)R * sizeof(int)));
    if (hipMalloc((void**)&dcall, sizeof(RollCall)) != hipSuccess) { (void)hipFree(list); set_error("rgrg_debug_roll_step: hipMalloc failed"); return RGRG_EHIP; }
    const RollCall call{reinterpret_cast<long long*>(ids), lens, ukv, ld_ids, S, max_length, ld_ukv, nullptr, 1, S, S};
    hipError_t e = hipMemcpyAsync(dcall, &call, sizeof(call), hipMemcpyHostToDevice, st);
    const RollRows rows{row_seq, row_len, row_tok, row_pos, row_step, list, shared};
    int rc = RGRG_OK;
    if (e == hipSuccess) {
        if (kv) rc = launch_retire_refill(rows, arg, dcall, R, kv, layer_stride, kv_stride, H, T_slots, n_layer,
                                          kv16 ? (fp16 ? KV_F16 : KV_BF16) : KV_F32, fp16 ? 1 : 0, st);
        else { hipLaunchKernelGGL(roll_retire_kernel, dim3(1), dim3(256), 0, st, rows, arg, dcall, R, 0); e = hipGetLastError(); }
    }
    const hipError_t es = hipStreamSynchronize(st);   // the list and the call block are the call's own: they must outlive the launches
    (void)hipFree(list);
    (void)hipFree(dcall);
    if (!rc && (e != hipSuccess || es != hipSuccess)) {
        set_error("rgrg_debug_roll_step: %s", hipGetErrorString(e != hipSuccess ? e : es));
        return RGRG_EHIP;
    }
    return rc;
}

// ---- The rolling session: the call above with an open list.  S grows by submits between steps, the output and the
// ukv rows live in rings the decoder owns, finished sequences are collected and released in order while others run.
namespace rgrg {

// A submit of `count` sequences q0 .. q0 + count - 1 (c: the host's block, S = q0 still): their ring rows in the state
// roll_begin_kernel gives a sequence that never ran - BOS then PAD (with prompt rings, c.plen: the P prompt tokens of its feature
// row's ring row, then PAD), log-probs 0, len 0 - and nothing else; then S and the unfinished word grow by count.  The kernels behind it in the stream see the new S.
// ring (or NULL: no request ring, or a test hook whose caller has written it): entry q % C of every new sequence becomes `req`.
__global__ __launch_bounds__(256) void roll_submit_kernel(const RollCall c, RollCall* __restrict__ call, int* __restrict__ shared, int q0,
                                                          int count, RollReq* __restrict__ ring, const RollReq req) {
    const size_t total = (size_t)count * c.max_length;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int q = q0 + (int)(i / c.max_length), col = (int)(i % c.max_length);
        const size_t o = (size_t)(q % c.C) * c.ld + col;
        long long tok = col == 0 ? BOS_ID : PAD_ID;
        if (c.plen) {
            const int f = q / c.n % c.Cf;
            if (col < roll_prompt_len(c.plen[f], c.MP)) tok = c.ptok[(size_t)f * c.MP + col];
        }
        c.ids[o] = tok;
        if (c.lp) c.lp[o] = 0.f;
    }
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < count; s += gridDim.x * blockDim.x) {
        c.len[(q0 + s) % c.C] = 0;
        if (ring) ring[(q0 + s) % c.C] = req;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        call->S = q0 + count;
        shared[ROLL_UNFINISHED] += count;
    }
}

static int launch_roll_submit(const RollCall& c, RollCall* dcall, int* shared, int q0, int count, hipStream_t st, RollReq* ring = nullptr,
                              const RollReq& req = RollReq{}) {
    const int blocks = (int)std::min<size_t>(64, ((size_t)count * c.max_length + 255) / 256);
    hipLaunchKernelGGL(roll_submit_kernel, dim3(std::max(blocks, 1)), dim3(256), 0, st, c, dcall, shared, q0, count, ring, req);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// rgrg_decoder_roll_cancel: the cancel flag of sequences first .. first + count - 1, outside the captured step.  The retire pass of the
// next step sees it (stream order); nothing else of the entry changes, so a sequence that has ended keeps its length word.
__global__ __launch_bounds__(256) void roll_cancel_kernel(RollReq* __restrict__ ring, int C, int first, int count) {
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < count; s += gridDim.x * blockDim.x) ring[(first + s) % C].flags |= ROLL_REQ_CANCEL;
}

void roll_session_free(rgrg_decoder* d) {
    rgrg_decoder::RollSession& s = d->sess;
    if (s.ids) (void)hipFree(s.ids);
    if (s.lp) (void)hipFree(s.lp);
    if (s.len) (void)hipFree(s.len);
    if (s.req) (void)hipFree(s.req);
    if (s.ptok) (void)hipFree(s.ptok);
    if (s.plen) (void)hipFree(s.plen);
    if (s.pkv) (void)hipFree(s.pkv);
    if (s.pids) (void)hipFree(s.pids);
    if (s.h_ptok) (void)hipHostFree(s.h_ptok);
    if (s.h_plen) (void)hipHostFree(s.h_plen);
    if (s.h_len) (void)hipHostFree(s.h_len);
    s = rgrg_decoder::RollSession{};
}

// the session every call but open and close needs: open, and no other decode entry has run on the decoder since
static int roll_session_live(rgrg_decoder* d, const char* who) {
    if (!d->sess.open) { set_error("%s: no rolling session is open on this decoder", who); return RGRG_EINVAL; }
    if (d->sess.epoch != d->epoch) {
        set_error("%s: the rolling session is stale: another decode call has used the decoder's cache rows since it was opened (close it and open a new one)", who);
        return RGRG_EINVAL;
    }
    return RGRG_OK;
}

}  // namespace rgrg

// The prompt rings of a session that is being opened (s.call is not set yet) and the work space of its prompt passes: everything a
// submit needs, so that a submit allocates nothing.  On failure the caller frees the session.
static int roll_prompt_reserve(rgrg_decoder* d, const char* who, int R, int Cf, int MP) {
    rgrg_decoder::RollSession& s = d->sess;
    const KvFormat fmt = (KvFormat)rgrg_decoder_kv_format_in_use(d, R);
    const size_t kv_bytes = (size_t)d->n_layer * 2 * Cf * d->H * MP * 64 * (fmt == KV_F32 ? 4 : 2);
    s.prompt_chunk = MP > 1 ? std::max(MP - 1, ROLL_PROMPT_CHUNK) : 0;
    if (hipMalloc(&s.pkv, kv_bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: no memory for the prompt K/V ring: %d feature rows x %d prompt slots x %d layers need %.1f MiB (a smaller capacity or "
                  "max_prompt_length fits)", who, Cf, MP, d->n_layer, (double)kv_bytes / (1024.0 * 1024.0));
        return RGRG_EHIP;
    }
    const size_t tok_bytes = (size_t)Cf * MP * sizeof(int);
    if (hipMalloc((void**)&s.ptok, tok_bytes) != hipSuccess || hipMalloc((void**)&s.plen, (size_t)Cf * sizeof(int)) != hipSuccess ||
        hipHostMalloc((void**)&s.h_ptok, tok_bytes) != hipSuccess || hipHostMalloc((void**)&s.h_plen, (size_t)Cf * sizeof(int)) != hipSuccess ||
        (s.prompt_chunk && hipMalloc((void**)&s.pids, (size_t)s.prompt_chunk * sizeof(long long)) != hipSuccess)) {
        (void)hipGetLastError();
        set_error("%s: no memory for the prompt token rings: %d feature rows x %d tokens need %.1f MiB on the device and as much pinned on the "
                  "host (the K/V ring of %.1f MiB is allocated)", who, Cf, MP, (double)tok_bytes / (1024.0 * 1024.0), (double)kv_bytes / (1024.0 * 1024.0));
        return RGRG_EHIP;
    }
    if (s.prompt_chunk && (tf_reserve(d, (size_t)s.prompt_chunk) || (d->bf16_gemms && tf_reserve_a16(d, (size_t)s.prompt_chunk)))) {
        (void)hipGetLastError();
        set_error("%s: no memory for the work space of a prompt pass over %d token rows (about %.0f MiB behind the K/V ring of %.1f MiB)", who,
                  s.prompt_chunk, (double)s.prompt_chunk * (14.0 * d->D + d->V) * 4.0 / (1024.0 * 1024.0), (double)kv_bytes / (1024.0 * 1024.0));
        return RGRG_EHIP;
    }
    return RGRG_OK;
}

extern "C" int rgrg_decoder_roll_open(rgrg_decoder* d, int R, int capacity, int n, int max_length, int sample, float temperature, int top_k,
                                      float top_p, uint64_t seed, int use_graph, void* stream) {
    return rgrg_decoder_roll_open_prompt(d, R, capacity, n, max_length, 0, sample, temperature, top_k, top_p, seed, use_graph, stream);
}

extern "C" int rgrg_decoder_roll_open_prompt(rgrg_decoder* d, int R, int capacity, int n, int max_length, int max_prompt_length, int sample,
                                             float temperature, int top_k, float top_p, uint64_t seed, int use_graph, void* stream) {
    RGRG_CHECK_ARG(d && n > 0);
    const char* who = max_prompt_length ? "rgrg_decoder_roll_open_prompt" : "rgrg_decoder_roll_open";
    if (d->sess.open) { set_error("%s: a rolling session is already open on this decoder (one per decoder: close it first)", who); return RGRG_EINVAL; }
    if (d->bsess.open) { set_error("%s: a rolling beam session is already open on this decoder (one per decoder: close it first)", who); return RGRG_EINVAL; }
    if (capacity < 1 || (long long)capacity * n >= 0x7fffffffLL / 1024) {
        set_error("%s: a ring of %d feature rows x %d sequences, 1 .. %lld sequences are possible", who, capacity, n, 0x7fffffffLL / 1024 - 1);
        return RGRG_EINVAL;
    }
    int rc;
    if ((rc = roll_check(d, who, R, max_length))) return rc;
    const int MP = max_prompt_length;
    if (MP < 0 || MP >= max_length) {
        set_error("%s: max_prompt_length %d, 0 (no prompts) .. %d are possible (max_length %d counts the prompt and one token is always generated)",
                  who, MP, max_length - 1, max_length);
        return RGRG_EINVAL;
    }
    if ((rc = roll_reserve(d, capacity))) return rc;
    if (sample && !d->sample_prm && (rc = dmalloc(d, &d->sample_prm, sample_params_bytes(), true))) return rc;
    rgrg_decoder::RollSession& s = d->sess;
    const size_t C = (size_t)capacity * n;
    if (hipMalloc((void**)&s.ids, C * max_length * sizeof(long long)) != hipSuccess || hipMalloc((void**)&s.len, C * sizeof(int)) != hipSuccess ||
        (sample && hipMalloc((void**)&s.lp, C * max_length * sizeof(float)) != hipSuccess) ||
        hipMalloc((void**)&s.req, C * sizeof(RollReq)) != hipSuccess || hipHostMalloc((void**)&s.h_len, C * sizeof(int)) != hipSuccess) {
        roll_session_free(d);
        set_error("%s: no memory for a ring of %zu sequences of %d tokens", who, C, max_length);
        return RGRG_EHIP;
    }
    std::fill(s.h_len, s.h_len + C, 0);
    if (MP > 0 && (rc = roll_prompt_reserve(d, who, R, capacity, MP))) {
        roll_session_free(d);
        return rc;
    }
    if ((rc = decode_begin(d, stream)) || (sample && (rc = enqueue_sample_params(d->sample_prm, temperature, top_k, top_p, seed, d->stream)))) {
        roll_session_free(d);
        return rc;
    }
    s.call = RollCall{s.ids, s.len, d->roll.ukv, max_length, 0, max_length, d->ld_ukv, s.lp, n, (int)C, capacity, s.req, s.ptok, s.plen, s.pkv, MP};
    // what a submit without a request asks for: the session's limit and parameters, its numbering (q0 = 0), EOS alone
    s.defaults = RollReq{seed, sample ? 1.0f / temperature : 1.0f, sample ? top_k : 0, sample ? top_p : 1.0f, max_length, 0,
                         {ROLL_NO_STOP, ROLL_NO_STOP, ROLL_NO_STOP, ROLL_NO_STOP}, 0u};
    s.R = R; s.use_graph = use_graph; s.end = sample ? STEP_ROLL_SAMPLE : STEP_ROLL;
    // the device block, every row idle, nothing pending (S = 0: roll_begin_kernel writes no output row)
    hipLaunchKernelGGL(roll_begin_kernel, dim3(1), dim3(256), 0, d->stream, s.call, static_cast<RollCall*>(d->roll.call), roll_rows(d), R);
    if (hipGetLastError() != hipSuccess) { roll_session_free(d); set_error("%s: the launch of roll_begin_kernel failed", who); return RGRG_EHIP; }
    s.epoch = d->epoch;
    s.open = true;
    return RGRG_OK;
}

// The prompt of feature rows f0 .. f0 + M - 1 of the ring (no wrap inside; token and ukv ring rows are written): rows 0 .. P - 2 in
// teacher-forced passes of up to prompt_chunk token rows, every layer's keys / values -> slots 1 .. P - 1 of the ring rows.  The
// pass reads the ukv ring rows as its image keys / values and writes the work space of tf_reserve and the K/V ring - nothing the
// captured step reads but the ring: not d->ukv_out, d->tf.pos, d->ids, d->step or the epoch.
struct RingStore { int f0, M, P; };
static int store_ring_kv(rgrg_decoder* d, int l, const float* qkv, const void* arg) {
    const RingStore& a = *static_cast<const RingStore*>(arg);
    const rgrg_decoder::RollSession& s = d->sess;
    const bool kv16 = (KvFormat)rgrg_decoder_kv_format_in_use(d, s.R) != KV_F32;
    const size_t plane = (size_t)s.call.Cf * d->H * s.call.MP * 64, row = (size_t)d->H * s.call.MP * 64, esz = kv16 ? 2 : 4;
    char* k = static_cast<char*>(s.pkv) + (((size_t)l * 2) * plane + (size_t)a.f0 * row) * esz;
    return launch_prompt_kv_store(qkv, k, k + plane * esz, a.M, d->H, a.P - 1, s.call.MP, 1, kv16, d->f16(), d->stream);
}
static int enqueue_roll_prompt_pass(rgrg_decoder* d, int f0, int M, int P) {
    rgrg_decoder::RollSession& s = d->sess;
    const int T = P - 1, per_pass = s.prompt_chunk / T;
    int rc;
    if ((rc = tf_reserve(d, (size_t)s.prompt_chunk))) return rc;   // (reserved at open: nothing happens unless the work space was dropped since)
    for (int m0 = 0; m0 < M; m0 += per_pass) {
        const RingStore a{f0 + m0, std::min(per_pass, M - m0), P};
        hipLaunchKernelGGL(roll_prompt_ids_kernel, dim3((a.M * T + 255) / 256), dim3(256), 0, d->stream, s.ptok + (size_t)a.f0 * s.call.MP,
                           s.call.MP, T, a.M, s.pids);
        RGRG_LAUNCH_CHECK();
        // kv_only: the pass ends behind the last layer's q | k | v, and in fp32 its result does not depend on the row count
        if ((rc = tf_hidden_pass(d, s.pids, nullptr, nullptr, 1, a.M, T, store_ring_kv, &a, d->roll.ukv + (size_t)a.f0 * d->ld_ukv, true)))
            return rc;
    }
    return RGRG_OK;
}

// submit with the request `req` for all m * n new sequences; q0 < 0 in it: the first new sequence (a request with a seed of its own).
// prompt (or NULL): HOST int64 [m][P], checked by the caller; a session with prompt rings gives a submit without one P = 1, BOS.
static int roll_submit(rgrg_decoder* d, const char* who, const float* feats, int m, RollReq req, long long* first_out, void* stream,
                       const int64_t* prompt = nullptr, int P = 1) {
    int rc;
    rgrg_decoder::RollSession& s = d->sess;
    const int n = s.call.n, C = s.call.C, Cf = s.call.Cf;
    const long long q0 = s.call.S, count = (long long)m * n;
    if (q0 + count >= 0x7fffffffLL / 1024) {
        set_error("%s: sequence numbers of a session stay below %lld (%lld submitted so far): open a new session", who, 0x7fffffffLL / 1024, q0);
        return RGRG_EINVAL;
    }
    if (q0 + count > s.watermark + C) {
        set_error("%s: %d feature rows (%lld sequences) do not fit the ring: capacity %d feature rows (%d sequences), room for %lld "
                  "feature rows until finished sequences are collected and released", who, m, count, Cf, C, (s.watermark + C - q0) / n);
        return RGRG_EINVAL;
    }
    RGRG_HIP(hipEventRecord(d->ev_in, as_stream(stream)));   // the feature rows are the caller's stream's
    RGRG_HIP(hipStreamWaitEvent(d->stream, d->ev_in, 0));
    // 1. the three GEMMs of the m rows into their ukv ring rows, split where the ring wraps
    const int f0 = (int)((q0 / n) % Cf), head = std::min(m, Cf - f0);
    if ((rc = enqueue_roll_prefill(d, feats, head, (size_t)f0))) return rc;
    if (m > head && (rc = enqueue_roll_prefill(d, feats + (size_t)head * d->D, m - head, 0))) return rc;
    // 1b. the prompts: token and length ring rows from their pinned sources (a ring row is free: its earlier sequences have been
    // released, so the copies that read it are done), then the prompt passes behind the ukv rows they attend to
    if (const int MP = s.call.MP) {
        for (int i = 0; i < m; ++i) {
            const int f = (f0 + i) % Cf;
            s.h_plen[f] = P;
            for (int j = 0; j < MP; ++j) s.h_ptok[(size_t)f * MP + j] = (prompt && j < P) ? (int)prompt[(size_t)i * P + j] : BOS_ID;
        }
        const int seg[2][2] = {{f0, head}, {0, m - head}};
        for (const auto& g : seg) {
            if (g[1] <= 0) continue;
            RGRG_HIP(hipMemcpyAsync(s.ptok + (size_t)g[0] * MP, s.h_ptok + (size_t)g[0] * MP, (size_t)g[1] * MP * sizeof(int), hipMemcpyHostToDevice, d->stream));
            RGRG_HIP(hipMemcpyAsync(s.plen + g[0], s.h_plen + g[0], (size_t)g[1] * sizeof(int), hipMemcpyHostToDevice, d->stream));
            if (P > 1 && (rc = enqueue_roll_prompt_pass(d, g[0], g[1], P))) return rc;
        }
    }
    // 2. + 3. the new output rows, S and the unfinished word; 4. idle rows take what is pending, their slot 0 is filled
    if (req.q0 < 0) req.q0 = (int)q0;
    if ((rc = launch_roll_submit(s.call, static_cast<RollCall*>(d->roll.call), d->roll.shared, (int)q0, (int)count, d->stream, s.req, req)))
        return rc;
    for (long long q = q0; q < q0 + count; ++q) s.h_len[q % C] = 0;
    s.call.S = (int)(q0 + count);
    s.unfinished += count;
    s.drained = false;
    if ((rc = roll_retire_refill(d, s.R, 1, s.call.MP > 0))) return rc;
    if (first_out) *first_out = q0;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_roll_submit(rgrg_decoder* d, const float* feats, int m, long long* first_out, void* stream) {
    RGRG_CHECK_ARG(d && feats && m > 0);
    const char* who = "rgrg_decoder_roll_submit";
    int rc;
    if ((rc = roll_session_live(d, who))) return rc;
    return roll_submit(d, who, feats, m, d->sess.defaults, first_out, stream);
}

// the request of rgrg_decoder_roll_submit_req / _submit_prompt -> *out, or the refusal (0 / -1 / NULL arguments: the session's values)
static int roll_parse_req(rgrg_decoder* d, const char* who, int max_length, float temperature, int top_k, float top_p, int has_seed,
                          uint64_t seed, const int* stop_ids, int n_stop, RollReq* out) {
    const rgrg_decoder::RollSession& s = d->sess;
    RollReq req = s.defaults;
    if (max_length != 0) {
        if (max_length < 2 || max_length > s.call.max_length) {
            set_error("%s: max_length %d, 2 .. %d (the session's) are possible", who, max_length, s.call.max_length);
            return RGRG_EINVAL;
        }
        req.max_length = max_length;
    }
    const bool sampling = temperature != 0.f || top_k >= 0 || top_p != 0.f || has_seed;
    if (sampling && s.end != STEP_ROLL_SAMPLE) {
        set_error("%s: temperature, top_k, top_p and seed belong to a sampling session, this one is a greedy session", who);
        return RGRG_EINVAL;
    }
    if (temperature != 0.f) {
        if (!(temperature > 0.f)) { set_error("%s: temperature %g has to be positive", who, (double)temperature); return RGRG_EINVAL; }
        req.inv_T = 1.0f / temperature;
    }
    if (top_k >= 0) req.top_k = top_k;
    if (top_p != 0.f) {
        if (!(top_p > 0.f && top_p <= 1.0f)) { set_error("%s: top_p %g, (0, 1] is possible", who, (double)top_p); return RGRG_EINVAL; }
        req.top_p = top_p;
    }
    if (has_seed) { req.seed = seed; req.q0 = -1; }   // (roll_submit: the submit's first sequence)
    if (n_stop < 0 || n_stop > ROLL_MAX_STOPS) {
        set_error("%s: %d stop token ids, 0 .. %d are possible", who, n_stop, ROLL_MAX_STOPS);
        return RGRG_EINVAL;
    }
    for (int i = 0; i < n_stop; ++i) {
        if (stop_ids[i] < 0 || stop_ids[i] >= (int)ROLL_NO_STOP) {
            set_error("%s: stop token id %d, 0 .. %d are possible", who, stop_ids[i], (int)ROLL_NO_STOP - 1);
            return RGRG_EINVAL;
        }
        req.stop[i] = (unsigned short)stop_ids[i];
    }
    *out = req;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_roll_submit_req(rgrg_decoder* d, const float* feats, int m, int max_length, float temperature, int top_k,
                                            float top_p, int has_seed, uint64_t seed, const int* stop_ids, int n_stop,
                                            long long* first_out, void* stream) {
    RGRG_CHECK_ARG(d && feats && m > 0 && (n_stop == 0 || stop_ids));
    const char* who = "rgrg_decoder_roll_submit_req";
    int rc;
    if ((rc = roll_session_live(d, who))) return rc;
    RollReq req;
    if ((rc = roll_parse_req(d, who, max_length, temperature, top_k, top_p, has_seed, seed, stop_ids, n_stop, &req))) return rc;
    return roll_submit(d, who, feats, m, req, first_out, stream);
}

extern "C" int rgrg_decoder_roll_submit_prompt(rgrg_decoder* d, const float* feats, int m, const int64_t* prompt_ids, int P, int max_length,
                                               float temperature, int top_k, float top_p, int has_seed, uint64_t seed, const int* stop_ids,
                                               int n_stop, long long* first_out, void* stream) {
    RGRG_CHECK_ARG(d && feats && m > 0 && prompt_ids && (n_stop == 0 || stop_ids));
    const char* who = "rgrg_decoder_roll_submit_prompt";
    int rc;
    if (d->bsess.open) { set_error("%s: a rolling beam session takes no prompts (its scheduler lives on the host)", who); return RGRG_EINVAL; }
    if ((rc = roll_session_live(d, who))) return rc;
    const rgrg_decoder::RollSession& s = d->sess;
    if (s.call.MP == 0) {
        set_error("%s: the session was opened without max_prompt_length: it holds no prompt rings", who);
        return RGRG_EINVAL;
    }
    RollReq req;
    if ((rc = roll_parse_req(d, who, max_length, temperature, top_k, top_p, has_seed, seed, stop_ids, n_stop, &req))) return rc;
    if (P < 1 || P > s.call.MP || P + 1 > req.max_length) {
        set_error("%s: a prompt of %d tokens, 1 .. %d are possible (max_prompt_length %d; max_length %d counts the prompt and one token is "
                  "always generated)", who, P, std::min(s.call.MP, req.max_length - 1), s.call.MP, req.max_length);
        return RGRG_EINVAL;
    }
    for (size_t i = 0; i < (size_t)m * P; ++i)
        if (prompt_ids[i] < 0 || prompt_ids[i] >= d->V) {
            set_error("%s: prompt token id %lld (row %zu, column %zu), 0 .. %d are possible", who, (long long)prompt_ids[i], i / P, i % P, d->V - 1);
            return RGRG_EINVAL;
        }
    return roll_submit(d, who, feats, m, req, first_out, stream, prompt_ids, P);
}

extern "C" int rgrg_decoder_roll_cancel(rgrg_decoder* d, long long first, int count) {
    RGRG_CHECK_ARG(d && count > 0);
    const char* who = "rgrg_decoder_roll_cancel";
    int rc;
    if ((rc = roll_session_live(d, who))) return rc;
    const rgrg_decoder::RollSession& s = d->sess;
    if (first < s.watermark || first + count > s.call.S) {
        set_error("%s: sequences %lld .. %lld, the ring holds %lld .. %d", who, first, first + count - 1, s.watermark, s.call.S - 1);
        return RGRG_EINVAL;
    }
    hipLaunchKernelGGL(roll_cancel_kernel, dim3((count + 255) / 256), dim3(256), 0, d->stream, s.req, s.call.C, (int)first, count);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

extern "C" int rgrg_decoder_roll_advance(rgrg_decoder* d, int max_steps, int* launched_out, int* unfinished_out, int* steps_out) {
    RGRG_CHECK_ARG(d);
    const char* who = "rgrg_decoder_roll_advance";
    int rc;
    if ((rc = roll_session_live(d, who))) return rc;
    rgrg_decoder::RollSession& s = d->sess;
    hipStream_t st = d->stream;
    const int R = s.R, L = s.call.max_length;
    // until drained (max_steps < 0): the bound of roll_run over what is unfinished now
    const long long bound = ((s.unfinished + R - 1) / R + 1) * (L - 1);
    const long long limit = max_steps < 0 ? bound : max_steps;
    long long launched = 0;
    if (!s.drained && limit > 0) {
        StepSpec step;
        step.rows = R; step.tok = d->roll.tok; step.row_pos = d->roll.pos; step.row_step = d->roll.step; step.end = s.end;
        step.roll_prompt = s.call.MP > 0;
        hipGraphExec_t exec = nullptr;
        if (s.use_graph && (rc = step_graph(d, step, [&] { return enqueue_step(d, step, true); }, &exec))) return rc;
        // polled as roll_run polls: every 16 steps, waiting for the copy queued 16 steps earlier
        int polls = 0;
        d->h_done[1] = d->h_done[2] = 1;
        for (long long t = 0; t < limit; ++t) {
            if (exec) RGRG_HIP(hipGraphLaunch(exec, st));
            else if ((rc = enqueue_step(d, step, !s.counted))) return rc;
            s.counted = true;
            ++launched;
            if ((t & 15) == 15 && t + 1 < limit) {
                if (polls > 0) {
                    const int prev = (polls - 1) & 1;
                    RGRG_HIP(hipEventSynchronize(d->ev_poll[prev]));
                    if (d->h_done[1 + prev] == 0) break;
                }
                const int cur = polls & 1;
                RGRG_HIP(hipMemcpyAsync(d->h_done + 1 + cur, d->roll.shared + ROLL_UNFINISHED, sizeof(int), hipMemcpyDeviceToHost, st));
                RGRG_HIP(hipEventRecord(d->ev_poll[cur], st));
                ++polls;
            }
        }
    }
    // (also when nothing was launched: a submit's hand-out pass may be queued, and the caller gets the device's counts)
    if (launched > 0 || !s.drained) {
        RGRG_HIP(hipMemcpyAsync(d->h_done, d->roll.shared + ROLL_UNFINISHED, sizeof(int), hipMemcpyDeviceToHost, st));
        RGRG_HIP(hipMemcpyAsync(d->h_done + 1, d->roll.shared + ROLL_STEPS, sizeof(int), hipMemcpyDeviceToHost, st));
        RGRG_HIP(hipMemcpyAsync(s.h_len, s.len, (size_t)s.call.C * sizeof(int), hipMemcpyDeviceToHost, st));
        RGRG_HIP(hipStreamSynchronize(st));
        d->logits_stale_rows = 0;
        s.unfinished = d->h_done[0];
        s.drained = s.unfinished == 0;
        s.steps = d->h_done[1];
    }
    if (launched_out) *launched_out = (int)launched;
    if (unfinished_out) *unfinished_out = (int)s.unfinished;
    if (steps_out) *steps_out = s.steps;
    if (max_steps < 0 && s.unfinished != 0) {
        set_error("%s: %lld sequences unfinished after the bound of %lld steps on %d rows", who, s.unfinished, bound, R);
        return RGRG_EHIP;
    }
    return RGRG_OK;
}

extern "C" int rgrg_decoder_roll_collect(rgrg_decoder* d, long long first, int count, int64_t* ids_out, float* logprobs_out, int* lens_out,
                                         void* stream) {
    RGRG_CHECK_ARG(d && count > 0 && lens_out);
    const char* who = "rgrg_decoder_roll_collect";
    int rc;
    if ((rc = roll_session_live(d, who))) return rc;
    rgrg_decoder::RollSession& s = d->sess;
    const int C = s.call.C, L = s.call.max_length;
    if (first < s.watermark || first + count > s.call.S) {
        set_error("%s: sequences %lld .. %lld, the ring holds %lld .. %d", who, first, first + count - 1, s.watermark, s.call.S - 1);
        return RGRG_EINVAL;
    }
    if (logprobs_out && !s.lp) { set_error("%s: a greedy session keeps no log-probs", who); return RGRG_EINVAL; }
    for (int i = 0; i < count; ++i) lens_out[i] = s.h_len[(first + i) % C];
    if (ids_out) {
        hipStream_t st = d->stream;
        for (int i = 0; i < count;) {   // whole runs of ring rows
            const int slot = (int)((first + i) % C), run = std::min(count - i, C - slot);
            RGRG_HIP(hipMemcpyAsync(ids_out + (size_t)i * L, s.ids + (size_t)slot * L, (size_t)run * L * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
            if (logprobs_out)
                RGRG_HIP(hipMemcpyAsync(logprobs_out + (size_t)i * L, s.lp + (size_t)slot * L, (size_t)run * L * sizeof(float), hipMemcpyDeviceToDevice, st));
            i += run;
        }
        RGRG_HIP(hipStreamSynchronize(st));
    }
    (void)stream;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_roll_release(rgrg_decoder* d, long long watermark) {
    RGRG_CHECK_ARG(d);
    const char* who = "rgrg_decoder_roll_release";
    int rc;
    if ((rc = roll_session_live(d, who))) return rc;
    rgrg_decoder::RollSession& s = d->sess;
    if (watermark < s.watermark || watermark > s.call.S) {
        set_error("%s: watermark %lld, %lld .. %d are possible", who, watermark, s.watermark, s.call.S);
        return RGRG_EINVAL;
    }
    for (long long q = s.watermark; q < watermark; ++q)
        if (s.h_len[q % s.call.C] == 0) {
            set_error("%s: sequence %lld below the new watermark %lld has not finished", who, q, watermark);
            return RGRG_EINVAL;
        }
    s.watermark = watermark;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_roll_close(rgrg_decoder* d) {
    RGRG_CHECK_ARG(d);
    if (!d->sess.open) return RGRG_OK;
    const hipError_t e = hipStreamSynchronize(d->stream);   // queued steps read the rings
    roll_session_free(d);
    if (e != hipSuccess) { set_error("rgrg_decoder_roll_close: %s", hipGetErrorString(e)); return RGRG_EHIP; }
    return RGRG_OK;
}

// Test hook: what a session enqueues around one step, on the caller's state with a ring - submit-init of `submit` new sequences
// (S_before .. S_before + submit - 1; 0: none), the hand-out-only pass (handout), a whole retire pass (retire), each pass with its
// refill launch when ukv / kv are given.  Arrays as rgrg_debug_roll_step, but ids / lp [C][ld_ids], lens [C], ukv [C / n][ld_ukv].
static int debug_roll_session_step(const char* who, int* row_seq, int* row_len, int* row_tok, int* row_pos, int* row_step, int* shared,
                                   const int* arg, int64_t* ids, float* lp, int ld_ids, int* lens, int C, int n, int S_before,
                                   int submit, int handout, int retire, int R, int max_length, const float* ukv, int ld_ukv,
                                   void* kv, size_t layer_stride, size_t kv_stride, int H, int T_slots, int n_layer, int kv16,
                                   int fp16, const RollReq* req, void* stream, const int* ptok = nullptr, const int* plen = nullptr,
                                   const void* pkv = nullptr, int MP = 0) {
    RGRG_CHECK_ARG(row_seq && row_len && row_tok && row_pos && row_step && shared && arg && ids && lens);
    RGRG_CHECK_ARG(C > 0 && n > 0 && C % n == 0 && S_before >= 0 && submit >= 0 && submit % n == 0 && submit <= C &&
                   (long long)S_before + submit < 0x7fffffffLL / 1024);
    RGRG_CHECK_ARG(R > 0 && R < 65536 && max_length >= 2 && ld_ids >= max_length);
    RGRG_CHECK_ARG((ukv == nullptr) == (kv == nullptr));
    RGRG_CHECK_ARG(!kv || (H > 0 && T_slots >= 2 && n_layer > 0 && ld_ukv >= n_layer * 2 * H * 64 && kv_stride >= (size_t)R * H * T_slots * 64 &&
                           layer_stride >= 2 * kv_stride));
    hipStream_t st = as_stream(stream);
    int* list = nullptr;
    RollCall* dcall = nullptr;
    RGRG_HIP(hipMalloc((void**)&list, 2 * (size_t)R * sizeof(int)));
    if (hipMalloc((void**)&dcall, sizeof(RollCall)) != hipSuccess) { (void)hipFree(list); set_error("%s: hipMalloc failed", who); return RGRG_EHIP; }
    const RollCall call{reinterpret_cast<long long*>(ids), lens, ukv, ld_ids, S_before, max_length, ld_ukv, lp, n, C, C / n, req, ptok, plen, pkv, MP};
    hipError_t e = hipMemcpyAsync(dcall, &call, sizeof(call), hipMemcpyHostToDevice, st);
    const RollRows rows{row_seq, row_len, row_tok, row_pos, row_step, list, shared};
    const KvFormat fmt = kv16 ? (fp16 ? KV_F16 : KV_BF16) : KV_F32;
    int rc = RGRG_OK;
    auto pass = [&](int handout_only) {
        if (kv) return launch_retire_refill(rows, arg, dcall, R, kv, layer_stride, kv_stride, H, T_slots, n_layer, fmt, fp16 ? 1 : 0, st, handout_only,
                                            MP > 0);
        hipLaunchKernelGGL(roll_retire_kernel, dim3(1), dim3(256), 0, st, rows, arg, dcall, R, handout_only);
        RGRG_LAUNCH_CHECK();
        return (int)RGRG_OK;
    };
    if (e == hipSuccess) {
        if (submit > 0) rc = launch_roll_submit(call, dcall, shared, S_before, submit, st);
        if (!rc && handout) rc = pass(1);
        if (!rc && retire) rc = pass(0);
    }
    const hipError_t es = hipStreamSynchronize(st);   // the list and the call block are the call's own: they must outlive the launches
    (void)hipFree(list);
    (void)hipFree(dcall);
    if (!rc && (e != hipSuccess || es != hipSuccess)) {
        set_error("%s: %s", who, hipGetErrorString(e != hipSuccess ? e : es));
        return RGRG_EHIP;
    }
    return rc;
}

extern "C" int rgrg_debug_roll_session_step(int* row_seq, int* row_len, int* row_tok, int* row_pos, int* row_step, int* shared,
                                            const int* arg, int64_t* ids, float* lp, int ld_ids, int* lens, int C, int n, int S_before,
                                            int submit, int handout, int retire, int R, int max_length, const float* ukv, int ld_ukv,
                                            void* kv, size_t layer_stride, size_t kv_stride, int H, int T_slots, int n_layer, int kv16,
                                            int fp16, void* stream) {
    return debug_roll_session_step("rgrg_debug_roll_session_step", row_seq, row_len, row_tok, row_pos, row_step, shared, arg, ids, lp, ld_ids,
                                   lens, C, n, S_before, submit, handout, retire, R, max_length, ukv, ld_ukv, kv, layer_stride, kv_stride, H,
                                   T_slots, n_layer, kv16, fp16, nullptr, stream);
}

// The request ring `req` [C] of a test hook, read back and checked on the host before any kernel trusts it: limits 2 .. max_length
// (0: not checked - the sampler hook), parameters the sampler accepts, stop ids below 65535 or unused.  Synchronises `st`.
static int debug_check_req_ring(const char* who, const void* req, int C, int max_length, hipStream_t st) {
    std::vector<RollReq> h((size_t)C);
    RGRG_HIP(hipMemcpyAsync(h.data(), req, (size_t)C * sizeof(RollReq), hipMemcpyDeviceToHost, st));
    RGRG_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < C; ++i) {
        const RollReq& q = h[(size_t)i];
        const bool ok = (max_length == 0 || (q.max_length >= 2 && q.max_length <= max_length)) && q.inv_T > 0.f && q.top_k >= 0 &&
                        q.top_p > 0.f && q.top_p <= 1.0f && q.q0 >= 0;
        if (!ok) {
            set_error("%s: request ring entry %d: max_length %d (2 .. %d), 1 / temperature %g (> 0), top_k %d (>= 0), top_p %g ((0, 1]), q0 %d (>= 0)",
                      who, i, q.max_length, max_length, (double)q.inv_T, q.top_k, (double)q.top_p, q.q0);
            return RGRG_EINVAL;
        }
    }
    return RGRG_OK;
}

// Test hook: rgrg_debug_roll_session_step with the caller's request ring `req` [C] (40-byte entries, include/rgrg_hip.h "Request ring";
// NULL: the hook above).  The submit-init does not write the ring: the caller has written the entries of the new sequences.
extern "C" int rgrg_debug_roll_session_step_req(int* row_seq, int* row_len, int* row_tok, int* row_pos, int* row_step, int* shared,
                                                const int* arg, int64_t* ids, float* lp, int ld_ids, int* lens, int C, int n,
                                                int S_before, int submit, int handout, int retire, int R, int max_length,
                                                const float* ukv, int ld_ukv, void* kv, size_t layer_stride, size_t kv_stride, int H,
                                                int T_slots, int n_layer, int kv16, int fp16, const void* req, void* stream) {
    const char* who = "rgrg_debug_roll_session_step_req";
    RGRG_CHECK_ARG(C > 0 && max_length >= 2);
    int rc;
    if (req && (rc = debug_check_req_ring(who, req, C, max_length, as_stream(stream)))) return rc;
    return debug_roll_session_step(who, row_seq, row_len, row_tok, row_pos, row_step, shared, arg, ids, lp, ld_ids, lens, C, n, S_before,
                                   submit, handout, retire, R, max_length, ukv, ld_ukv, kv, layer_stride, kv_stride, H, T_slots, n_layer,
                                   kv16, fp16, static_cast<const RollReq*>(req), stream);
}

// Test hook: the rolling sampler (roll_sample_kernel as a STEP_ROLL_SAMPLE step launches it) on the caller's state.  Device: logits f32
// [R][ld], row_seq / row_len / arg int32 [R], lp f32 [largest sequence + 1][ld_lp] or NULL.  Synchronises `stream`.
static int debug_roll_sample(const char* who, const float* logits, int64_t ld, int V, int R, const int* row_seq, const int* row_len,
                             float temperature, int top_k, float top_p, uint64_t seed, const RollReq* req, int C, int* arg, float* lp,
                             int ld_lp, void* stream) {
    RGRG_CHECK_ARG(logits && row_seq && row_len && arg && R > 0 && R < 65536 && V > 0 && ld >= V && (!lp || ld_lp >= 2));
    hipStream_t st = as_stream(stream);
    void* prm = nullptr;
    RollCall* dcall = nullptr;
    RGRG_HIP(hipMalloc(&prm, sample_params_bytes()));
    if (hipMalloc((void**)&dcall, sizeof(RollCall)) != hipSuccess) { (void)hipFree(prm); set_error("%s: hipMalloc failed", who); return RGRG_EHIP; }
    const RollCall call{nullptr, nullptr, nullptr, ld_lp, 0, 0, 0, lp, 1, C, C, req};   // C = 0x7fffffff: no ring, the row is the sequence
    int rc = enqueue_sample_params(prm, temperature, top_k, top_p, seed, st);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(dcall, &call, sizeof(call), hipMemcpyHostToDevice, st);
    if (!rc && e == hipSuccess) rc = launch_roll_sample(logits, (size_t)ld, R, V, prm, row_seq, row_len, dcall, arg, st);
    const hipError_t es = hipStreamSynchronize(st);   // the two blocks are the call's own: they must outlive the launches
    (void)hipFree(prm);
    (void)hipFree(dcall);
    if (!rc && (e != hipSuccess || es != hipSuccess)) {
        set_error("%s: %s", who, hipGetErrorString(e != hipSuccess ? e : es));
        return RGRG_EHIP;
    }
    return rc;
}

extern "C" int rgrg_debug_roll_sample(const float* logits, int64_t ld, int V, int R, const int* row_seq, const int* row_len,
                                      float temperature, int top_k, float top_p, uint64_t seed, int* arg, float* lp, int ld_lp,
                                      void* stream) {
    return debug_roll_sample("rgrg_debug_roll_sample", logits, ld, V, R, row_seq, row_len, temperature, top_k, top_p, seed, nullptr,
                             0x7fffffff, arg, lp, ld_lp, stream);
}

// Test hook: rgrg_debug_roll_sample with the caller's request ring `req` [C]: an active row draws with the parameters of entry
// row_seq[r] % C under the counter (row_seq[r] - q0, row_len[r] - 1) and its log-prob goes to lp[(row_seq[r] % C) * ld_lp + row_len[r]].
// (temperature, top_k, top_p, seed) fill the parameter block of the step, which the kernel must NOT read then.  req NULL: the hook
// above (C is not used).
extern "C" int rgrg_debug_roll_sample_req(const float* logits, int64_t ld, int V, int R, const int* row_seq, const int* row_len,
                                          float temperature, int top_k, float top_p, uint64_t seed, const void* req, int C, int* arg,
                                          float* lp, int ld_lp, void* stream) {
    const char* who = "rgrg_debug_roll_sample_req";
    if (!req) return debug_roll_sample(who, logits, ld, V, R, row_seq, row_len, temperature, top_k, top_p, seed, nullptr, 0x7fffffff, arg, lp,
                                       ld_lp, stream);
    RGRG_CHECK_ARG(C > 0);
    int rc;
    if ((rc = debug_check_req_ring(who, req, C, 0, as_stream(stream)))) return rc;
    return debug_roll_sample(who, logits, ld, V, R, row_seq, row_len, temperature, top_k, top_p, seed, static_cast<const RollReq*>(req), C,
                             arg, lp, ld_lp, stream);
}

// Test hook: rgrg_debug_roll_session_step_req with prompt rings: ptok int32 [C / n][MP], plen int32 [C / n] - read back
// and checked on the host before any kernel trusts them: 1 .. MP, below max_length, and tokens 0 .. 65535 -, pkv the K/V ring
// [n_layer][2][C / n][H][MP][64] in the cache's element format (NULL together with kv).  The submit-init writes the prompts into the id
// ring, a seating pass gives len = P, tok = prompt[P - 1], pos = step = P - 1 and copies ring slots 1 .. P - 1 behind slot 0.
extern "C" int rgrg_debug_roll_prompt_step(int* row_seq, int* row_len, int* row_tok, int* row_pos, int* row_step, int* shared, const int* arg,
                                           int64_t* ids, float* lp, int ld_ids, int* lens, int C, int n, int S_before, int submit,
                                           int handout, int retire, int R, int max_length, const float* ukv, int ld_ukv, void* kv,
                                           size_t layer_stride, size_t kv_stride, int H, int T_slots, int n_layer, int kv16, int fp16,
                                           const void* req, const int* ptok, const int* plen, const void* pkv, int MP, void* stream) {
    const char* who = "rgrg_debug_roll_prompt_step";
    RGRG_CHECK_ARG(C > 0 && n > 0 && C % n == 0 && max_length >= 2 && ptok && plen && MP >= 1 && MP < max_length);
    RGRG_CHECK_ARG((pkv == nullptr) == (kv == nullptr) && (!kv || MP + 1 <= T_slots));
    int rc;
    hipStream_t st = as_stream(stream);
    if (req && (rc = debug_check_req_ring(who, req, C, max_length, st))) return rc;
    const int Cf = C / n;
    std::vector<int> h((size_t)Cf * (MP + 1));
    RGRG_HIP(hipMemcpyAsync(h.data(), plen, (size_t)Cf * sizeof(int), hipMemcpyDeviceToHost, st));
    RGRG_HIP(hipMemcpyAsync(h.data() + Cf, ptok, (size_t)Cf * MP * sizeof(int), hipMemcpyDeviceToHost, st));
    RGRG_HIP(hipStreamSynchronize(st));
    for (int f = 0; f < Cf; ++f) {
        bool ok = h[(size_t)f] >= 1 && h[(size_t)f] <= MP;
        for (int j = 0; ok && j < h[(size_t)f]; ++j) ok = h[(size_t)Cf + (size_t)f * MP + j] >= 0 && h[(size_t)Cf + (size_t)f * MP + j] < 65536;
        if (!ok) { set_error("%s: prompt ring row %d: a length of %d tokens (1 .. %d), or a token outside 0 .. 65535", who, f, h[(size_t)f], MP); return RGRG_EINVAL; }
    }
    return debug_roll_session_step(who, row_seq, row_len, row_tok, row_pos, row_step, shared, arg, ids, lp, ld_ids, lens, C, n, S_before,
                                   submit, handout, retire, R, max_length, ukv, ld_ukv, kv, layer_stride, kv_stride, H, T_slots, n_layer,
                                   kv16, fp16, static_cast<const RollReq*>(req), stream, ptok, plen, pkv, MP);
}
