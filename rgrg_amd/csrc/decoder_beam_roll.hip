// Rolling-batch beam search (rgrg_decoder_beam_search_rolling): G = R / num_beams region SLOTS of num_beams consecutive
// decoder rows through which any number of regions flow.  A region whose scorer is done - or whose hypotheses have reached max_length
// tokens - is finalized and leaves; its slot takes the next pending region in the same step.  The work follows the sum of the regions'
// iterations instead of regions x the slowest one, and the K/V cache is sized by R.
//
// The BeamSearchScorer lives on the host (decoder_beam.hip: beam_process_group / beam_finalize_item / beam_write_best, the ONE
// restatement both loops call) and the host synchronises once per step, as in lock step: it knows, per slot, the moment its region is
// done and writes what the next step needs - per row a token, a beam score and a TURN: the parent row, or a code for a fresh or an idle
// row - plus the (row, region) list of the slots that take a new region.  Per step:
//   beam_roll_turn_kernel   one launch for what beam_advance_kernel + beam_step_inc_kernel + beam_init_kernel do in lock step: the new
//                           ancestor table (ping-pong: reads and writes never alias) and the PER-ROW step, which is also the row's
//                           embedding position (StepSpec::row_pos == row_step)
//   roll_refill_kernel      decoder_roll.hip's: the image key / value of every region seated -> slot 0 of its slot's first row
//   the step                enqueue_step with tok, src, row_pos, row_step, STEP_BEAM: the attention reads the ancestor table AND the
//                           row's own step (attn_decode_kernel<true, .., true>, attn_decode_kv16_wave_kernel<true, .., true>)
//   the ranking             launch_beam_row_topk / launch_beam_merge over the G slots: they do not read the step
// Which slot decodes which region is a function of the tokens alone (free slots take the pending regions in ascending slot order), so a
// second call returns the same bits.
//
// The rolling beam SESSION (rgrg_decoder_beam_roll_*) is the same loop body - beam_roll_begin / beam_roll_seat /
// beam_roll_step below - with a state that outlives a call: regions arrive by submits between steps, their image key / value rows
// live in a ring of `capacity` rows, and a slot is seated only in front of a step that is launched.
#include <algorithm>
#include <vector>

#include "decoder_internal.h"

namespace rgrg {

constexpr int TURN_FRESH = -1, TURN_IDLE = -2;   // parent codes of beam_roll_turn_kernel (include/rgrg_hip.h rgrg_debug_beam_roll_turn)

// Every cell of both ancestor tables of rows 0 .. R - 1 -> the first row of the row's slot: cell 0 (the image key / value lives there)
// keeps that value for the whole call, and a cell that no region has written yet still names a row of the slot - the attention requests
// cell t + 1 of a row before it substitutes the new key.  Every row idle at step 0.
__global__ __launch_bounds__(256) void beam_roll_begin_kernel(int* __restrict__ src_a, int* __restrict__ src_b, int* __restrict__ step,
                                                              int T, int nb, int R) {
    const size_t total = (size_t)R * T;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int base = (int)(i / T) / nb * nb;
        src_a[i] = base;
        src_b[i] = base;
    }
    if (blockIdx.x == 0)
        for (int r = threadIdx.x; r < R; r += 256) step[r] = 0;
}

// One workgroup per row r with turn p = parent[r] (written by the host):
//   p == TURN_FRESH  the row's slot takes a new region this step: src_new[r][0] = the slot's first row, step[r] = 0
//   p == TURN_IDLE   no pending region is left for the row's slot: step[r] = 0 and no table cell is touched
//   otherwise        the row continues beam p of its slot: src_new[r][0 .. t] = src_old[p][0 .. t], src_new[r][t + 1] = p (the slot
//                    the parent's row wrote in the step just run), step[r] = t + 1
// t is the step ALL rows of a slot share, so the row reads it from its own word - the only word of `step` its workgroup writes - and
// no workgroup reads a word another one writes.  Cells behind t + 1 keep what they held.
__global__ __launch_bounds__(256) void beam_roll_turn_kernel(const int* __restrict__ src_old, int* __restrict__ src_new,
                                                             const int* __restrict__ parent, int* __restrict__ step, int T, int nb) {
    const int r = blockIdx.x, p = parent[r];   // uniform over the workgroup, and so is every branch below
    if (p == TURN_IDLE) {
        if (threadIdx.x == 0) step[r] = 0;
        return;
    }
    if (p == TURN_FRESH) {
        if (threadIdx.x == 0) { src_new[(size_t)r * T] = r / nb * nb; step[r] = 0; }
        return;
    }
    const int t = step[r];
    for (int j = threadIdx.x; j <= t; j += 256) src_new[(size_t)r * T + j] = src_old[(size_t)p * T + j];
    __syncthreads();   // every thread has read step[r]
    if (threadIdx.x == 0) { src_new[(size_t)r * T + t + 1] = p; step[r] = t + 1; }
}

static int launch_beam_roll_turn(const int* src_old, int* src_new, const int* parent, int* step, int T, int nb, int R, hipStream_t st) {
    hipLaunchKernelGGL(beam_roll_turn_kernel, dim3(R), dim3(256), 0, st, src_old, src_new, parent, step, T, nb);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// ---- The loop body the one-shot call and the session share: begin, seat, one step with its scorer pass.

// a slot without a region: it runs along at step 0 on BOS rows and its candidates are not read
static void beam_roll_idle(BeamRollState& s, int g) {
    const int r0 = g * s.nb;
    s.region[g] = -1;
    s.cur_len[g] = 1;
    s.done[g] = 0;
    for (int j = 0; j < s.nb; ++j) {
        s.ids[r0 + j].assign(1, BOS_ID);
        s.beam_tok[r0 + j] = BOS_ID;
        s.beam_scores[r0 + j] = 0.f;
        s.turn[r0 + j] = TURN_IDLE;
    }
}

// The host state of G slots of nb rows, every slot idle, and the device tables to match (beam_roll_begin_kernel on d->stream).
static int beam_roll_begin(rgrg_decoder* d, BeamRollState& s, int nb, int G, int max_length, int early_stopping, float length_penalty,
                           int use_graph) {
    const int K = 2 * nb, Ru = G * nb;
    s = BeamRollState{};
    s.nb = nb; s.G = G; s.Ru = Ru; s.max_length = max_length; s.early = early_stopping; s.use_graph = use_graph;
    s.wide = beam_wide(K);
    s.lp = (double)length_penalty;
    s.ids.assign(Ru, std::vector<long long>(1, BOS_ID)); s.nids.resize(Ru);
    s.beam_scores.assign(Ru, 0.f); s.nscore.resize(Ru); s.h_score.resize((size_t)G * K);
    s.beam_tok.assign(Ru, BOS_ID); s.turn.assign(Ru, TURN_IDLE); s.ntok.resize(Ru); s.nidx.resize(Ru);
    s.h_tok.resize((size_t)G * K); s.h_beam.resize((size_t)G * K); s.refill.resize(2 * (size_t)G);
    s.region.assign(G, -1); s.cur_len.assign(G, 1); s.done.assign(G, 0);
    s.src_cur = d->src_a; s.src_nxt = d->src_b;
    hipLaunchKernelGGL(beam_roll_begin_kernel, dim3(64), dim3(256), 0, d->stream, d->src_a, d->src_b, d->roll.step, d->T, nb, Ru);
    RGRG_LAUNCH_CHECK();
    d->logits_stale_rows = 0;   // beam steps write d->logits
    return RGRG_OK;
}

// Free slot g takes region q for the step that is launched next: fresh rows, beam scores 0, -1e9, ..., token BOS, a cur_len of its
// own (the heap is the region's), and the image key / value of q - ring row q / n % Cf of the device block - goes to the refill list.
static void beam_roll_seat(BeamRollState& s, int g, long long q) {
    const int r0 = g * s.nb;
    s.region[g] = q;
    s.cur_len[g] = 1;
    s.done[g] = 0;
    for (int j = 0; j < s.nb; ++j) {
        s.ids[r0 + j].assign(1, BOS_ID);
        s.beam_tok[r0 + j] = BOS_ID;
        s.beam_scores[r0 + j] = j > 0 ? -1e9f : 0.f;
        s.turn[r0 + j] = TURN_FRESH;
    }
    s.refill[2 * s.nrefill] = r0; s.refill[2 * s.nrefill + 1] = (int)q; ++s.nrefill;
    ++s.occupied;
}

// One step on the Ru rows: the turn upload and beam_roll_turn_kernel, the refill list of the slots just seated, the captured step and
// ranking, the three read-backs and ONE synchronisation; then BeamSearchScorer.process per occupied slot on hyps(region), and a
// region that is done, or whose hypotheses have max_length tokens, is finalized - finished(region) - and leaves its slot idle.
template <class Hyps, class Finished>
static int beam_roll_step(rgrg_decoder* d, BeamRollState& s, Hyps&& hyps, Finished&& finished) {
    hipStream_t st = d->stream;
    const int nb = s.nb, K = 2 * nb, G = s.G, Ru = s.Ru;
    int rc;
    // the turn: tables and per-row steps of this step, then the image key / value of the regions seated for it
    RGRG_HIP(hipMemcpyAsync(d->beam_parent, s.turn.data(), Ru * sizeof(int), hipMemcpyHostToDevice, st));
    RGRG_HIP(hipMemcpyAsync(d->beam_tok, s.beam_tok.data(), Ru * sizeof(int), hipMemcpyHostToDevice, st));
    RGRG_HIP(hipMemcpyAsync(d->beam_scores, s.beam_scores.data(), Ru * sizeof(float), hipMemcpyHostToDevice, st));
    if ((rc = launch_beam_roll_turn(s.src_cur, s.src_nxt, d->beam_parent, d->roll.step, d->T, nb, Ru, st))) return rc;
    if ((rc = enqueue_roll_refill_list(d, s.refill.data(), s.nrefill, Ru))) return rc;
    s.nrefill = 0;
    std::swap(s.src_cur, s.src_nxt);
    // the step (embed .. lm_head .. ranking) is captured once per spec - the table it reads is part of it: two graphs - and replayed
    StepSpec step;
    step.rows = Ru; step.tok = d->beam_tok; step.src = s.src_cur; step.row_pos = d->roll.step; step.row_step = d->roll.step;
    step.end = STEP_BEAM; step.nb = nb;
    auto body = [&]() -> int {
        const int r = enqueue_step(d, step, false);
        if (r) return r;
        launch_beam_row_topk(d->logits, d->ld_logits, d->V, Ru, K, d->row_max, d->row_logsum, s.wide ? d->wide_val : d->top_val,
                             s.wide ? d->wide_tok : d->top_tok, false, st);
        launch_beam_merge(d->row_max, d->row_logsum, s.wide ? d->wide_val : d->top_val, s.wide ? d->wide_tok : d->top_tok, d->beam_scores,
                          G, nb, d->V, d->wide_score, d->cand_score, d->cand_tok, d->cand_beam, false, st);
        return RGRG_OK;
    };
    if (s.use_graph) {
        hipGraphExec_t exec = nullptr;
        if ((rc = step_graph(d, step, body, &exec))) return rc;
        RGRG_HIP(hipGraphLaunch(exec, st));
    } else {
        if ((rc = body())) return rc;
        RGRG_LAUNCH_CHECK();
    }
    RGRG_HIP(hipMemcpyAsync(s.h_score.data(), d->cand_score, (size_t)G * K * sizeof(float), hipMemcpyDeviceToHost, st));
    RGRG_HIP(hipMemcpyAsync(s.h_tok.data(), d->cand_tok, (size_t)G * K * sizeof(int), hipMemcpyDeviceToHost, st));
    RGRG_HIP(hipMemcpyAsync(s.h_beam.data(), d->cand_beam, (size_t)G * K * sizeof(int), hipMemcpyDeviceToHost, st));
    RGRG_HIP(hipStreamSynchronize(st));
    // BeamSearchScorer.process per occupied slot; input_ids = cat(input_ids[beam_idx], tokens)
    for (int g = 0; g < G; ++g) {
        if (s.region[g] < 0) continue;
        const int r0 = g * nb;
        const size_t c0 = (size_t)g * K;
        if ((rc = beam_process_group(hyps(s.region[g]), s.done[g], s.h_score.data() + c0, s.h_tok.data() + c0, s.h_beam.data() + c0, nb, nb,
                                     r0, s.ids, s.cur_len[g], s.early != 0, s.lp, s.nscore.data() + r0, s.ntok.data() + r0,
                                     s.nidx.data() + r0)))
            return rc;
        for (int j = 0; j < nb; ++j) { s.nids[r0 + j] = s.ids[s.nidx[r0 + j]]; s.nids[r0 + j].push_back(s.ntok[r0 + j]); }
        for (int j = 0; j < nb; ++j) {
            s.ids[r0 + j].swap(s.nids[r0 + j]);
            s.beam_scores[r0 + j] = s.nscore[r0 + j]; s.beam_tok[r0 + j] = s.ntok[r0 + j]; s.turn[r0 + j] = s.nidx[r0 + j];
        }
        ++s.cur_len[g];
    }
    for (int g = 0; g < G; ++g) {
        if (s.region[g] < 0 || (!s.done[g] && s.cur_len[g] < s.max_length)) continue;
        const int r0 = g * nb;
        const long long q = s.region[g];
        beam_finalize_item(hyps(q), s.done[g] != 0, &s.ids[r0], &s.beam_scores[r0], nb, s.lp);
        beam_roll_idle(s, g);
        --s.occupied;
        finished(q);
    }
    return RGRG_OK;
}

// the arguments the one-shot call and the session's open refuse alike, in this order; -> G
static int beam_roll_check(rgrg_decoder* d, const char* who, int nb, int num_return_sequences, int R) {
    RGRG_CHECK_ARG(nb > 1 && nb <= (1 << 14));
    RGRG_CHECK_ARG(num_return_sequences >= 1 && num_return_sequences <= nb);
    if (R < nb) {
        set_error("%s: %d decoder rows hold no region of %d beams, the cache of this decoder holds %d .. %d", who, R, nb, nb, d->max_seqs);
        return RGRG_EINVAL;
    }
    return RGRG_OK;
}

// the session every call but open and close needs: open, and no other decode entry has run on the decoder since
static int beam_roll_live(rgrg_decoder* d, const char* who) {
    if (!d->bsess.open) { set_error("%s: no rolling beam session is open on this decoder", who); return RGRG_EINVAL; }
    if (d->bsess.epoch != d->epoch) {
        set_error("%s: the rolling beam session is stale: another decode call has used the decoder's cache rows since it was opened (close it and open a new one)", who);
        return RGRG_EINVAL;
    }
    return RGRG_OK;
}

}  // namespace rgrg

using namespace rgrg;

extern "C" int rgrg_decoder_beam_search_rolling(rgrg_decoder* d, const float* feats, int S, int num_beams, int R, int max_length,
                                                int early_stopping, float length_penalty, int num_return_sequences, int64_t* out_ids,
                                                int out_ld, int* out_len, int* steps_out, int use_graph, void* stream) {
    static const char* who = "rgrg_decoder_beam_search_rolling";
    RGRG_CHECK_ARG(d && feats && out_ids && out_len && S > 0);
    const int nb = num_beams, K = 2 * nb;
    int rc;
    if ((rc = beam_roll_check(d, who, nb, num_return_sequences, R))) return rc;
    if ((rc = roll_check(d, who, R, max_length))) return rc;
    RGRG_CHECK_ARG(out_ld >= max_length);
    const int G = std::min(R / nb, S), Ru = G * nb;   // slots, and the rows the step runs on (S <= R / nb: no slot is ever refilled)
    if ((rc = roll_check(d, who, Ru, max_length))) return rc;   // (the cache format is that of the rows in use)
    if (beam_wide(K) && (rc = beam_reserve_wide(d, Ru, K))) return rc;
    if ((rc = roll_reserve(d, S))) return rc;
    if ((rc = decode_begin(d, stream))) return rc;
    hipStream_t st = d->stream;
    // the prefill runs once over the S feature rows, not over S * num_beams: roll.ukv [S][ld_ukv]
    if ((rc = enqueue_roll_prefill(d, feats, S))) return rc;
    const RollCall call{nullptr, nullptr, d->roll.ukv, 0, S, max_length, d->ld_ukv, nullptr, 1, S, S};   // what roll_refill_kernel reads: ukv, ld_ukv, n, Cf
    RGRG_HIP(hipMemcpyAsync(d->roll.call, &call, sizeof(call), hipMemcpyHostToDevice, st));
    RGRG_HIP(hipStreamSynchronize(st));   // `call` is this frame's
    BeamRollState state;
    if ((rc = beam_roll_begin(d, state, nb, G, max_length, early_stopping, length_penalty, use_graph))) return rc;
    std::vector<BeamHyps> hyps(S);
    int next = 0, finished = 0, steps = 0;
    // A region takes at most max_length - 1 steps and a free slot never waits while a region is pending (list scheduling): all S are
    // through within ceil(S / G) (max_length - 1) steps of full slots plus one more region's worth.
    const long long bound = ((long long)(S + G - 1) / G + 1) * (max_length - 1);
    while (finished < S) {
        if (steps >= bound) {
            set_error("%s: %d of %d regions unfinished after the bound of %lld steps on %d slots", who, S - finished, S, bound, G);
            return RGRG_EHIP;
        }
        // free slots - those whose region has just left, and idle ones - take the pending regions in ascending slot order
        for (int g = 0; g < G && next < S; ++g)
            if (state.region[g] < 0) beam_roll_seat(state, g, next++);
        if ((rc = beam_roll_step(d, state, [&](long long q) -> BeamHyps& { return hyps[q]; }, [&](long long) { ++finished; }))) return rc;
        ++steps;   // (every step of the loop has an occupied slot: the loop ends with the last region)
    }
    if ((rc = beam_write_best(hyps, num_return_sequences, max_length, out_ids, out_ld, out_len, st))) return rc;
    if (steps_out) *steps_out = steps;
    return RGRG_OK;   // (logits_valid stays false: the last step's rows belong to different regions at different steps)
}

// ---- The rolling beam session: the call above with an open list.  Regions arrive by submits between steps, their
// image key / value rows live in a ring the decoder owns, their heaps on the host until they are released.

extern "C" int rgrg_decoder_beam_roll_open(rgrg_decoder* d, int R, int num_beams, int capacity, int max_length, int early_stopping,
                                           float length_penalty, int num_return_sequences, int use_graph, void* stream) {
    static const char* who = "rgrg_decoder_beam_roll_open";
    RGRG_CHECK_ARG(d);
    const int nb = num_beams, K = 2 * nb;
    int rc;
    if ((rc = beam_roll_check(d, who, nb, num_return_sequences, R))) return rc;
    const int G = R / nb, Ru = G * nb;   // fixed for the life of the session: there is no S to bound it
    if ((rc = roll_check(d, who, Ru, max_length))) return rc;
    if (capacity < 1) { set_error("%s: a ring of %d regions, at least 1 is needed", who, capacity); return RGRG_EINVAL; }
    if (d->sess.open || d->bsess.open) {
        set_error("%s: a rolling %ssession is already open on this decoder (one per decoder: close it first)", who, d->bsess.open ? "beam " : "");
        return RGRG_EINVAL;
    }
    if (beam_wide(K) && (rc = beam_reserve_wide(d, Ru, K))) return rc;
    if ((rc = roll_reserve(d, capacity))) return rc;
    if ((rc = decode_begin(d, stream))) return rc;
    rgrg_decoder::BeamRollSession& s = d->bsess;
    s = rgrg_decoder::BeamRollSession{};
    s.call = RollCall{nullptr, nullptr, d->roll.ukv, 0, 0, max_length, d->ld_ukv, nullptr, 1, capacity, capacity};
    RGRG_HIP(hipMemcpyAsync(d->roll.call, &s.call, sizeof(s.call), hipMemcpyHostToDevice, d->stream));
    if ((rc = beam_roll_begin(d, s.st, nb, G, max_length, early_stopping, length_penalty, use_graph))) return rc;
    s.capacity = capacity; s.keep = num_return_sequences;
    s.epoch = d->epoch;
    s.open = true;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_beam_roll_submit(rgrg_decoder* d, const float* feats, int m, long long* first_out, void* stream) {
    static const char* who = "rgrg_decoder_beam_roll_submit";
    RGRG_CHECK_ARG(d && feats && m > 0);
    int rc;
    if ((rc = beam_roll_live(d, who))) return rc;
    rgrg_decoder::BeamRollSession& s = d->bsess;
    const long long q0 = s.submitted;
    if (q0 + m >= 0x7fffffffLL) {
        set_error("%s: region numbers of a session stay below %lld (%lld submitted so far): open a new session", who, 0x7fffffffLL, q0);
        return RGRG_EINVAL;
    }
    if (q0 + m > s.watermark + s.capacity) {
        set_error("%s: %d regions do not fit the ring: capacity %d regions, room for %lld until finished regions are collected and "
                  "released", who, m, s.capacity, s.watermark + s.capacity - q0);
        return RGRG_EINVAL;
    }
    RGRG_HIP(hipEventRecord(d->ev_in, as_stream(stream)));   // the feature rows are the caller's stream's
    RGRG_HIP(hipStreamWaitEvent(d->stream, d->ev_in, 0));
    // the three GEMMs of the m rows into their ring rows q % capacity, in two passes where the ring wraps
    const int f0 = (int)(q0 % s.capacity), head = std::min(m, s.capacity - f0);
    if ((rc = enqueue_roll_prefill(d, feats, head, (size_t)f0))) return rc;
    if (m > head && (rc = enqueue_roll_prefill(d, feats + (size_t)head * d->D, m - head, 0))) return rc;
    s.hyps.resize(s.hyps.size() + m);
    s.finalized.resize(s.finalized.size() + m, 0);
    s.submitted = q0 + m;
    if (first_out) *first_out = q0;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_beam_roll_advance(rgrg_decoder* d, int max_steps, int* launched_out, int* unfinished_out, int* steps_out) {
    static const char* who = "rgrg_decoder_beam_roll_advance";
    RGRG_CHECK_ARG(d);
    int rc;
    if ((rc = beam_roll_live(d, who))) return rc;
    rgrg_decoder::BeamRollSession& s = d->bsess;
    BeamRollState& st = s.st;
    auto unfinished = [&] { return (s.submitted - s.next) + st.occupied; };
    // until drained (max_steps < 0): the bound of the one-shot call over what is unfinished now
    const long long bound = ((unfinished() + st.G - 1) / st.G + 1) * (st.max_length - 1);
    const long long limit = max_steps < 0 ? bound : max_steps;
    long long launched = 0;
    while (launched < limit && unfinished() > 0) {
        // a slot is seated only here, in front of a step that is launched: free slots take the pending regions in ascending slot order
        for (int g = 0; g < st.G && s.next < s.submitted; ++g)
            if (st.region[g] < 0) beam_roll_seat(st, g, s.next++);
        if ((rc = beam_roll_step(d, st, [&](long long q) -> BeamHyps& { return s.hyps[(size_t)(q - s.watermark)]; },
                                 [&](long long q) { s.finalized[(size_t)(q - s.watermark)] = 1; })))
            return rc;
        ++launched;
        ++s.steps;   // (the step had an occupied slot)
    }
    if (launched_out) *launched_out = (int)launched;
    if (unfinished_out) *unfinished_out = (int)unfinished();
    if (steps_out) *steps_out = s.steps;
    if (max_steps < 0 && unfinished() != 0) {
        set_error("%s: %lld regions unfinished after the bound of %lld steps on %d slots", who, unfinished(), bound, st.G);
        return RGRG_EHIP;
    }
    return RGRG_OK;
}

extern "C" int rgrg_decoder_beam_roll_collect(rgrg_decoder* d, long long first, int count, int64_t* out_ids, int out_ld, int* out_len,
                                              int* finished_out, void* stream) {
    static const char* who = "rgrg_decoder_beam_roll_collect";
    RGRG_CHECK_ARG(d && count > 0 && (out_ids || finished_out) && (!out_ids || out_len));
    int rc;
    if ((rc = beam_roll_live(d, who))) return rc;
    rgrg_decoder::BeamRollSession& s = d->bsess;
    if (first < s.watermark || first + count > s.submitted) {
        set_error("%s: regions %lld .. %lld, the session holds %lld .. %lld", who, first, first + count - 1, s.watermark, s.submitted - 1);
        return RGRG_EINVAL;
    }
    const size_t i0 = (size_t)(first - s.watermark);
    if (finished_out)
        for (int i = 0; i < count; ++i) finished_out[i] = s.finalized[i0 + i];
    if (!out_ids) return RGRG_OK;
    if (out_ld < s.st.max_length) { set_error("%s: out_ld %d, at least max_length %d is needed", who, out_ld, s.st.max_length); return RGRG_EINVAL; }
    for (int i = 0; i < count; ++i)
        if (!s.finalized[i0 + i]) {
            set_error("%s: region %lld has not finished as of the last advance", who, first + i);
            return RGRG_EINVAL;
        }
    const std::vector<BeamHyps> range(s.hyps.begin() + i0, s.hyps.begin() + i0 + count);
    (void)stream;   // beam_write_best synchronises the decoder's stream, as the one-shot call does
    return beam_write_best(range, s.keep, s.st.max_length, out_ids, out_ld, out_len, d->stream);
}

extern "C" int rgrg_decoder_beam_roll_release(rgrg_decoder* d, long long watermark) {
    static const char* who = "rgrg_decoder_beam_roll_release";
    RGRG_CHECK_ARG(d);
    int rc;
    if ((rc = beam_roll_live(d, who))) return rc;
    rgrg_decoder::BeamRollSession& s = d->bsess;
    if (watermark < s.watermark || watermark > s.submitted) {
        set_error("%s: watermark %lld, %lld .. %lld are possible", who, watermark, s.watermark, s.submitted);
        return RGRG_EINVAL;
    }
    for (long long q = s.watermark; q < watermark; ++q)
        if (!s.finalized[(size_t)(q - s.watermark)]) {
            set_error("%s: region %lld below the new watermark %lld has not finished", who, q, watermark);
            return RGRG_EINVAL;
        }
    const size_t n = (size_t)(watermark - s.watermark);
    s.hyps.erase(s.hyps.begin(), s.hyps.begin() + n);
    s.finalized.erase(s.finalized.begin(), s.finalized.begin() + n);
    s.watermark = watermark;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_beam_roll_close(rgrg_decoder* d) {
    RGRG_CHECK_ARG(d);
    if (!d->bsess.open) return RGRG_OK;
    const hipError_t e = hipStreamSynchronize(d->stream);   // a submit's GEMMs may be queued
    d->bsess = rgrg_decoder::BeamRollSession{};
    if (e != hipSuccess) { set_error("rgrg_decoder_beam_roll_close: %s", hipGetErrorString(e)); return RGRG_EHIP; }
    return RGRG_OK;
}

// Test hook: beam_roll_turn_kernel alone, as the rolling loop launches it.  Device int32: src_old / src_new [R][T] (two buffers),
// parent [R] (a row of the row's slot, -1 = fresh, -2 = idle), step [R] (updated in place).  Read back and checked first (one
// synchronisation): R a multiple of nb, a parent inside its row's slot, one step per slot among its continuing rows, 0 <= step <= T - 2.
extern "C" int rgrg_debug_beam_roll_turn(const int* src_old, int* src_new, const int* parent, int* step, int T, int nb, int R, void* stream) {
    RGRG_CHECK_ARG(src_old && src_new && src_old != src_new && parent && step && T >= 2 && nb >= 1 && R >= nb && R % nb == 0 && R < 65536);
    std::vector<int> hp(R), hs(R);
    hipStream_t st = as_stream(stream);
    RGRG_HIP(hipStreamSynchronize(st));
    RGRG_HIP(hipMemcpy(hp.data(), parent, (size_t)R * sizeof(int), hipMemcpyDeviceToHost));
    RGRG_HIP(hipMemcpy(hs.data(), step, (size_t)R * sizeof(int), hipMemcpyDeviceToHost));
    for (int r = 0; r < R; ++r) {
        const int p = hp[r], base = r / nb * nb;
        if (p == TURN_FRESH || p == TURN_IDLE) continue;
        if (p < base || p >= base + nb) {
            set_error("rgrg_debug_beam_roll_turn: parent[%d] = %d, the row's slot holds rows %d .. %d (-1 fresh, -2 idle)", r, p, base, base + nb - 1);
            return RGRG_EINVAL;
        }
        int first = r;   // the slot's first continuing row: every other one stands at its step
        for (int q = base; q < r; ++q)
            if (hp[q] != TURN_FRESH && hp[q] != TURN_IDLE) { first = q; break; }
        if (hs[r] < 0 || hs[r] > T - 2 || hs[p] != hs[r] || hs[first] != hs[r]) {
            set_error("rgrg_debug_beam_roll_turn: step[%d] = %d, parent %d at step %d, row %d at step %d: the rows of a slot share one step 0 .. %d",
                      r, hs[r], p, hs[p], first, hs[first], T - 2);
            return RGRG_EINVAL;
        }
    }
    const int rc = launch_beam_roll_turn(src_old, src_new, parent, step, T, nb, R, st);
    if (rc) return rc;
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) { set_error("rgrg_debug_beam_roll_turn: %s", hipGetErrorString(e)); return RGRG_EHIP; }
    return RGRG_OK;
}
