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

}  // namespace rgrg

using namespace rgrg;

extern "C" int rgrg_decoder_beam_search_rolling(rgrg_decoder* d, const float* feats, int S, int num_beams, int R, int max_length,
                                                int early_stopping, float length_penalty, int num_return_sequences, int64_t* out_ids,
                                                int out_ld, int* out_len, int* steps_out, int use_graph, void* stream) {
    static const char* who = "rgrg_decoder_beam_search_rolling";
    RGRG_CHECK_ARG(d && feats && out_ids && out_len && S > 0 && num_beams > 1 && num_beams <= (1 << 14));
    RGRG_CHECK_ARG(num_return_sequences >= 1 && num_return_sequences <= num_beams);
    const int nb = num_beams, K = 2 * nb;
    if (R < nb) {
        set_error("%s: %d decoder rows hold no region of %d beams, the cache of this decoder holds %d .. %d", who, R, nb, nb, d->max_seqs);
        return RGRG_EINVAL;
    }
    int rc;
    if ((rc = roll_check(d, who, R, max_length))) return rc;
    RGRG_CHECK_ARG(out_ld >= max_length);
    const int G = std::min(R / nb, S), Ru = G * nb;   // slots, and the rows the step runs on (S <= R / nb: no slot is ever refilled)
    if ((rc = roll_check(d, who, Ru, max_length))) return rc;   // (the cache format is that of the rows in use)
    const bool wide = beam_wide(K);
    if (wide && (rc = beam_reserve_wide(d, Ru, K))) return rc;
    if ((rc = roll_reserve(d, S))) return rc;
    if ((rc = decode_begin(d, stream))) return rc;
    hipStream_t st = d->stream;
    // the prefill runs once over the S feature rows, not over S * num_beams: roll.ukv [S][ld_ukv]
    if ((rc = enqueue_roll_prefill(d, feats, S))) return rc;
    const RollCall call{nullptr, nullptr, d->roll.ukv, 0, S, max_length, d->ld_ukv, nullptr, 1, S, S};   // what roll_refill_kernel reads: ukv, ld_ukv, n, Cf
    RGRG_HIP(hipMemcpyAsync(d->roll.call, &call, sizeof(call), hipMemcpyHostToDevice, st));
    RGRG_HIP(hipStreamSynchronize(st));   // `call` is this frame's
    hipLaunchKernelGGL(beam_roll_begin_kernel, dim3(64), dim3(256), 0, st, d->src_a, d->src_b, d->roll.step, d->T, nb, Ru);
    RGRG_LAUNCH_CHECK();

    // host state, per row of the Ru rows ...
    std::vector<std::vector<long long>> ids(Ru, std::vector<long long>(1, BOS_ID)), nids(Ru);
    std::vector<float> beam_scores(Ru, 0.f), nscore(Ru), h_score((size_t)G * K);
    std::vector<int> beam_tok(Ru, BOS_ID), turn(Ru, TURN_IDLE), ntok(Ru), nidx(Ru), h_tok((size_t)G * K), h_beam((size_t)G * K), refill(2 * (size_t)G);
    // ... per slot: the region it holds (-1 = idle), that region's cur_len and `done` flag; per region: its heap
    std::vector<int> region(G, -1), cur_len(G, 0);
    std::vector<char> done(G, 0);
    std::vector<BeamHyps> hyps(S);
    const double lp = (double)length_penalty;
    int next = 0, finished = 0, steps = 0, nrefill = 0;
    // a free slot takes the next pending region (the caller walks the slots in ascending order): fresh rows, beam scores 0, -1e9, ...,
    // token BOS, a heap and a cur_len of its own; without one it is idle
    auto seat = [&](int g) {
        const int r0 = g * nb;
        const bool given = next < S;
        region[g] = given ? next : -1;
        cur_len[g] = 1;
        done[g] = 0;
        for (int j = 0; j < nb; ++j) {
            ids[r0 + j].assign(1, BOS_ID);
            beam_tok[r0 + j] = BOS_ID;
            beam_scores[r0 + j] = (given && j > 0) ? -1e9f : 0.f;
            turn[r0 + j] = given ? TURN_FRESH : TURN_IDLE;
        }
        if (given) { refill[2 * nrefill] = r0; refill[2 * nrefill + 1] = next; ++nrefill; ++next; }
    };
    for (int g = 0; g < G; ++g) seat(g);

    int* src_cur = d->src_a;
    int* src_nxt = d->src_b;
    auto enqueue_ranking = [&]() -> int {
        launch_beam_row_topk(d->logits, d->ld_logits, d->V, Ru, K, d->row_max, d->row_logsum, wide ? d->wide_val : d->top_val,
                             wide ? d->wide_tok : d->top_tok, false, st);
        launch_beam_merge(d->row_max, d->row_logsum, wide ? d->wide_val : d->top_val, wide ? d->wide_tok : d->top_tok, d->beam_scores,
                          G, nb, d->V, d->wide_score, d->cand_score, d->cand_tok, d->cand_beam, false, st);
        return RGRG_OK;
    };
    d->logits_stale_rows = 0;   // beam steps write d->logits
    // A region takes at most max_length - 1 steps and a free slot never waits while a region is pending (list scheduling): all S are
    // through within ceil(S / G) (max_length - 1) steps of full slots plus one more region's worth.
    const long long bound = ((long long)(S + G - 1) / G + 1) * (max_length - 1);
    while (finished < S) {
        if (steps >= bound) {
            set_error("%s: %d of %d regions unfinished after the bound of %lld steps on %d slots", who, S - finished, S, bound, G);
            return RGRG_EHIP;
        }
        // the turn: tables and per-row steps of this step, then the image key / value of the regions seated for it
        RGRG_HIP(hipMemcpyAsync(d->beam_parent, turn.data(), Ru * sizeof(int), hipMemcpyHostToDevice, st));
        RGRG_HIP(hipMemcpyAsync(d->beam_tok, beam_tok.data(), Ru * sizeof(int), hipMemcpyHostToDevice, st));
        RGRG_HIP(hipMemcpyAsync(d->beam_scores, beam_scores.data(), Ru * sizeof(float), hipMemcpyHostToDevice, st));
        if ((rc = launch_beam_roll_turn(src_cur, src_nxt, d->beam_parent, d->roll.step, d->T, nb, Ru, st))) return rc;
        if ((rc = enqueue_roll_refill_list(d, refill.data(), nrefill, Ru))) return rc;
        nrefill = 0;
        { int* tmp = src_cur; src_cur = src_nxt; src_nxt = tmp; }
        // the step (embed .. lm_head .. ranking) is captured once per spec - the table it reads is part of it: two graphs - and replayed
        StepSpec step;
        step.rows = Ru; step.tok = d->beam_tok; step.src = src_cur; step.row_pos = d->roll.step; step.row_step = d->roll.step;
        step.end = STEP_BEAM; step.nb = nb;
        auto body = [&]() -> int {
            const int r = enqueue_step(d, step, false);
            return r ? r : enqueue_ranking();
        };
        if (use_graph) {
            hipGraphExec_t exec = nullptr;
            if ((rc = step_graph(d, step, body, &exec))) return rc;
            RGRG_HIP(hipGraphLaunch(exec, st));
        } else {
            if ((rc = body())) return rc;
            RGRG_LAUNCH_CHECK();
        }
        RGRG_HIP(hipMemcpyAsync(h_score.data(), d->cand_score, (size_t)G * K * sizeof(float), hipMemcpyDeviceToHost, st));
        RGRG_HIP(hipMemcpyAsync(h_tok.data(), d->cand_tok, (size_t)G * K * sizeof(int), hipMemcpyDeviceToHost, st));
        RGRG_HIP(hipMemcpyAsync(h_beam.data(), d->cand_beam, (size_t)G * K * sizeof(int), hipMemcpyDeviceToHost, st));
        RGRG_HIP(hipStreamSynchronize(st));
        ++steps;   // (every step of the loop has an occupied slot: the loop ends with the last region)
        // BeamSearchScorer.process per occupied slot; input_ids = cat(input_ids[beam_idx], tokens)
        for (int g = 0; g < G; ++g) {
            if (region[g] < 0) continue;
            const int r0 = g * nb;
            const size_t c0 = (size_t)g * K;
            if ((rc = beam_process_group(hyps[region[g]], done[g], h_score.data() + c0, h_tok.data() + c0, h_beam.data() + c0, nb, nb, r0, ids,
                                         cur_len[g], early_stopping != 0, lp, nscore.data() + r0, ntok.data() + r0, nidx.data() + r0)))
                return rc;
            for (int j = 0; j < nb; ++j) { nids[r0 + j] = ids[nidx[r0 + j]]; nids[r0 + j].push_back(ntok[r0 + j]); }
            for (int j = 0; j < nb; ++j) {
                ids[r0 + j].swap(nids[r0 + j]);
                beam_scores[r0 + j] = nscore[r0 + j]; beam_tok[r0 + j] = ntok[r0 + j]; turn[r0 + j] = nidx[r0 + j];
            }
            ++cur_len[g];
        }
        // a region that is done, or whose hypotheses have max_length tokens, is finalized and leaves; free slots - these, and idle ones -
        // take the pending regions in ascending slot order
        for (int g = 0; g < G; ++g) {
            if (region[g] >= 0) {
                if (!done[g] && cur_len[g] < max_length) continue;
                const int r0 = g * nb;
                beam_finalize_item(hyps[region[g]], done[g] != 0, &ids[r0], &beam_scores[r0], nb, lp);
                ++finished;
            }
            seat(g);
        }
    }
    if ((rc = beam_write_best(hyps, num_return_sequences, max_length, out_ids, out_ld, out_len, st))) return rc;
    if (steps_out) *steps_out = steps;
    return RGRG_OK;   // (logits_valid stays false: the last step's rows belong to different regions at different steps)
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
