// Sampling decode (rgrg_decoder_sample): the decode loop of rgrg_decoder_generate (run_decode_loop, decoder.hip) with the step's
// arg-max replaced by the token sampler (sample.hip).  A STEP_SAMPLE step leaves logits - as a beam step does, on every step plan -
// and ends in ONE sample_kernel launch, which draws the token and does the greedy bookkeeping.
#include "decoder_internal.h"

using namespace rgrg;

int rgrg::enqueue_sampler(rgrg_decoder* d, int S) {
    return launch_sample_step(d->logits, d->ld_logits, S, d->V, d->sample_prm, d->ids, d->max_len, d->finished, d->step, d->done_len,
                              d->sync, d->sample_lp, d->max_len, d->stream);
}

extern "C" int rgrg_decoder_sample(rgrg_decoder* d, const float* feats, int S, int max_length, float temperature, int top_k,
                                   float top_p, uint64_t seed, int64_t* out_ids, int out_ld, float* out_logprobs, int* out_len,
                                   int use_graph, void* stream) {
    RGRG_CHECK_ARG(d && feats && out_ids && out_len && S > 0 && S <= d->max_seqs);
    const int limit = (max_length > 0) ? max_length : d->max_len;
    RGRG_CHECK_ARG(limit >= 2 && limit <= d->max_len && out_ld >= limit);
    int rc;
    if ((rc = sample_begin(d, S, temperature, top_k, top_p, seed, stream))) return rc;
    StepSpec step;
    step.rows = S; step.end = STEP_SAMPLE;
    if ((rc = run_decode_loop(d, feats, step, nullptr, limit, use_graph, out_ids, out_ld, out_logprobs, out_len))) return rc;
    d->logits_stale_rows = 0;   // every step wrote d->logits: the logits the last draw was made from
    return RGRG_OK;
}

// what every sampling entry does before its decode loop: buffers, d->stream behind the caller's, the parameter block, zero log-probs
int rgrg::sample_begin(rgrg_decoder* d, int S, float temperature, int top_k, float top_p, uint64_t seed, void* stream) {
    int rc;
    if (!d->sample_prm && (rc = dmalloc(d, &d->sample_prm, sample_params_bytes(), true))) return rc;
    if (!d->sample_lp && (rc = dmalloc(d, (void**)&d->sample_lp, (size_t)d->rows * d->max_len * sizeof(float), true))) return rc;
    if ((rc = decode_begin(d, stream))) return rc;
    // the parameter block lives in device memory: the captured step serves every seed and parameter set
    if ((rc = enqueue_sample_params(d->sample_prm, temperature, top_k, top_p, seed, d->stream))) return rc;
    RGRG_HIP(hipMemsetAsync(d->sample_lp, 0, (size_t)S * d->max_len * sizeof(float), d->stream));   // BOS / prompt columns, steps not run
    return RGRG_OK;
}
