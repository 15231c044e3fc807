// Prompted greedy decode (rgrg_decoder_generate_prompted; LanguageModel.greedy_search with a prompt, language_model.py:609-652):
// the image slot as in rgrg_decoder_generate, then ONE teacher-forced pass over the S x T prompt rows (tf_hidden_pass,
// decoder_lm.hip) whose keys / values go to slots 1 .. T of the decode cache, lm_head + arg-max over the S last-position rows, and
// the decode loop of rgrg_decoder_generate from step T on.  A left-padded prompt keeps its padded slots out of every later step and
// embeds every row's tokens at the row's own position (prepare_inputs_for_generation, :498-520).
// rgrg_decoder_sample_prompted is the same entry with the sampler behind the prompt's last position and behind every step.
// rgrg_decoder_beam_search_prompted (beam_search, :529-607) runs the prompt pass once per ITEM: the nb beams of an item share its
// prompt, whose keys / values live once, in cache row s * nb, and reach every beam row through the ancestor table.
#include <algorithm>

#include "decoder_internal.h"

using namespace rgrg;

namespace rgrg {
namespace {

enum { MASK_ROW_EMPTY = 1, MASK_NOT_LEFT = 2, MASK_HAS_PAD = 4, MASK_NOT_BINARY = 8 };

// One thread per row of attention_mask [S][T]: pad[s] = the zeros in front; flags |= what the host refuses or needs to know
__global__ __launch_bounds__(256) void prompt_mask_scan_kernel(const float* __restrict__ am, int S, int T, int* __restrict__ pad,
                                                               int* __restrict__ flags) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    int p = 0, f = 0;
    while (p < T && am[(size_t)s * T + p] == 0.f) ++p;
    if (p == T) f |= MASK_ROW_EMPTY;
    if (p > 0) f |= MASK_HAS_PAD;
    for (int t = p; t < T; ++t) {
        const float v = am[(size_t)s * T + t];
        if (v == 0.f) f |= MASK_NOT_LEFT;
        else if (v != 1.f) f |= MASK_NOT_BINARY;
    }
    pad[s] = p;
    if (f) atomicOr(flags, f);
}

// The prompt into the id buffer (ids clamped into the vocabulary like forward_cached_tokens_kernel: the host mirror rejects others),
// the step counter onto the last prompt position and - a padded prompt - position ids cumsum(mask) - 1, 1 where masked (:506-509),
// plus the additive mask of every cache slot for the fp32 attention kernel: -1e4 on slots 1 .. pad[s], 0 on the image slot and on
// everything behind the prompt (:316-334, :522-527)
__global__ __launch_bounds__(256) void prompt_setup_kernel(const long long* __restrict__ in, int S, int T, int V, long long* __restrict__ ids,
                                                           int ld_ids, int* __restrict__ step, const int* __restrict__ pad,
                                                           long long* __restrict__ pos, float* __restrict__ kmask, int slots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *step = T - 1;
    if (i < S * T) {
        const int s = i / T, t = i - s * T;
        const long long tok = in[i];
        ids[(size_t)s * ld_ids + t] = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
        if (pad) pos[i] = t >= pad[s] ? t - pad[s] : 1;
    }
    if (kmask && i < S * slots) {
        const int s = i / slots, j = i - s * slots;
        kmask[i] = (j >= 1 && j <= pad[s]) ? -10000.0f : 0.f;
    }
}

// q | k | v rows [S*T][3D] (fp32) of one layer -> slots 1 .. T of the decode cache planes [rows][H][slots][64] of that layer.  A
// (sequence, head) owns T consecutive slots = T * 64 consecutive elements of a plane; a lane moves 16 bytes of the DESTINATION:
// consecutive lanes write consecutive 16-byte pieces (a wave 1 KiB in one piece) and read whole 256-byte head rows of the source.
// row_mul: sequence s owns cache row s * row_mul (beam search: the first beam row of the item).
template <typename KV>   // float, or u16 in the 16-bit type f16
__global__ __launch_bounds__(256) void prompt_kv_store_kernel(const float* __restrict__ qkv, KV* __restrict__ kplane, KV* __restrict__ vplane,
                                                              int S, int H, int T, int slots, int f16, int row_mul) {
    constexpr int PER = 16 / sizeof(KV);      // elements per lane
    constexpr int LANES = 64 / PER;           // lanes per head row
    const int D = H * 64;
    const size_t total = (size_t)S * H * 2 * T * LANES;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int e = (int)(i % LANES) * PER;
        size_t r = i / LANES;
        const int t = (int)(r % T); r /= T;
        const int kv = (int)(r & 1); r >>= 1;
        const int hd = (int)(r % H), s = (int)(r / H);
        const float* src = qkv + ((size_t)s * T + t) * 3 * D + (size_t)(1 + kv) * D + hd * 64 + e;
        KV* dst = (kv ? vplane : kplane) + (((size_t)s * row_mul * H + hd) * slots + 1 + t) * 64 + e;
        const f32x4 a = *reinterpret_cast<const f32x4*>(src);
        if constexpr (sizeof(KV) == 4) {
            *reinterpret_cast<f32x4*>(dst) = a;
        } else {
            const f32x4 b = *reinterpret_cast<const f32x4*>(src + 4);
            u32x4 o;
            o[0] = to16_rt(a[0], f16) | (to16_rt(a[1], f16) << 16);
            o[1] = to16_rt(a[2], f16) | (to16_rt(a[3], f16) << 16);
            o[2] = to16_rt(b[0], f16) | (to16_rt(b[1], f16) << 16);
            o[3] = to16_rt(b[2], f16) | (to16_rt(b[3], f16) << 16);
            *reinterpret_cast<u32x4*>(dst) = o;
        }
    }
}

// ln_f row of every sequence's last prompt position -> the decode step's lm_head input (fp32, and 16 bit where that step reads
// 16-bit activations): the lm_head runs on S rows, not S x T.  Block r writes row r from sequence r / row_div (beam search: the nb
// rows of an item start from the same row).
__global__ __launch_bounds__(256) void prompt_last_rows_kernel(const float* __restrict__ xn_all, int T, int D, float* __restrict__ xn,
                                                               u16* __restrict__ xn16, int f16, int row_div) {
    const int r = blockIdx.x, s = r / row_div, tid = threadIdx.x;   // D == 1024
    const f32x4 v = reinterpret_cast<const f32x4*>(xn_all + ((size_t)s * T + T - 1) * D)[tid];
    reinterpret_cast<f32x4*>(xn + (size_t)r * D)[tid] = v;
    if (xn16) store_16x4(xn16 + (size_t)r * D + 4 * tid, v, f16);
}

// Beam search from a prompt: slots 0 .. T of all R = S * nb rows of BOTH ancestor tables -> row (r / nb) * nb, where the image slot
// and the prompt pass put them; beam_pad[r] = the padded prompt slots of the row's item (0 without padding)
__global__ __launch_bounds__(256) void beam_prompt_init_kernel(int* __restrict__ src_a, int* __restrict__ src_b, int slots, int nb, int R,
                                                               int T, const int* __restrict__ pad, int* __restrict__ beam_pad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * (T + 1)) return;
    const int r = i / (T + 1), j = i - r * (T + 1);
    src_a[(size_t)r * slots + j] = (r / nb) * nb;
    src_b[(size_t)r * slots + j] = (r / nb) * nb;
    if (j == 0) beam_pad[r] = pad ? pad[r / nb] : 0;
}

// Before every beam step behind a padded prompt: beam row r embeds its token at position step - pad of its item
__global__ __launch_bounds__(256) void beam_row_pos_kernel(const int* __restrict__ step, const int* __restrict__ beam_pad,
                                                           int* __restrict__ row_pos, int R) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < R) row_pos[r] = *step - beam_pad[r];
}

// Before every step behind a padded prompt: row s embeds its token at position step - pad[s] (the cache slot stays step + 1); the
// fused plan takes token and position per row together (DX_EMBED_TOKPOS), so the token is read out of the id buffer as well
__global__ __launch_bounds__(256) void prompt_step_rows_kernel(const long long* __restrict__ ids, int ld_ids, const int* __restrict__ step,
                                                               const int* __restrict__ pad, int* __restrict__ tok, int* __restrict__ row_pos, int S) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const int t = *step;
    tok[s] = (int)ids[(size_t)s * ld_ids + t];
    row_pos[s] = t - pad[s];
}

// The launches of the kernels above on raw pointers: the product path below and the test hooks at the end of the file share them.
int launch_prompt_mask_scan(const float* am, int S, int T, int* pad, int* flags, hipStream_t st) {
    hipLaunchKernelGGL(prompt_mask_scan_kernel, dim3((S + 255) / 256), dim3(256), 0, st, am, S, T, pad, flags);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
// one thread per prompt token and, with kmask, per cache slot of the S rows
int launch_prompt_setup(const long long* in, int S, int T, int V, long long* ids, int ld_ids, int* step, const int* pad, long long* pos,
                        float* kmask, int slots, hipStream_t st) {
    const int n = std::max(S * T, kmask ? S * slots : 0);
    hipLaunchKernelGGL(prompt_setup_kernel, dim3((n + 255) / 256), dim3(256), 0, st, in, S, T, V, ids, ld_ids, step, pad, pos, kmask, slots);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
int launch_prompt_last_rows(const float* xn_all, int T, int D, float* xn, u16* xn16, int f16, int row_div, int R, hipStream_t st) {
    hipLaunchKernelGGL(prompt_last_rows_kernel, dim3(R), dim3(256), 0, st, xn_all, T, D, xn, xn16, f16, row_div);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
int launch_prompt_step_rows(const long long* ids, int ld_ids, const int* step, const int* pad, int* tok, int* row_pos, int S, hipStream_t st) {
    hipLaunchKernelGGL(prompt_step_rows_kernel, dim3((S + 255) / 256), dim3(256), 0, st, ids, ld_ids, step, pad, tok, row_pos, S);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
int launch_beam_prompt_init(int* src_a, int* src_b, int slots, int nb, int R, int T, const int* pad, int* beam_pad, hipStream_t st) {
    hipLaunchKernelGGL(beam_prompt_init_kernel, dim3((R * (T + 1) + 255) / 256), dim3(256), 0, st, src_a, src_b, slots, nb, R, T, pad, beam_pad);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
int launch_beam_row_pos(const int* step, const int* beam_pad, int* row_pos, int R, hipStream_t st) {
    hipLaunchKernelGGL(beam_row_pos_kernel, dim3((R + 255) / 256), dim3(256), 0, st, step, beam_pad, row_pos, R);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

struct PromptCall {
    const long long* ids;
    const float* am;     // NULL unless the prompt is padded
    int S, T;
    int row_mul = 1;     // beam search: num_beams - sequence s owns cache row s * row_mul, the cache format is that of S * row_mul rows
    bool sample = false; // the token behind the prompt is drawn (enqueue_sampler), not the arg-max
};

int store_prompt_kv(rgrg_decoder* d, int l, const float* qkv, const void* arg) {
    const PromptCall& c = *static_cast<const PromptCall*>(arg);
    const int S = c.S, fmt = rgrg_decoder_kv_format_in_use(d, S * c.row_mul);
    if (fmt == KV_F32) {
        float* kc = d->kv + (size_t)l * d->kv_layer_stride;
        return launch_prompt_kv_store(qkv, kc, kc + d->kv_kv_stride, S, d->H, c.T, d->T, c.row_mul, false, 0, d->stream);
    }
    // the 16-bit cache lives in the same allocation with the same element strides (enqueue_prefill)
    u16* kc = reinterpret_cast<u16*>(d->kv) + (size_t)l * d->kv_layer_stride;
    return launch_prompt_kv_store(qkv, kc, kc + d->kv_kv_stride, S, d->H, c.T, d->T, c.row_mul, true, d->f16(), d->stream);
}

// The prompt pass of every prompted entry, between the image slot and the head: ids, step counter and position ids (and, with
// kmask, the additive mask of the S rows' cache slots), the teacher-forced pass over the S x T prompt rows with keys / values into
// slots 1 .. T of cache row s * row_mul, and the ln_f row of every sequence's last position in the lm_head input of its row_mul rows
int enqueue_prompt_pass(rgrg_decoder* d, const PromptCall& c, float* kmask) {
    const int S = c.S, T = c.T, R = S * c.row_mul, fmt = rgrg_decoder_kv_format_in_use(d, R);
    hipStream_t st = d->stream;
    int rc;
    if ((rc = launch_prompt_setup(c.ids, S, T, d->V, d->ids, d->max_len, d->step, c.am ? d->prompt_pad : (const int*)nullptr, d->prompt_pos, kmask,
                                  d->T, st)))
        return rc;
    if ((rc = tf_hidden_pass(d, c.ids, c.am, c.am ? d->prompt_pos : nullptr, c.am ? S * T : 1, S, T, store_prompt_kv, &c))) return rc;
    u16* xn16 = (fmt != KV_F32 && d->xn16) ? d->xn16 : nullptr;
    return launch_prompt_last_rows(d->tf.xn, T, d->D, d->xn, xn16, d->f16(), c.row_mul, R, st);
}

// the prologue of run_decode_loop: everything between the image slot and step T
int enqueue_prompt(rgrg_decoder* d, int S, const void* arg) {
    const PromptCall& c = *static_cast<const PromptCall*>(arg);
    int rc;
    // the fp32 attention kernel takes the additive mask, the 16-bit one pad[] itself
    const bool mask32 = c.am && rgrg_decoder_kv_format_in_use(d, S) == KV_F32;
    if ((rc = enqueue_prompt_pass(d, c, mask32 ? d->key_mask : nullptr))) return rc;
    if (!c.sample) return enqueue_head_argmax(d, S);
    // the device step word is T - 1: the Philox counter of row r for the token in column T is (r, T - 1), as a step would have it
    if ((rc = enqueue_head_logits(d, S))) return rc;
    return enqueue_sampler(d, S);
}

// in front of every greedy / sampling step behind a padded prompt
int enqueue_prompt_step_rows(rgrg_decoder* d, int S) {
    return launch_prompt_step_rows(d->ids, d->max_len, d->step, d->prompt_pad, d->beam_tok, d->row_pos, S, d->stream);
}

// The mask scan of every prompted entry on d->stream, with ONE read-back: a mask the kernels cannot honour is refused before any
// work.  -> *padded; d->prompt_pad[s] = the zeros in front of row s.  extra_dst / extra_src: a copy that rides on the same wait.
int prompt_mask_check(rgrg_decoder* d, const char* who, const float* attention_mask, int S, int T, bool* padded, void* extra_dst = nullptr,
                      const void* extra_src = nullptr, size_t extra_bytes = 0) {
    int rc;
    *padded = false;
    if (!d->prompt_pad && (rc = dmalloc(d, (void**)&d->prompt_pad, (size_t)d->rows * sizeof(int), true))) return rc;
    if (extra_dst) RGRG_HIP(hipMemcpyAsync(extra_dst, extra_src, extra_bytes, hipMemcpyDeviceToHost, d->stream));
    if (attention_mask) {
        int* flags = d->next;   // a scratch word of the decoder
        RGRG_HIP(hipMemsetAsync(flags, 0, sizeof(int), d->stream));
        if ((rc = launch_prompt_mask_scan(attention_mask, S, T, d->prompt_pad, flags, d->stream))) return rc;
        RGRG_HIP(hipMemcpyAsync(d->h_done, flags, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    }
    if (attention_mask || extra_dst) RGRG_HIP(hipStreamSynchronize(d->stream));
    if (attention_mask) {
        const int f = *d->h_done;
        if (f & (MASK_ROW_EMPTY | MASK_NOT_LEFT | MASK_NOT_BINARY)) {
            set_error("%s: attention_mask %s", who, (f & MASK_ROW_EMPTY) ? "has a row of zeros only (no token to continue from)"
                      : (f & MASK_NOT_LEFT) ? "is not left padding (a zero behind a one): only padding in front of the prompt is supported"
                      : "holds values other than 0 and 1");
            return RGRG_EINVAL;
        }
        *padded = (f & MASK_HAS_PAD) != 0;
    }
    if (*padded) {
        if (!d->prompt_pos && (rc = dmalloc(d, (void**)&d->prompt_pos, (size_t)d->rows * d->max_len * sizeof(long long), true))) return rc;
        if (!d->key_mask && (rc = dmalloc(d, (void**)&d->key_mask, (size_t)d->rows * d->T * sizeof(float), true))) return rc;
    }
    return RGRG_OK;
}

// What every prompted entry refuses before any work, as `who`; rows: the token rows of its steps.  -> *limit, the length the call
// decodes to.  Greedy search and sampling always produce one token: max_length <= 0 means the cache, a shorter one grows to T + 1.
// Beam search (:541, :597-605): the first iteration always runs, and finalize cannot hold a hypothesis longer than max_length.
int check_prompted(rgrg_decoder* d, const char* who, int rows, int T, int max_length, bool beam, int out_ld, int* limit_out) {
    int limit = max_length;
    if (beam) {
        if (max_length < T + 1 || max_length > d->max_len) {
            set_error("%s: max_length %d with a prompt of %d tokens: %d .. %d (the cache) are possible", who, max_length, T, T + 1, d->max_len);
            return RGRG_EINVAL;
        }
    } else {
        if (T + 1 > d->max_len) {
            set_error("%s: a prompt of %d tokens and one generated token need %d token slots, the cache has %d", who, T, T + 1, d->max_len);
            return RGRG_EINVAL;
        }
        limit = std::max(max_length > 0 ? max_length : d->max_len, T + 1);   // greedy_search (:622, :649): cur_len starts at T
        RGRG_CHECK_ARG(limit <= d->max_len && out_ld >= limit);
    }
    *limit_out = limit;
    if (rgrg_decoder_kv_format_in_use(d, rows) == KV_E4M3) {
        set_error("%s: the e4m3 K/V cache takes no prompt: call rgrg_decoder_set_kv_format(d, 0) first", who);
        return RGRG_EINVAL;
    }
    return RGRG_OK;
}

// rgrg_decoder_generate_prompted / rgrg_decoder_sample_prompted behind decode_begin / sample_begin: mask scan, prompt pass, loop
int prompted_decode_loop(rgrg_decoder* d, const char* who, const float* feats, const int64_t* input_ids, const float* attention_mask, int S,
                         int T, int limit, StepEnd end, int use_graph, int64_t* out_ids, int out_ld, float* out_logprobs, int* out_len) {
    int rc;
    bool padded = false;
    if ((rc = prompt_mask_check(d, who, attention_mask, S, T, &padded))) return rc;
    if ((rc = tf_reserve(d, (size_t)S * T))) return rc;
    PromptCall call{reinterpret_cast<const long long*>(input_ids), padded ? attention_mask : nullptr, S, T};
    call.sample = end == STEP_SAMPLE;
    const DecodePrologue pro{enqueue_prompt, &call, T};
    // a mask of ones leaves the steps of the entry without a prompt (and their captured graph); behind a padded prompt the step has
    // per-row positions and padded slots - and, on the fused plan, which embeds token and position per row together, its tokens
    // from prompt_step_rows_kernel
    StepSpec step;
    step.rows = S; step.end = end;
    if (padded) {
        step = padded_step_spec(d, step, d->prompt_pad);
        if (S <= rgrg_decoder_row_limit(d)) step.tok = d->beam_tok;
    }
    return run_decode_loop(d, feats, step, padded ? enqueue_prompt_step_rows : nullptr, limit, use_graph, out_ids, out_ld, out_logprobs,
                           out_len, &pro);
}

}  // namespace

// (declared in decoder_internal.h: the rolling session's prompt pass writes its ring through it)  kv16: the planes are 16 bit in the type f16; at most 4096 workgroups, the kernel strides
int launch_prompt_kv_store(const float* qkv, void* kplane, void* vplane, int S, int H, int T, int slots, int row_mul, bool kv16, int f16,
                           hipStream_t st) {
    const size_t total = (size_t)S * H * 2 * T * (kv16 ? 8 : 16);
    const dim3 grid((unsigned)std::min<size_t>((total + 255) / 256, 4096)), blk(256);
    if (!kv16)
        hipLaunchKernelGGL(prompt_kv_store_kernel<float>, grid, blk, 0, st, qkv, static_cast<float*>(kplane), static_cast<float*>(vplane), S, H, T,
                           slots, 0, row_mul);
    else
        hipLaunchKernelGGL(prompt_kv_store_kernel<u16>, grid, blk, 0, st, qkv, static_cast<u16*>(kplane), static_cast<u16*>(vplane), S, H, T,
                           slots, f16, row_mul);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

int enqueue_beam_prompt(rgrg_decoder* d, const BeamPrompt& p, int S, int nb, bool* padded, std::vector<long long>* host_ids) {
    const int T = p.T, R = S * nb;
    hipStream_t st = d->stream;
    int rc;
    host_ids->resize((size_t)S * T);
    if ((rc = prompt_mask_check(d, "rgrg_decoder_beam_search_prompted", p.am, S, T, padded, host_ids->data(), p.ids,
                                (size_t)S * T * sizeof(long long))))
        return rc;
    if (!d->beam_pad && (rc = dmalloc(d, (void**)&d->beam_pad, (size_t)d->rows * sizeof(int), true))) return rc;
    if ((rc = tf_reserve(d, (size_t)S * T))) return rc;
    PromptCall c{p.ids, *padded ? p.am : nullptr, S, T};
    c.row_mul = nb;
    // (the id buffer rows the pass writes are not read: beam search keeps its histories on the host; the slot mask is per beam row)
    if ((rc = enqueue_prompt_pass(d, c, nullptr))) return rc;
    if ((rc = launch_beam_prompt_init(d->src_a, d->src_b, d->T, nb, R, T, c.am ? d->prompt_pad : (const int*)nullptr, d->beam_pad, st))) return rc;
    if (*padded && rgrg_decoder_kv_format_in_use(d, R) == KV_F32) return launch_beam_first_mask(d->beam_pad, R, d->T, d->key_mask, st);
    return RGRG_OK;
}

int enqueue_beam_row_pos(rgrg_decoder* d, int R) {
    return launch_beam_row_pos(d->step, d->beam_pad, d->row_pos, R, d->stream);
}

}  // namespace rgrg

extern "C" int rgrg_decoder_generate_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask,
                                              int S, int T, int max_length, int64_t* out_ids, int out_ld, int* out_len, int use_graph,
                                              void* stream) {
    RGRG_CHECK_ARG(d && feats && input_ids && out_ids && out_len && S > 0 && S <= d->max_seqs && T >= 1);
    int rc, limit;
    if ((rc = check_prompted(d, "rgrg_decoder_generate_prompted", S, T, max_length, false, out_ld, &limit))) return rc;
    if ((rc = decode_begin(d, stream))) return rc;
    if ((rc = prompted_decode_loop(d, "rgrg_decoder_generate_prompted", feats, input_ids, attention_mask, S, T, limit, STEP_ARGMAX, use_graph,
                                   out_ids, out_ld, nullptr, out_len)))
        return rc;
    d->logits_stale_rows = lm_head_cand_path(d, S) ? S : 0;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_beam_search_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask,
                                                 int S, int T, int num_beams, int max_length, int early_stopping, float length_penalty,
                                                 int num_return_sequences, int64_t* out_ids, int out_ld, int* out_len, void* stream) {
    RGRG_CHECK_ARG(d && feats && input_ids && out_ids && out_len && S > 0 && T >= 1 && num_beams > 1 && num_beams <= (1 << 14));
    RGRG_CHECK_ARG((long long)S * num_beams <= d->max_seqs);
    int rc, limit;
    if ((rc = check_prompted(d, "rgrg_decoder_beam_search_prompted", S * num_beams, T, max_length, true, out_ld, &limit))) return rc;
    const BeamPrompt p{reinterpret_cast<const long long*>(input_ids), attention_mask, T};
    return beam_search_run(d, feats, S, num_beams, limit, early_stopping, length_penalty, num_return_sequences, out_ids, out_ld, out_len,
                           stream, &p);
}

extern "C" int rgrg_decoder_group_beam_search_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask,
                                                       int S, int T, int num_beams, int num_beam_groups, float diversity_penalty, int max_length,
                                                       int early_stopping, float length_penalty, int num_return_sequences, int64_t* out_ids,
                                                       int out_ld, int* out_len, void* stream) {
    RGRG_CHECK_ARG(d && feats && input_ids && out_ids && out_len && S > 0 && T >= 1);
    int rc, limit;
    if ((rc = check_beam_groups("rgrg_decoder_group_beam_search_prompted", num_beams, num_beam_groups, diversity_penalty, num_return_sequences)))
        return rc;
    RGRG_CHECK_ARG((long long)S * num_beams <= d->max_seqs);
    if ((rc = check_prompted(d, "rgrg_decoder_group_beam_search_prompted", S * num_beams, T, max_length, true, out_ld, &limit))) return rc;
    const BeamPrompt p{reinterpret_cast<const long long*>(input_ids), attention_mask, T};
    const BeamGroups grp{num_beam_groups, num_beam_groups > 1 ? diversity_penalty : 0.f};
    return beam_search_run(d, feats, S, num_beams, limit, early_stopping, length_penalty, num_return_sequences, out_ids, out_ld, out_len,
                           stream, &p, &grp);
}

extern "C" int rgrg_decoder_beam_sample_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask,
                                                 int S, int T, int num_beams, int max_length, int early_stopping, float length_penalty,
                                                 int num_return_sequences, float temperature, int top_k, float top_p, uint64_t seed,
                                                 int64_t* out_ids, int out_ld, int* out_len, void* stream) {
    int rc, limit;
    if ((rc = check_beam_sample("rgrg_decoder_beam_sample_prompted", num_beams, num_return_sequences, temperature, top_k, top_p))) return rc;
    RGRG_CHECK_ARG(d && feats && input_ids && out_ids && out_len && S > 0 && T >= 1);
    RGRG_CHECK_ARG((long long)S * num_beams <= d->max_seqs);
    if ((rc = check_prompted(d, "rgrg_decoder_beam_sample_prompted", S * num_beams, T, max_length, true, out_ld, &limit))) return rc;
    const BeamPrompt p{reinterpret_cast<const long long*>(input_ids), attention_mask, T};
    const BeamSample smp{temperature, top_k, top_p, seed};
    return beam_search_run(d, feats, S, num_beams, limit, early_stopping, length_penalty, num_return_sequences, out_ids, out_ld, out_len,
                           stream, &p, nullptr, &smp);
}

extern "C" int rgrg_decoder_sample_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask, int S,
                                            int T, int max_length, float temperature, int top_k, float top_p, uint64_t seed,
                                            int64_t* out_ids, int out_ld, float* out_logprobs, int* out_len, int use_graph, void* stream) {
    RGRG_CHECK_ARG(d && feats && input_ids && out_ids && out_len && S > 0 && S <= d->max_seqs && T >= 1);
    int rc, limit;
    if ((rc = check_prompted(d, "rgrg_decoder_sample_prompted", S, T, max_length, false, out_ld, &limit))) return rc;
    if ((rc = sample_begin(d, S, temperature, top_k, top_p, seed, stream))) return rc;
    if ((rc = prompted_decode_loop(d, "rgrg_decoder_sample_prompted", feats, input_ids, attention_mask, S, T, limit, STEP_SAMPLE, use_graph,
                                   out_ids, out_ld, out_logprobs, out_len)))
        return rc;
    d->logits_stale_rows = 0;   // the head behind the prompt and every step wrote d->logits
    return RGRG_OK;
}

// Test hooks of the prompt kernels alone (tests/test_gpu_step_rows.py): the caller's device buffers, the given stream, the launchers
// the prompt pass itself goes through.  Every argument is validated before anything is launched.
extern "C" int rgrg_debug_prompt_mask_scan(const float* am, int S, int T, int* pad, int* flags, void* stream) {
    RGRG_CHECK_ARG(am && pad && flags && S >= 1 && T >= 1);
    return launch_prompt_mask_scan(am, S, T, pad, flags, as_stream(stream));
}

extern "C" int rgrg_debug_prompt_setup(const int64_t* in, int S, int T, int V, int64_t* ids, int ld_ids, int* step, const int* pad,
                                       int64_t* pos, float* kmask, int slots, void* stream) {
    RGRG_CHECK_ARG(in && ids && step && S >= 1 && T >= 1 && V >= 1 && ld_ids >= T);
    RGRG_CHECK_ARG(!pad || pos);             // positions are written whenever pad is given
    RGRG_CHECK_ARG(!kmask || pad);           // the slot mask is made from pad[]
    RGRG_CHECK_ARG(!kmask || slots >= T + 1);
    return launch_prompt_setup(reinterpret_cast<const long long*>(in), S, T, V, reinterpret_cast<long long*>(ids), ld_ids, step, pad,
                               reinterpret_cast<long long*>(pos), kmask, slots, as_stream(stream));
}

extern "C" int rgrg_debug_prompt_kv_store(const float* qkv, void* kplane, void* vplane, int S, int H, int T, int slots, int row_mul,
                                          int kv_bytes, int fp16, void* stream) {
    RGRG_CHECK_ARG(qkv && kplane && vplane && S >= 1 && H >= 1 && T >= 1 && slots >= T + 1 && row_mul >= 1);
    RGRG_CHECK_ARG(kv_bytes == 4 || kv_bytes == 2);   // the e4m3 cache takes no prompt
    RGRG_CHECK_ARG(kv_bytes == 2 || !fp16);
    return launch_prompt_kv_store(qkv, kplane, vplane, S, H, T, slots, row_mul, kv_bytes == 2, fp16 ? 1 : 0, as_stream(stream));
}

extern "C" int rgrg_debug_prompt_last_rows(const float* xn_all, int T, int D, float* xn, uint16_t* xn16, int fp16, int R, int row_div,
                                           void* stream) {
    RGRG_CHECK_ARG(xn_all && xn && T >= 1 && D == 1024 && R >= 1 && row_div >= 1);
    RGRG_CHECK_ARG(xn16 || !fp16);
    return launch_prompt_last_rows(xn_all, T, D, xn, xn16, fp16 ? 1 : 0, row_div, R, as_stream(stream));
}

extern "C" int rgrg_debug_prompt_step_rows(const int64_t* ids, int ld_ids, const int* step, const int* pad, int* tok, int* row_pos, int S,
                                           void* stream) {
    RGRG_CHECK_ARG(ids && step && pad && tok && row_pos && S >= 1 && ld_ids >= 1);
    return launch_prompt_step_rows(reinterpret_cast<const long long*>(ids), ld_ids, step, pad, tok, row_pos, S, as_stream(stream));
}

extern "C" int rgrg_debug_beam_prompt_init(int* src_a, int* src_b, int slots, int nb, int R, int T, const int* pad, int* beam_pad,
                                           void* stream) {
    RGRG_CHECK_ARG(src_a && src_b && beam_pad && nb >= 1 && R >= 1 && R % nb == 0 && T >= 1 && slots >= T + 1);
    return launch_beam_prompt_init(src_a, src_b, slots, nb, R, T, pad, beam_pad, as_stream(stream));
}

extern "C" int rgrg_debug_beam_row_pos(const int* step, const int* beam_pad, int* row_pos, int R, void* stream) {
    RGRG_CHECK_ARG(step && beam_pad && row_pos && R >= 1);
    return launch_beam_row_pos(step, beam_pad, row_pos, R, as_stream(stream));
}
