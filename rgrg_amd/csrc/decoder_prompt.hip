// Prompted greedy decode (rgrg_decoder_generate_prompted; LanguageModel.greedy_search with a prompt, language_model.py:609-652):
// the image slot as in rgrg_decoder_generate, then ONE teacher-forced pass over the S x T prompt rows (tf_hidden_pass,
// decoder_lm.hip) whose keys / values go to slots 1 .. T of the decode cache, lm_head + arg-max over the S last-position rows, and
// the decode loop of rgrg_decoder_generate from step T on.  A left-padded prompt keeps its padded slots out of every later step and
// embeds every row's tokens at the row's own position (prepare_inputs_for_generation, :498-520).
#include <algorithm>

#include "decoder_internal.h"

using namespace rgrg;

namespace rgrg {
namespace {

typedef unsigned short u16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

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
template <typename KV>   // float, or u16 in the 16-bit type f16
__global__ __launch_bounds__(256) void prompt_kv_store_kernel(const float* __restrict__ qkv, KV* __restrict__ kplane, KV* __restrict__ vplane,
                                                              int S, int H, int T, int slots, int f16) {
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
        KV* dst = (kv ? vplane : kplane) + (((size_t)s * H + hd) * slots + 1 + t) * 64 + e;
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

// ln_f row of every sequence's last prompt position -> row s of the decode step's lm_head input (fp32, and 16 bit where that step
// reads 16-bit activations): the lm_head runs on S rows, not S x T
__global__ __launch_bounds__(256) void prompt_last_rows_kernel(const float* __restrict__ xn_all, int T, int D, float* __restrict__ xn,
                                                               u16* __restrict__ xn16, int f16) {
    const int s = blockIdx.x, tid = threadIdx.x;   // D == 1024
    const f32x4 v = reinterpret_cast<const f32x4*>(xn_all + ((size_t)s * T + T - 1) * D)[tid];
    reinterpret_cast<f32x4*>(xn + (size_t)s * D)[tid] = v;
    if (xn16) store_16x4(xn16 + (size_t)s * D + 4 * tid, v, f16);
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

struct PromptCall {
    const long long* ids;
    const float* am;     // NULL unless the prompt is padded
    int S, T;
};

int store_prompt_kv(rgrg_decoder* d, int l, const float* qkv, const void* arg) {
    const PromptCall& c = *static_cast<const PromptCall*>(arg);
    const int S = c.S, fmt = rgrg_decoder_kv_format_in_use(d, S);
    const size_t total = (size_t)S * d->H * 2 * c.T * (fmt == KV_F32 ? 16 : 8);
    const dim3 grid((unsigned)std::min<size_t>((total + 255) / 256, 4096)), blk(256);
    if (fmt == KV_F32) {
        float* kc = d->kv + (size_t)l * d->kv_layer_stride;
        hipLaunchKernelGGL(prompt_kv_store_kernel<float>, grid, blk, 0, d->stream, qkv, kc, kc + d->kv_kv_stride, S, d->H, c.T, d->T, 0);
    } else {   // the 16-bit cache lives in the same allocation with the same element strides (enqueue_prefill)
        u16* kc = reinterpret_cast<u16*>(d->kv) + (size_t)l * d->kv_layer_stride;
        hipLaunchKernelGGL(prompt_kv_store_kernel<u16>, grid, blk, 0, d->stream, qkv, kc, kc + d->kv_kv_stride, S, d->H, c.T, d->T, d->f16());
    }
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// the prologue of run_decode_loop: everything between the image slot and step T
int enqueue_prompt(rgrg_decoder* d, int S, const void* arg) {
    const PromptCall& c = *static_cast<const PromptCall*>(arg);
    const int T = c.T, fmt = rgrg_decoder_kv_format_in_use(d, S);
    hipStream_t st = d->stream;
    int rc;
    const bool mask32 = c.am && fmt == KV_F32;   // the fp32 attention kernel takes the additive mask, the 16-bit one pad[] itself
    const int n = std::max(S * T, mask32 ? S * d->T : 0);
    hipLaunchKernelGGL(prompt_setup_kernel, dim3((n + 255) / 256), dim3(256), 0, st, c.ids, S, T, d->V, d->ids, d->max_len, d->step,
                       c.am ? d->prompt_pad : (const int*)nullptr, d->prompt_pos, mask32 ? d->key_mask : (float*)nullptr, d->T);
    RGRG_LAUNCH_CHECK();
    if ((rc = tf_hidden_pass(d, c.ids, c.am, c.am ? d->prompt_pos : nullptr, c.am ? S * T : 1, S, T, store_prompt_kv, arg))) return rc;
    u16* xn16 = (fmt != KV_F32 && d->xn16) ? d->xn16 : nullptr;
    hipLaunchKernelGGL(prompt_last_rows_kernel, dim3(S), dim3(256), 0, st, d->tf.xn, T, d->D, d->xn, xn16, d->f16());
    RGRG_LAUNCH_CHECK();
    return enqueue_head_argmax(d, S);
}

int greedy_step(rgrg_decoder* d, int S, bool count) { return enqueue_step(d, S, count); }

int padded_step(rgrg_decoder* d, int S, bool count) {
    hipLaunchKernelGGL(prompt_step_rows_kernel, dim3((S + 255) / 256), dim3(256), 0, d->stream, d->ids, d->max_len, d->step, d->prompt_pad,
                       d->beam_tok, d->row_pos, S);
    RGRG_LAUNCH_CHECK();
    const bool kv16 = rgrg_decoder_kv_format_in_use(d, S) != KV_F32;
    d->pos_override_cur = d->row_pos;
    if (kv16) d->kv_first_cur = d->prompt_pad;
    else d->key_mask_cur = d->key_mask;
    const int rc = enqueue_step(d, S, count, S <= rgrg_decoder_row_limit(d) ? d->beam_tok : nullptr);
    d->pos_override_cur = nullptr;
    d->kv_first_cur = nullptr;
    d->key_mask_cur = nullptr;
    return rc;
}

}  // namespace
}  // namespace rgrg

extern "C" int rgrg_decoder_generate_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask,
                                              int S, int T, int max_length, int64_t* out_ids, int out_ld, int* out_len, int use_graph,
                                              void* stream) {
    RGRG_CHECK_ARG(d && feats && input_ids && out_ids && out_len && S > 0 && S <= d->max_seqs && T >= 1);
    if (T + 1 > d->max_len) {
        set_error("rgrg_decoder_generate_prompted: a prompt of %d tokens and one generated token need %d token slots, the cache has %d",
                  T, T + 1, d->max_len);
        return RGRG_EINVAL;
    }
    // greedy_search (:622, :649): cur_len starts at T, one token is always produced, the loop ends at cur_len >= max_length
    int limit = (max_length > 0) ? max_length : d->max_len;
    if (limit < T + 1) limit = T + 1;
    RGRG_CHECK_ARG(limit <= d->max_len && out_ld >= limit);
    if (rgrg_decoder_kv_format_in_use(d, S) == KV_E4M3) {
        set_error("rgrg_decoder_generate_prompted: the e4m3 K/V cache takes no prompt: call rgrg_decoder_set_kv_format(d, 0) first");
        return RGRG_EINVAL;
    }
    int rc;
    if (!d->prompt_pad && (rc = dmalloc(d, (void**)&d->prompt_pad, (size_t)d->rows * sizeof(int), true))) return rc;
    if ((rc = decode_begin(d, stream))) return rc;
    bool padded = false;
    if (attention_mask) {   // one read-back per call: a mask the kernels cannot honour is refused before any work
        int* flags = d->next;   // a scratch word of the decoder
        RGRG_HIP(hipMemsetAsync(flags, 0, sizeof(int), d->stream));
        hipLaunchKernelGGL(prompt_mask_scan_kernel, dim3((S + 255) / 256), dim3(256), 0, d->stream, attention_mask, S, T, d->prompt_pad, flags);
        RGRG_LAUNCH_CHECK();
        RGRG_HIP(hipMemcpyAsync(d->h_done, flags, sizeof(int), hipMemcpyDeviceToHost, d->stream));
        RGRG_HIP(hipStreamSynchronize(d->stream));
        const int f = *d->h_done;
        if (f & (MASK_ROW_EMPTY | MASK_NOT_LEFT | MASK_NOT_BINARY)) {
            set_error("rgrg_decoder_generate_prompted: attention_mask %s", (f & MASK_ROW_EMPTY) ? "has a row of zeros only (no token to continue from)"
                      : (f & MASK_NOT_LEFT) ? "is not left padding (a zero behind a one): only padding in front of the prompt is supported"
                      : "holds values other than 0 and 1");
            return RGRG_EINVAL;
        }
        padded = (f & MASK_HAS_PAD) != 0;
    }
    if (padded) {
        if (!d->prompt_pos && (rc = dmalloc(d, (void**)&d->prompt_pos, (size_t)d->rows * d->max_len * sizeof(long long), true))) return rc;
        if (!d->key_mask && (rc = dmalloc(d, (void**)&d->key_mask, (size_t)d->rows * d->T * sizeof(float), true))) return rc;
    }
    if ((rc = tf_reserve(d, (size_t)S * T))) return rc;
    const PromptCall call{reinterpret_cast<const long long*>(input_ids), padded ? attention_mask : nullptr, S, T};
    const DecodePrologue pro{enqueue_prompt, &call, T};
    // a mask of ones leaves the steps of rgrg_decoder_generate (and their captured graph); a padded prompt has its own (key 4)
    if ((rc = run_decode_loop(d, feats, S, limit, padded ? 4 : 0, padded ? padded_step : greedy_step, use_graph, out_ids, out_ld, nullptr,
                              out_len, &pro)))
        return rc;
    d->logits_stale_rows = lm_head_cand_path(d, S) ? S : 0;
    return RGRG_OK;
}
