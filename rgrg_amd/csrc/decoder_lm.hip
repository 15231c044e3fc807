// Teacher-forced pass (LanguageModel.forward without a cache: logits / loss) and training pass (loss + the gradients of
// what the reference trains in the decoder) of the RGRG language model, over the rgrg_decoder object of decoder.hip.
// The backward kernels are in train_ops.hip / attn_train16.hip, the GEMMs in gemm_f32.hip / gemm_bf16.hip.
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "decoder_internal.h"

namespace rgrg {

// ------------------------------------------------------------------ teacher-forced pass (LanguageModel.forward, no cache)
// x[s,t] = wte[ids[s,t]] + wte[t] (position_ids default to arange(T) and are embedded with wte, language_model.py:298-307),
// xn = ln_1 of layer 0.  One workgroup per token row.
// Token ids are validated HERE (no host round trip before the launch): an id outside [0, V) is clamped, so nothing is
// read out of bounds, and raises the decoder's device-side error word; the loss of that pass comes out as NaN and the
// next decoder call reports the error (torch.nn.Embedding raises IndexError synchronously on the CPU / asserts on the GPU).
__global__ __launch_bounds__(256) void embed_seq_ln_kernel(const float* __restrict__ wte, const long long* __restrict__ ids,
                                                           int T, const float* __restrict__ g, const float* __restrict__ b,
                                                           float* __restrict__ x, float* __restrict__ xn, int D, int V,
                                                           int* __restrict__ id_error, const long long* __restrict__ pos_ids, int pos_rows) {
    __shared__ float sh[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    long long tok = ids[row];
    if (tok < 0 || tok >= V) {
        if (tid == 0) atomicOr(id_error, 1);
        tok = tok < 0 ? 0 : V - 1;
    }
    // position_ids (language_model.py:293-307): default arange(T); given ones ([S,T], or [1,T] broadcast over the sentences:
    // pos_rows = T) index the TOKEN table like the default ones do (the reference's wte[position_ids] quirk), so their range
    // is the vocabulary's and they are checked like the token ids
    long long pos = row % T;
    if (pos_ids) {
        pos = pos_ids[row % pos_rows];
        if (pos < 0 || pos >= V) {
            if (tid == 0) atomicOr(id_error, 1);
            pos = pos < 0 ? 0 : V - 1;
        }
    }
    const f32x4 v = reinterpret_cast<const f32x4*>(wte + (size_t)tok * D)[tid] + reinterpret_cast<const f32x4*>(wte + (size_t)pos * D)[tid];
    reinterpret_cast<f32x4*>(x + (size_t)row * D)[tid] = v;
    reinterpret_cast<f32x4*>(xn + (size_t)row * D)[tid] = ln_row(v, g, b, sh, D);
}
static int launch_embed_seq_ln(const float* wte, const long long* ids, int T, const float* g, const float* b, float* x, float* xn, int D, int V,
                               int* id_error, const long long* pos_ids, int pos_rows, int M, hipStream_t st) {
    hipLaunchKernelGGL(embed_seq_ln_kernel, dim3(M), dim3(256), 0, st, wte, ids, T, g, b, x, xn, D, V, id_error, pos_ids, pos_rows);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// GPT2PseudoAttention.forward without layer_past (:124-160) and _attn (:84-122) over T tokens: keys/values are
// [uk(img) ; k_0..k_{T-1}], scores / 8, future token columns replaced by -1e4 (the image column is never masked),
// plus the additive padding mask (1 - [1|attention_mask]) * -10000 (:325-334), softmax, . V.
//
// One WAVE per (sequence, head, 32-query tile), everything in registers on the exact-fp32 matrix core
// (v_mfma_f32_32x32x2_f32), no LDS:
//   * scores are computed TRANSPOSED, S^T = K Q^T (A = 32 keys x dims, B = dims x 32 queries; a lane half owns
//     dims [32h, 32h+32), so a lane reads 128 contiguous bytes of its key / query row).  In the accumulator layout a
//     lane then holds ONE query (column lane&31) and 16 keys per tile, half of that query's keys - the softmax row
//     reduction is a register loop plus one exchange with lane^32;
//   * that same layout is exactly the B operand (keys x queries) of O^T = V^T P^T: register j of a tile is fed to
//     the MFMA as is, next to A = V[key(j, lane half)][dim], a coalesced 128-byte row read.  No transpose.
// Key tiles entirely in the future of the query tile are skipped: their weights are exp(-1e4 - max) = 0 in fp32
// because the never-masked image column keeps max = O(1).  Keys beyond T (tile padding) get -inf.
constexpr int TF_MAX_T = 1023;  // T + 1 keys <= the 1024 positions of GPT-2's causal-mask buffer (the reference's limit)
template <int NT>  // key tiles held in registers: T + 1 <= 32 * NT
__global__ __launch_bounds__(256) void attn_prefill_kernel(const float* __restrict__ qkv, const float* __restrict__ ukv, int ld_ukv,
                                                           int kcol, const float* __restrict__ am, float* __restrict__ out,
                                                           int S, int H, int T, float* __restrict__ lse, const DropoutParams drop,
                                                           unsigned short* __restrict__ out16, int f16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int QT = (T + 31) / 32;
    const int item = blockIdx.x * 4 + wave;
    if (item >= S * H * QT) return;
    const int qt = item % QT, sh = item / QT, hd = sh % H, s = sh / H;
    const int NK = T + 1, D = H * 64;
    const int col = lane & 31, half = lane >> 5;
    const int iq = qt * 32 + col;                    // this lane's query (column of S^T)
    const int need = min(NK - 1, qt * 32 + 32) / 32 + 1;  // key tiles with a key <= last query of the tile + 1
    auto krow = [&](int c) -> const float* {         // K row of key c (c = 0: image key); V row = K row + D
        c = min(c, NK - 1);
        return c == 0 ? ukv + (size_t)s * ld_ukv + kcol + hd * 64 : qkv + ((size_t)s * T + c - 1) * 3 * D + D + hd * 64;
    };
    // B operand of S^T: this lane's query row, dims [32*half, 32*half + 32)
    f32x4 qf[8];
    {
        const float* qp = qkv + ((size_t)s * T + min(iq, T - 1)) * 3 * D + hd * 64 + half * 32;
#pragma unroll
        for (int u = 0; u < 8; ++u) qf[u] = *reinterpret_cast<const f32x4*>(qp + 4 * u);
    }
    f32x16 sc[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        if (kt < need) {
            f32x4 kf[8];
            const float* kp = krow(kt * 32 + col) + half * 32;   // A operand: key row kt*32 + (lane&31), same dims
#pragma unroll
            for (int u = 0; u < 8; ++u) kf[u] = *reinterpret_cast<const f32x4*>(kp + 4 * u);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][e], qf[u][e], acc, 0, 0, 0);
            sc[kt] = acc;
        }
    }
    // masks, scale, softmax over the keys of query iq (this lane: 16 keys per tile, lane^32 the other 16)
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        if (kt < need) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                float w = -INFINITY;
                if (c < NK) {
                    const bool allowed = (c == 0) || (c - 1 <= iq);
                    const float addm = (c == 0 || !am) ? 0.f : (1.0f - am[(size_t)s * T + c - 1]) * -10000.0f;
                    w = (allowed ? sc[kt][r] / 8.0f : -1e4f) + addm;
                }
                sc[kt][r] = w;
                m = fmaxf(m, w);
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        if (kt < need) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pexp = expf(sc[kt][r] - m);
                sc[kt][r] = pexp;
                sum += pexp;
            }
        }
    }
    sum += __shfl_xor(sum, 32, 64);
    if (lse && half == 0 && iq < T) lse[((size_t)s * T + iq) * H + hd] = m + logf(sum);  // kept for the backward pass
    // O^T = V^T P^T : A = V[key(j, half)][dim = lane&31 (+32)], B = register j of the tile
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        if (kt < need) {
            float v0[16], v1[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float* vp = krow(kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * half) + D;
                v0[j] = vp[col];
                v1[j] = vp[32 + col];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                float pj = sc[kt][j] / sum;
                if (drop.p > 0.f)  // attn_dropout on the probabilities (training pass); index = [s][head][query][key]
                    pj *= dropout_mask(drop, (((unsigned long long)s * H + hd) * T + min(iq, T - 1)) * dropout_key_pitch(NK) +
                                                 min(kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * half, NK - 1));
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[j], pj, o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[j], pj, o1, 0, 0, 0);
            }
        }
    }
    if (iq < T) {
        float* op = out + ((size_t)s * T + iq) * D + hd * 64;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dim = (r & 3) + 8 * (r >> 2) + 4 * half;
            op[dim] = o0[r];
            op[32 + dim] = o1[r];
        }
        if (out16) {   // 16-bit training flow: the copy attn_proj's GEMM reads (4 consecutive dims per 8-byte store)
            unsigned short* o16 = out16 + ((size_t)s * T + iq) * D + hd * 64 + 4 * half;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                store_16x4(o16 + 8 * q4, f32x4{o0[4 * q4], o0[4 * q4 + 1], o0[4 * q4 + 2], o0[4 * q4 + 3]}, f16);
                store_16x4(o16 + 32 + 8 * q4, f32x4{o1[4 * q4], o1[4 * q4 + 1], o1[4 * q4 + 2], o1[4 * q4 + 3]}, f16);
            }
        }
    }
}

// T + 1 > 256 keys (up to the reference's 1024 positions, language_model.py:60-67): the score tiles no longer fit in
// registers, so they are RECOMPUTED - pass 1 row max, pass 2 row sum, pass 3 probabilities x V - in the same tile and
// register order as attn_prefill_kernel, which makes the two kernels bit-identical where both apply (tested).  3x the
// score MFMAs of the register kernel; only long reports take this path.
__global__ __launch_bounds__(256) void attn_prefill_stream_kernel(const float* __restrict__ qkv, const float* __restrict__ ukv, int ld_ukv,
                                                                  int kcol, const float* __restrict__ am, float* __restrict__ out,
                                                                  int S, int H, int T, float* __restrict__ lse, const DropoutParams drop,
                                                                  unsigned short* __restrict__ out16, int f16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int QT = (T + 31) / 32;
    const int item = blockIdx.x * 4 + wave;
    if (item >= S * H * QT) return;
    const int qt = item % QT, sh = item / QT, hd = sh % H, s = sh / H;
    const int NK = T + 1, D = H * 64;
    const int col = lane & 31, half = lane >> 5;
    const int iq = qt * 32 + col;
    const int need = min(NK - 1, qt * 32 + 32) / 32 + 1;
    auto krow = [&](int c) -> const float* {
        c = min(c, NK - 1);
        return c == 0 ? ukv + (size_t)s * ld_ukv + kcol + hd * 64 : qkv + ((size_t)s * T + c - 1) * 3 * D + D + hd * 64;
    };
    f32x4 qf[8];
    {
        const float* qp = qkv + ((size_t)s * T + min(iq, T - 1)) * 3 * D + hd * 64 + half * 32;
#pragma unroll
        for (int u = 0; u < 8; ++u) qf[u] = *reinterpret_cast<const f32x4*>(qp + 4 * u);
    }
    // masked, scaled scores of key tile kt for this lane's query (16 keys: rows (r&3) + 8*(r>>2) + 4*half of the tile)
    auto tile_scores = [&](int kt) -> f32x16 {
        f32x4 kf[8];
        const float* kp = krow(kt * 32 + col) + half * 32;
#pragma unroll
        for (int u = 0; u < 8; ++u) kf[u] = *reinterpret_cast<const f32x4*>(kp + 4 * u);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][e], qf[u][e], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            float w = -INFINITY;
            if (c < NK) {
                const bool allowed = (c == 0) || (c - 1 <= iq);
                const float addm = (c == 0 || !am) ? 0.f : (1.0f - am[(size_t)s * T + c - 1]) * -10000.0f;
                w = (allowed ? acc[r] / 8.0f : -1e4f) + addm;
            }
            acc[r] = w;
        }
        return acc;
    };
    float m = -INFINITY;
    for (int kt = 0; kt < need; ++kt) {
        const f32x16 w = tile_scores(kt);
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaxf(m, w[r]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
    for (int kt = 0; kt < need; ++kt) {
        const f32x16 w = tile_scores(kt);
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += expf(w[r] - m);
    }
    sum += __shfl_xor(sum, 32, 64);
    if (lse && half == 0 && iq < T) lse[((size_t)s * T + iq) * H + hd] = m + logf(sum);
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    for (int kt = 0; kt < need; ++kt) {
        const f32x16 w = tile_scores(kt);
        float v0[16], v1[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float* vp = krow(kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * half) + D;
            v0[j] = vp[col];
            v1[j] = vp[32 + col];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float pj = expf(w[j] - m) / sum;
            if (drop.p > 0.f)
                pj *= dropout_mask(drop, (((unsigned long long)s * H + hd) * T + min(iq, T - 1)) * dropout_key_pitch(NK) +
                                             min(kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * half, NK - 1));
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[j], pj, o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[j], pj, o1, 0, 0, 0);
        }
    }
    if (iq < T) {
        float* op = out + ((size_t)s * T + iq) * D + hd * 64;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dim = (r & 3) + 8 * (r >> 2) + 4 * half;
            op[dim] = o0[r];
            op[32 + dim] = o1[r];
        }
        if (out16) {   // 16-bit training flow: the copy attn_proj's GEMM reads (4 consecutive dims per 8-byte store)
            unsigned short* o16 = out16 + ((size_t)s * T + iq) * D + hd * 64 + 4 * half;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                store_16x4(o16 + 8 * q4, f32x4{o0[4 * q4], o0[4 * q4 + 1], o0[4 * q4 + 2], o0[4 * q4 + 3]}, f16);
                store_16x4(o16 + 32 + 8 * q4, f32x4{o1[4 * q4], o1[4 * q4 + 1], o1[4 * q4 + 2], o1[4 * q4 + 3]}, f16);
            }
        }
    }
}

// RGRG_PREFILL_STREAM=1 forces the streaming kernel for every length (tests compare it with the register kernel)
static bool prefill_stream_forced() {
    static const bool v = [] { const char* e = getenv("RGRG_PREFILL_STREAM"); return e && atoi(e) != 0; }();
    return v;
}

// Which kernel the attention of a T-token teacher-forced pass runs on: 1 = attn_prefill_kernel<3>, 2 = <8>, 3 = streaming
static int attn_prefill_variant(int T) { return (T + 1 > 256 || prefill_stream_forced()) ? 3 : (T + 1 <= 96 ? 1 : 2); }

// variant 0: the rule above; 1 / 2 / 3 force a kernel (test hook) and fail when its key tiles cannot hold T + 1 keys
static int launch_attn_prefill(const float* qkv, const float* ukv, int ld_ukv, int kcol, const float* am, float* out, int S, int H,
                               int T, float* lse, const DropoutParams& drop, hipStream_t st, unsigned short* out16 = nullptr, int f16 = 0,
                               int variant = 0) {
    const int items = S * H * ((T + 31) / 32);
    const dim3 grid((items + 3) / 4), block(256);
    if (!variant) variant = attn_prefill_variant(T);
    if (T < 1 || T > TF_MAX_T || variant < 1 || variant > 3 || (variant == 1 && T + 1 > 96) || (variant == 2 && T + 1 > 256)) {
        set_error("attention of the teacher-forced pass: %d keys do not fit kernel variant %d", T + 1, variant);
        return RGRG_EINVAL;
    }
    if (variant == 3)
        hipLaunchKernelGGL(attn_prefill_stream_kernel, grid, block, 0, st, qkv, ukv, ld_ukv, kcol, am, out, S, H, T, lse, drop, out16, f16);
    else if (variant == 1)
        hipLaunchKernelGGL(attn_prefill_kernel<3>, grid, block, 0, st, qkv, ukv, ld_ukv, kcol, am, out, S, H, T, lse, drop, out16, f16);
    else
        hipLaunchKernelGGL(attn_prefill_kernel<8>, grid, block, 0, st, qkv, ukv, ld_ukv, kcol, am, out, S, H, T, lse, drop, out16, f16);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

// CrossEntropyLoss(ignore_index=-100) on the shifted logits/labels (:368-396): the row of token (s,t), t < T-1, is
// scored against ids[s][t+1] unless attention_mask[s][t+1] == 0.  One workgroup per logits row of the chunk.
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, size_t ld, int V, int row0,
                                                      const long long* __restrict__ ids, const float* __restrict__ am, int T,
                                                      float* __restrict__ row_loss, int* __restrict__ row_valid,
                                                      float* __restrict__ row_lse, int* __restrict__ id_error) {
    __shared__ float shv[4];
    const int r = row0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = r % T;
    const bool ignore = (t == T - 1) || (am && am[r + 1] == 0.f);
    if (ignore) {
        if (tid == 0) { row_loss[r] = 0.f; row_valid[r] = 0; }
        return;
    }
    const float* x = logits + (size_t)blockIdx.x * ld;
    float m = -INFINITY;
    for (int i = tid; i < V; i += 256) m = fmaxf(m, x[i]);
    m = wave_max(m);
    if (lane == 0) shv[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(shv[0], shv[1]), fmaxf(shv[2], shv[3]));
    __syncthreads();
    float sum = 0.f;
    for (int i = tid; i < V; i += 256) sum += expf(x[i] - m);
    sum = wave_sum(sum);
    if (lane == 0) shv[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        const float tot = (shv[0] + shv[1]) + (shv[2] + shv[3]);
        const float lse = m + logf(tot);
        // the label is a raw caller-supplied id: clamp it for the read (an id outside [0, V) would index outside the
        // logits row) and raise the error word - that pass's loss and gradients come out as NaN, the next call reports it
        long long label = ids[r + 1];
        if (label < 0 || label >= V) {
            atomicOr(id_error, 1);
            label = label < 0 ? 0 : V - 1;
        }
        row_loss[r] = lse - x[label];
        row_valid[r] = 1;
        if (row_lse) row_lse[r] = lse;
    }
}

// mean over the scored rows in a fixed order (double accumulation); no scored row -> nan, like torch
__global__ __launch_bounds__(256) void ce_finalize_kernel(const float* __restrict__ row_loss, const int* __restrict__ row_valid,
                                                          int n, float* __restrict__ loss, int* __restrict__ n_scored = nullptr,
                                                          const int* __restrict__ id_error = nullptr) {
    __shared__ double ssum[256];
    __shared__ int scnt[256];
    double a = 0.0;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += 256) { a += (double)row_loss[i]; c += row_valid[i]; }
    ssum[threadIdx.x] = a;
    scnt[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { ssum[threadIdx.x] += ssum[threadIdx.x + o]; scnt[threadIdx.x] += scnt[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (loss) *loss = (id_error && *id_error) ? nanf("") : (float)(ssum[0] / (double)scnt[0]);  // invalid token id: poisoned
        if (n_scored) *n_scored = scnt[0];
    }
}

// row_valid of every token row from the ids/mask alone (the scored-row count is needed before the first chunk's backward)
__global__ __launch_bounds__(256) void ce_valid_kernel(const float* __restrict__ am, int T, int n, float* __restrict__ row_loss,
                                                       int* __restrict__ row_valid) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
        const int t = r % T;
        row_valid[r] = !((t == T - 1) || (am && am[r + 1] == 0.f));
        row_loss[r] = 0.f;
    }
}

// Launchers of the three cross-entropy kernels: the passes below and the test hooks at the end of this file share the grid rules.
static int launch_ce_valid(const float* am, int T, int M, float* row_loss, int* row_valid, hipStream_t st) {
    hipLaunchKernelGGL(ce_valid_kernel, dim3((M + 255) / 256), dim3(256), 0, st, am, T, M, row_loss, row_valid);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
// rows [row0, row0 + rows) of the M = S * T token rows; `logits` points at the chunk's first row
static int launch_ce_rows(const float* logits, size_t ld, int V, int row0, int rows, const long long* ids, const float* am, int T,
                          float* row_loss, int* row_valid, float* row_lse, int* id_error, hipStream_t st) {
    hipLaunchKernelGGL(ce_rows_kernel, dim3(rows), dim3(256), 0, st, logits, ld, V, row0, ids, am, T, row_loss, row_valid, row_lse, id_error);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}
static int launch_ce_finalize(const float* row_loss, const int* row_valid, int n, float* loss, int* n_scored, const int* id_error,
                              hipStream_t st) {
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, st, row_loss, row_valid, n, loss, n_scored, id_error);
    RGRG_LAUNCH_CHECK();
    return RGRG_OK;
}

}  // namespace rgrg

using namespace rgrg;

// ------------------------------------------------------------------ teacher-forced pass (host side)
namespace rgrg {
// A previous teacher-forced pass saw a token id outside [0, vocab): report it now (its loss was NaN), clear the flag
static int check_id_error(rgrg_decoder* d) {
    if (d->h_id_error && *d->h_id_error) {
        *d->h_id_error = 0;
        (void)hipMemsetAsync(d->id_error, 0, 2 * sizeof(int), d->stream);
        set_error("index out of range in self: a token id of a previous teacher-forced pass was outside [0, %d)", d->V);
        return RGRG_EINVAL;
    }
    return RGRG_OK;
}
__global__ void id_error_fold_kernel(int* __restrict__ e) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && e[0]) e[1] = 1;
}
// start of a pass (on the decoder stream, after the wait for the caller): this pass's error word starts clean
static int id_error_begin(rgrg_decoder* d) {
    RGRG_HIP(hipMemsetAsync(d->id_error, 0, sizeof(int), d->stream));
    return RGRG_OK;
}
// end of a pass: fold this pass's word into the sticky one and mirror the sticky word to the host (asynchronously)
static int id_error_end(rgrg_decoder* d) {
    hipLaunchKernelGGL(id_error_fold_kernel, dim3(1), dim3(64), 0, d->stream, d->id_error);
    RGRG_LAUNCH_CHECK();
    RGRG_HIP(hipMemcpyAsync(d->h_id_error, d->id_error + 1, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    return RGRG_OK;
}
constexpr int TF_LOGIT_ROWS = 2048;  // lm_head + cross entropy run over chunks of this many token rows (412 MB of logits)

int tf_reserve(rgrg_decoder* d, size_t rows) {
    if (rows <= d->tf.rows) return RGRG_OK;
    d->tf.free();
    const size_t D = (size_t)d->D;
    const size_t chunk = rows < (size_t)TF_LOGIT_ROWS ? rows : (size_t)TF_LOGIT_ROWS;
    d->tf.ws_floats = 4 * rows * D;  // split-K partials of the narrow (N = 1024) GEMMs when there are few row tiles
    RGRG_HIP(hipMalloc((void**)&d->tf.x, rows * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tf.xn, rows * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tf.qkv, rows * 3 * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tf.att, rows * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tf.ff, rows * 4 * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tf.logits, chunk * (size_t)d->V * 4));
    RGRG_HIP(hipMalloc((void**)&d->tf.ws, d->tf.ws_floats * 4));
    RGRG_HIP(hipMalloc((void**)&d->tf.row_loss, rows * 4));
    RGRG_HIP(hipMalloc((void**)&d->tf.row_valid, rows * 4));
    d->tf.rows = rows;
    return RGRG_OK;
}

// tiled GEMM for the M = S*T token rows (never the skinny path: its buffers are sized for decode rows)
// bf16-weight GEMM of the teacher-forced / training passes on an fp32 activation matrix: X is rounded to bf16 ONCE into a
// scratch buffer (the same round-to-nearest-even the register-staged kernel applied tile by tile, so the operands are
// identical) and the product runs on the LDS-DMA kernel - at M = S x T token rows it reaches 2-3x the register-staged rate.
static int a16_reserve(rgrg_decoder* d, size_t need) {
    if (need > d->tr.a16_bytes) {
        RGRG_HIP(hipStreamSynchronize(d->stream));  // the old buffer may still be read by a queued GEMM
        if (d->tr.a16_scratch) (void)hipFree(d->tr.a16_scratch);
        d->tr.a16_scratch = nullptr; d->tr.a16_bytes = 0;
        RGRG_HIP(hipMalloc(&d->tr.a16_scratch, need));
        d->tr.a16_bytes = need;
    }
    return RGRG_OK;
}
int tf_reserve_a16(rgrg_decoder* d, size_t rows) { return a16_reserve(d, rows * 4 * (size_t)d->D * sizeof(unsigned short)); }   // (c_fc's output is the widest input)

static int bf16_linear_f32in(rgrg_decoder* d, const float* X, const void* Wb, const float* b, const float* R, float* Y, int M, int N,
                             int K, int ldy, int act) {
    int rc = a16_reserve(d, (size_t)M * K * sizeof(unsigned short));
    if (rc) return rc;
    rc = convert_f32_to_bf16(X, d->tr.a16_scratch, (size_t)M * K, d->stream, d->f16());
    if (rc) return rc;
    return launch_gemm_bf16w_ex(nullptr, d->tr.a16_scratch, Wb, b, R, Y, nullptr, M, N, K, ldy, act, d->stream, d->f16());
}

static int tf_linear(rgrg_decoder* d, const Lin& l, const float* X, const float* R, float* Y, int M, int ldy, int act, bool no_splitk = false) {
    if (d->bf16_gemms && l.wb && l.K % 256 == 0 && M > skinny_max_rows())
        return bf16_linear_f32in(d, X, l.wb, l.b, R, Y, M, l.N, l.K, ldy, act);
    return launch_gemm_dense(X, l.w, l.b, R, Y, M, l.N, l.K, ldy, act, d->tf.ws, no_splitk ? 0 : d->tf.ws_floats, d->stream);
}
int tf_hidden_pass(rgrg_decoder* d, const long long* ids, const float* attention_mask, const long long* pos, int pos_rows, int S, int T,
                   int (*after_qkv)(rgrg_decoder*, int, const float*, const void*), const void* arg, const float* ukv, bool kv_only) {
    const int D = d->D, M = S * T;
    if (!ukv) ukv = d->ukv_out;
    hipStream_t st = d->stream;
    int rc;
    if ((rc = launch_embed_seq_ln(d->wte, ids, T, d->layers[0].ln1_g, d->layers[0].ln1_b, d->tf.x, d->tf.xn, D, d->V, d->id_error, pos,
                                  pos_rows, M, st)))
        return rc;
    for (int l = 0; l < d->n_layer; ++l) {
        const LayerW& w = d->layers[l];
        const float* ng = (l + 1 < d->n_layer) ? d->layers[l + 1].ln1_g : d->lnf_g;
        const float* nb = (l + 1 < d->n_layer) ? d->layers[l + 1].ln1_b : d->lnf_b;
        if ((rc = tf_linear(d, w.c_attn, d->tf.xn, nullptr, d->tf.qkv, M, 3 * D, RGRG_ACT_NONE, kv_only))) return rc;
        if (after_qkv && (rc = after_qkv(d, l, d->tf.qkv, arg))) return rc;
        if (kv_only && l + 1 == d->n_layer) return RGRG_OK;   // nothing reads what the last layer does with its q | k | v
        if ((rc = launch_attn_prefill(d->tf.qkv, ukv, d->ld_ukv, l * 2 * D, attention_mask, d->tf.att, S, d->H, T, nullptr,
                                      DropoutParams{0ull, 0u, 0.f}, st)))
            return rc;
        if ((rc = tf_linear(d, w.attn_proj, d->tf.att, d->tf.x, d->tf.x, M, D, RGRG_ACT_NONE, kv_only))) return rc;
        if ((rc = launch_ln_rows(d->tf.x, w.ln2_g, w.ln2_b, d->tf.xn, D, nullptr, 0, M, st))) return rc;
        if ((rc = tf_linear(d, w.c_fc, d->tf.xn, nullptr, d->tf.ff, M, 4 * D, RGRG_ACT_GELU_NEW, kv_only))) return rc;
        if ((rc = tf_linear(d, w.mlp_proj, d->tf.ff, d->tf.x, d->tf.x, M, D, RGRG_ACT_NONE, kv_only))) return rc;
        if ((rc = launch_ln_rows(d->tf.x, ng, nb, d->tf.xn, D, nullptr, 0, M, st))) return rc;
    }
    return RGRG_OK;
}
}  // namespace rgrg

// position_ids of the teacher-forced passes (language_model.py:293-307): `pos` = int64 device array of S * T entries (per sentence)
// or T entries (one row, broadcast), read by the NEXT rgrg_decoder_lm_forward / rgrg_decoder_lm_loss_grad call of that shape and
// dropped by it; NULL = the default arange(T).  Like the token ids they index the token table (the reference's
// wte[position_ids]) and are range-checked on the device.
extern "C" int rgrg_decoder_set_lm_positions(rgrg_decoder* d, const int64_t* pos, int64_t n) {
    RGRG_CHECK_ARG(d && (pos == nullptr || n > 0));
    d->tf.pos = reinterpret_cast<const long long*>(pos);
    d->tf.pos_rows = pos ? (int)n : 1;
    return RGRG_OK;
}

extern "C" int rgrg_decoder_lm_forward(rgrg_decoder* d, const float* feats, const int64_t* input_ids,
                                       const float* attention_mask, int S, int T, float* logits_out, float* loss_out,
                                       void* stream) {
    RGRG_CHECK_ARG(d && feats && input_ids && S > 0 && S <= d->max_seqs && T >= 1 && T <= TF_MAX_T && (logits_out || loss_out));
    RGRG_CHECK_ARG(!loss_out || T >= 2);
    RGRG_CHECK_ARG(!d->tf.pos || d->tf.pos_rows == T || d->tf.pos_rows == S * T);   // rgrg_decoder_set_lm_positions: [T] or [S * T]
    const int D = d->D, M = S * T;
    int rc = check_id_error(d);
    if (rc) return rc;
    if ((rc = tf_reserve(d, (size_t)M))) return rc;
    hipStream_t caller = as_stream(stream), st = d->stream;
    RGRG_HIP(hipEventRecord(d->ev_in, caller));
    RGRG_HIP(hipStreamWaitEvent(st, d->ev_in, 0));
    if ((rc = id_error_begin(d))) return rc;
    // feature_space_transformation_nn (:284), then uk / uv of every layer in one GEMM (:145-150)
    RGRG_HIP(hipMemcpyAsync(d->feats, feats, (size_t)S * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    if ((rc = linear(d, d->fst0, d->feats, nullptr, d->h1, S, D, RGRG_ACT_RELU, false))) return rc;
    if ((rc = linear(d, d->fst2, d->h1, nullptr, d->img, S, D, RGRG_ACT_NONE, false))) return rc;
    if ((rc = linear(d, d->ukv, d->img, nullptr, d->ukv_out, S, d->ld_ukv, RGRG_ACT_NONE, false))) return rc;
    const long long* ids = reinterpret_cast<const long long*>(input_ids);
    rc = tf_hidden_pass(d, ids, attention_mask, d->tf.pos, d->tf.pos_rows, S, T);
    d->tf.pos = nullptr; d->tf.pos_rows = 1;   // consumed (rgrg_decoder_set_lm_positions)
    if (rc) return rc;
    // lm_head (tied to wte, no bias) and the loss, over chunks of token rows
    for (int r0 = 0; r0 < M; r0 += TF_LOGIT_ROWS) {
        const int rows = (M - r0 < TF_LOGIT_ROWS) ? M - r0 : TF_LOGIT_ROWS;
        float* lg = logits_out ? logits_out + (size_t)r0 * d->V : d->tf.logits;
        if ((rc = tf_linear(d, d->lm_head, d->tf.xn + (size_t)r0 * D, nullptr, lg, rows, d->V, RGRG_ACT_NONE))) return rc;
        if (loss_out && (rc = launch_ce_rows(lg, (size_t)d->V, d->V, r0, rows, ids, attention_mask, T, d->tf.row_loss, d->tf.row_valid,
                                             nullptr, d->id_error, st)))
            return rc;
    }
    if (loss_out && (rc = launch_ce_finalize(d->tf.row_loss, d->tf.row_valid, M, loss_out, nullptr, d->id_error, st))) return rc;
    if ((rc = id_error_end(d))) return rc;
    // the caller's stream continues after this pass (no host synchronisation)
    RGRG_HIP(hipEventRecord(d->ev_in, st));
    RGRG_HIP(hipStreamWaitEvent(caller, d->ev_in, 0));
    return RGRG_OK;
}

// ------------------------------------------------------------------ training pass: loss + gradients (host side)
namespace rgrg {
static int pad32(int n) { return (n + 31) / 32 * 32; }

// transposed copies of the frozen weights the activation gradients flow through (made once)
static int make_wT(rgrg_decoder* d, Lin& l) {
    const int Np = pad256(l.N);
    int rc;
    if (!l.wT) {
        if ((rc = dmalloc(d, (void**)&l.wT, (size_t)l.K * Np * sizeof(float), false))) return rc;
        if ((rc = launch_transpose_pad(l.w, l.wT, l.N, l.K, Np, d->stream))) return rc;
    }
    if (d->bf16_gemms && (!l.wTb || l.wTb_f16 != d->f16())) {   // (re)made in the current 16-bit type
        if (!l.wTb && (rc = dmalloc(d, &l.wTb, (size_t)l.K * Np * 2, false))) return rc;
        if ((rc = convert_f32_to_bf16(l.wT, l.wTb, (size_t)l.K * Np, d->stream, d->f16()))) return rc;
        l.wTb_f16 = d->f16();
    }
    return RGRG_OK;
}

static int ensure_wT(rgrg_decoder* d) {
    if (d->tr.have_wT && (!d->bf16_gemms || (d->layers[0].c_attn.wTb && d->layers[0].c_attn.wTb_f16 == d->f16()))) return RGRG_OK;
    int rc;
    if ((rc = make_wT(d, d->lm_head)) || (rc = make_wT(d, d->ukv)) || (rc = make_wT(d, d->fst2))) return rc;
    for (auto& w : d->layers)
        if ((rc = make_wT(d, w.c_attn)) || (rc = make_wT(d, w.attn_proj)) || (rc = make_wT(d, w.c_fc)) || (rc = make_wT(d, w.mlp_proj)))
            return rc;
    d->tr.have_wT = true;
    return RGRG_OK;
}

// The 16-bit flow runs lm_head + cross entropy over up to 16 384 token rows at a time (a configs[4] step = 14 848 rows in ONE
// chunk: 3.3 GB of fp32 logits + 1.65 GB of 16-bit d(logits), 116 x 394 tiles per GEMM instead of eight launches of 16 x 394)
constexpr int TR_LOGIT_ROWS_H16 = 16384;

static int tr_reserve(rgrg_decoder* d, size_t rows, size_t seqs, bool h16, bool a16) {
    // The work space holds the buffers of EVERY mode seen so far (16-bit / fp32 activation flow x 16-bit / fp32 attention): a16
    // follows T + 1 <= 128 and h16 follows S * T > 128, so batches whose padded length moves across those edges flip the mode
    // back and forth - freeing and re-allocating multi-GB buffers (plus a 1.6 GB memset) on every flip.  A mode
    // that is new to this decoder costs one re-allocation; after that only a larger batch does.
    bool& seen_a = a16 ? d->tr.seen_a16 : d->tr.seen_a32;
    bool& seen_h = h16 ? d->tr.seen_h16 : d->tr.seen_h32;
    const size_t cap = h16 ? (size_t)TR_LOGIT_ROWS_H16 : (size_t)TF_LOGIT_ROWS;
    if (rows <= d->tr.rows && seqs <= d->tr.seqs && seen_a && seen_h && (!h16 || a16 || d->tr.seen_h16_a32 || d->tr.seen_a16)) {
        d->tr.h16 = h16; d->tr.a16 = a16;
        d->tr.chunk = d->tr.rows < cap ? d->tr.rows : cap;
        return RGRG_OK;
    }
    const size_t keep = d->tr.rows, keep_s = d->tr.seqs;
    d->tr.free();
    seen_a = true; seen_h = true;
    if (h16 && !a16) d->tr.seen_h16_a32 = true;
    rows = rows > keep ? rows : keep;
    seqs = seqs > keep_s ? seqs : keep_s;
    const size_t D = (size_t)d->D, L = (size_t)d->n_layer, Sp = (size_t)pad32((int)seqs), VP = (size_t)pad256(d->V);
    const size_t cap_all = d->tr.seen_h16 ? (size_t)TR_LOGIT_ROWS_H16 : (size_t)TF_LOGIT_ROWS;   // the larger chunk of the modes seen
    const size_t chunk = rows < cap_all ? rows : cap_all;
    d->tr.h16 = h16;
    d->tr.a16 = a16;
    d->tr.chunk = rows < cap ? rows : cap;
    RGRG_HIP(hipMalloc((void**)&d->tr.xs, (2 * L + 1) * rows * D * 4));
    if (d->tr.seen_a16) {
        RGRG_HIP(hipMalloc((void**)&d->tr.qkv16, L * rows * 3 * D * 2));
        RGRG_HIP(hipMalloc((void**)&d->tr.att16, L * rows * D * 2));   // (the fp32-attention 16-bit flow uses its first rows x D)
        RGRG_HIP(hipMalloc((void**)&d->tr.datt16, rows * D * 2));
        RGRG_HIP(hipMalloc((void**)&d->tr.ukv16, seqs * (size_t)d->ld_ukv * 2));
    }
    if (d->tr.seen_a32) {
        RGRG_HIP(hipMalloc((void**)&d->tr.qkv, L * rows * 3 * D * 4));
        RGRG_HIP(hipMalloc((void**)&d->tr.att, L * rows * D * 4));
        RGRG_HIP(hipMalloc((void**)&d->tr.delta, rows * (size_t)d->H * 4));
        if (d->tr.seen_h16_a32 && !d->tr.seen_a16) RGRG_HIP(hipMalloc((void**)&d->tr.att16, rows * D * 2));
    }
    if (d->tr.seen_h16) {
        RGRG_HIP(hipMalloc((void**)&d->tr.xn16, rows * D * 2));
        RGRG_HIP(hipMalloc((void**)&d->tr.ff16, rows * 4 * D * 2));
        RGRG_HIP(hipMalloc((void**)&d->tr.ffpre16, L * rows * 4 * D * 2));
        RGRG_HIP(hipMalloc((void**)&d->tr.dx16, rows * D * 2));
        RGRG_HIP(hipMalloc((void**)&d->tr.dff16, rows * 4 * D * 2));
        RGRG_HIP(hipMalloc((void**)&d->tr.dqkv16, rows * 3 * D * 2));
        RGRG_HIP(hipMalloc((void**)&d->tr.dl16, chunk * VP * 2));
        RGRG_HIP(hipMemset(d->tr.dl16, 0, chunk * VP * 2));   // the K-padding columns stay 0 for the backward GEMM
    }
    if (d->tr.seen_h32) {
        RGRG_HIP(hipMalloc((void**)&d->tr.ffpre, L * rows * 4 * D * 4));
        RGRG_HIP(hipMalloc((void**)&d->tr.ff, rows * 4 * D * 4));
    }
    RGRG_HIP(hipMalloc((void**)&d->tr.dx, rows * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.dbig, rows * 4 * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.dxn, rows * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.logits, chunk * VP * 4));
    RGRG_HIP(hipMemset(d->tr.logits, 0, chunk * VP * 4));  // the K-padding columns stay 0 for the backward GEMM
    RGRG_HIP(hipMalloc((void**)&d->tr.dukv, seqs * (size_t)d->ld_ukv * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.t1, (size_t)d->ld_ukv * Sp * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.t2, D * Sp * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.dimg, seqs * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.dh1, seqs * D * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.row_lse, rows * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.lse, L * rows * (size_t)d->H * 4));
    RGRG_HIP(hipMalloc((void**)&d->tr.count, 4));
    d->tr.rows = rows;
    d->tr.seqs = seqs;
    return RGRG_OK;
}

// Y = X W^T (+R) on the fp32 tiled GEMM with the teacher-forced pass's split-K work space
static int tr_gemm(rgrg_decoder* d, const float* X, const float* W, const float* b, const float* R, float* Y, int M, int N, int K,
                   int ldy, int act = RGRG_ACT_NONE) {
    return launch_gemm_dense(X, W, b, R, Y, M, N, K, ldy, act, d->tf.ws, d->tf.ws_floats, d->stream);
}
// frozen-weight GEMM of the training pass: forward (Y = X W^T + b) or activation gradient (Y = X W, on the transposed
// copy); bf16 MFMA when the decoder is in bf16 mode (torch.autocast) and there are more than 128 token rows
static int tr_lin(rgrg_decoder* d, const Lin& l, bool transposed, const float* X, const float* R, float* Y, int M, int ldy,
                  int act = RGRG_ACT_NONE) {
    const int N = transposed ? l.K : l.N, K = transposed ? pad256(l.N) : l.K;
    const float* W = transposed ? l.wT : l.w;
    const void* Wb = transposed ? l.wTb : l.wb;
    const float* b = transposed ? nullptr : l.b;
    if (d->bf16_gemms && Wb && K % 256 == 0 && M > skinny_max_rows())
        return bf16_linear_f32in(d, X, Wb, b, R, Y, M, N, K, ldy, act);
    return launch_gemm_dense(X, W, b, R, Y, M, N, K, ldy, act, d->tf.ws, d->tf.ws_floats, d->stream);
}
// the same on 16-bit activations that their producer wrote (16-bit flow): no conversion pass, optional 16-bit output and the
// training epilogues (GemmLnFold::Ypre16 / G16)
static int tr_lin16(rgrg_decoder* d, const Lin& l, bool transposed, const unsigned short* A16, const float* R, float* Y,
                    unsigned short* Y16, int M, int ldy, int act = RGRG_ACT_NONE, const GemmLnFold* ex = nullptr) {
    const int N = transposed ? l.K : l.N, K = transposed ? pad256(l.N) : l.K;
    const void* Wb = transposed ? l.wTb : l.wb;
    if (!Wb || K % 256 != 0) { set_error("decoder: 16-bit weights missing for a training GEMM (N %d, K %d)", N, K); return RGRG_EINVAL; }
    return launch_gemm_bf16w_ex(nullptr, A16, Wb, transposed ? nullptr : l.b, R, Y, Y16, M, N, K, ldy, act, d->stream, d->f16(), ex);
}

// Forward (keeping what the backward needs), lm_head + loss + d(logits), and the backward through the 24 frozen blocks of
// rgrg_decoder_lm_loss_grad in the 16-bit activation flow (tr.h16).  Per layer, forward: c_attn (xn16 -> qkv fp32) ->
// attention (-> att fp32 + att16) -> attn_proj (-> y) -> x_mid = x_in + dropout(y), xn16 = ln_2(x_mid) [one kernel] ->
// c_fc (-> ffpre16 kept + ff16 = gelu) -> mlp_proj (-> y) -> x_out = x_mid + dropout(y), xn16 = next LayerNorm [one kernel].
// Backward: mlp_proj^T with the gelu' epilogue (dx16 -> dff16) -> c_fc^T (-> dxn) -> ln_2 backward (dx +=, dx16 = masked copy)
// -> attn_proj^T (-> d_att) -> attention backward (-> dqkv16, d_ukv) -> c_attn^T (-> dxn) -> ln_1 backward.
// fp16: gradients carry an internal scale of 2^15 from d(logits) to d_ukv (where the attention backward removes it), like
// the reference's GradScaler keeps fp16 gradients out of the flush-to-zero range (train_full_model.py:172-237).
static int tr_body16(rgrg_decoder* d, const long long* ids, const float* attention_mask, int S, int T, float loss_scale,
                     float dropout_p, uint64_t dropout_seed, float* loss_out) {
    const int D = d->D, M = S * T, L = d->n_layer, V = d->V, VP = pad256(V), LD = d->ld_ukv, f16 = d->f16();
    hipStream_t st = d->stream;
    const size_t MD = (size_t)M * D;
    int rc;
    auto xs = [&](int i) { return d->tr.xs + (size_t)i * MD; };
    auto dp = [&](int l, int site) { return DropoutParams{dropout_seed, (unsigned)(l * 4 + site), dropout_p}; };
    const DropoutParams none{0ull, 0u, 0.f};
    const float s_int = f16 ? 32768.0f : 1.0f;
    // [M, D] 16-bit scratch for a projection's output in front of the residual / dropout / LayerNorm kernel (forward: the
    // buffer of the masked gradient, unused until the backward) and for d(LayerNorm output) in front of the LayerNorm-backward
    // kernel (backward: the buffer of the LayerNorm outputs, unused after the forward).  16 bit like every GEMM output of the
    // reference under autocast: half the store tail of the K = 1024 GEMMs, whose 256 KiB tiles leave through the HBM write path.
    unsigned short* y16 = d->tr.dx16;
    unsigned short* dy16 = d->tr.xn16;
    const bool a16 = d->tr.a16;
    if (a16 && (rc = convert_f32_to_bf16(d->ukv_out, d->tr.ukv16, (size_t)S * LD, st, f16))) return rc;

    if ((rc = launch_embed_seq_ln(d->wte, ids, T, d->layers[0].ln1_g, d->layers[0].ln1_b, xs(0), d->tf.xn, D, d->V, d->id_error, d->tf.pos,
                                  d->tf.pos_rows, M, st)))
        return rc;
    d->tf.pos = nullptr; d->tf.pos_rows = 1;   // consumed (rgrg_decoder_set_lm_positions)
    // self.drop on the embeddings (language_model.py:311) and ln_1 of layer 0 as 16 bit
    if ((rc = launch_resid_dropout_ln16(xs(0), nullptr, nullptr, xs(0), d->layers[0].ln1_g, d->layers[0].ln1_b, d->tr.xn16, dp(0, 0), f16, M, D, st)))
        return rc;
    for (int l = 0; l < L; ++l) {
        const LayerW& w = d->layers[l];
        const float* ng = (l + 1 < L) ? d->layers[l + 1].ln1_g : d->lnf_g;
        const float* nb = (l + 1 < L) ? d->layers[l + 1].ln1_b : d->lnf_b;
        float* qkv = a16 ? nullptr : d->tr.qkv + (size_t)l * M * 3 * D;
        unsigned short* ffpre16 = d->tr.ffpre16 + (size_t)l * M * 4 * D;
        float* att = a16 ? nullptr : d->tr.att + (size_t)l * MD;
        float* lse = d->tr.lse + (size_t)l * M * d->H;
        if (a16) {
            unsigned short* qkv16 = d->tr.qkv16 + (size_t)l * M * 3 * D;
            unsigned short* att16 = d->tr.att16 + (size_t)l * MD;
            if ((rc = tr_lin16(d, w.c_attn, false, d->tr.xn16, nullptr, nullptr, qkv16, M, 3 * D))) return rc;
            if ((rc = launch_attn16_forward(qkv16, d->tr.ukv16, LD, l * 2 * D, attention_mask, att16, lse, S, d->H, T, dp(l, 1), f16, st)))
                return rc;
            if ((rc = tr_lin16(d, w.attn_proj, false, att16, nullptr, nullptr, y16, M, D))) return rc;
        } else {
            if ((rc = tr_lin16(d, w.c_attn, false, d->tr.xn16, nullptr, qkv, nullptr, M, 3 * D))) return rc;
            if ((rc = launch_attn_prefill(qkv, d->ukv_out, LD, l * 2 * D, attention_mask, att, S, d->H, T, lse, dp(l, 1), st, d->tr.att16, f16)))
                return rc;
            if ((rc = tr_lin16(d, w.attn_proj, false, d->tr.att16, nullptr, nullptr, y16, M, D))) return rc;
        }
        if ((rc = launch_resid_dropout_ln16(nullptr, y16, xs(2 * l), xs(2 * l + 1), w.ln2_g, w.ln2_b, d->tr.xn16, dp(l, 2), f16, M, D, st))) return rc;
        GemmLnFold pre{};
        pre.Ypre16 = ffpre16;
        if ((rc = tr_lin16(d, w.c_fc, false, d->tr.xn16, nullptr, nullptr, d->tr.ff16, M, 4 * D, RGRG_ACT_GELU_NEW, &pre))) return rc;
        if ((rc = tr_lin16(d, w.mlp_proj, false, d->tr.ff16, nullptr, nullptr, y16, M, D))) return rc;
        if ((rc = launch_resid_dropout_ln16(nullptr, y16, xs(2 * l + 1), xs(2 * l + 2), ng, nb, d->tr.xn16, dp(l, 3), f16, M, D, st))) return rc;
    }
    // lm_head + loss + d(logits) + d(ln_f output), chunk by chunk
    if ((rc = launch_ce_valid(attention_mask, T, M, d->tf.row_loss, d->tf.row_valid, st))) return rc;
    if ((rc = launch_ce_finalize(d->tf.row_loss, d->tf.row_valid, M, nullptr, d->tr.count, nullptr, st))) return rc;
    const int chunk = (int)d->tr.chunk;
    for (int r0 = 0; r0 < M; r0 += chunk) {
        const int rows = (M - r0 < chunk) ? M - r0 : chunk;
        if ((rc = tr_lin16(d, d->lm_head, false, d->tr.xn16 + (size_t)r0 * D, nullptr, d->tr.logits, nullptr, rows, VP))) return rc;
        if ((rc = launch_ce_rows(d->tr.logits, (size_t)VP, V, r0, rows, ids, attention_mask, T, d->tf.row_loss, d->tf.row_valid,
                                 d->tr.row_lse, d->id_error, st)))
            return rc;
        if ((rc = launch_ce_backward16(d->tr.logits, (size_t)VP, V, r0, rows, ids, d->tf.row_valid, d->tr.row_lse, d->tr.count,
                                       loss_scale * s_int, d->id_error, d->tr.dl16, f16, st)))
            return rc;
        // (fp32: the 16-bit scratch still holds the ln_f rows the lm_head of later chunks reads)
        if ((rc = tr_lin16(d, d->lm_head, true, d->tr.dl16, nullptr, d->tr.dxn + (size_t)r0 * D, nullptr, rows, D))) return rc;
    }
    if ((rc = launch_ce_finalize(d->tf.row_loss, d->tf.row_valid, M, loss_out, nullptr, d->id_error, st))) return rc;
    if ((rc = id_error_end(d))) return rc;
    // backward through ln_f and the 24 frozen blocks; dx16 always carries the mask of the branch the gradient enters next
    if ((rc = launch_ln_backward16(d->tr.dxn, nullptr, xs(2 * L), d->lnf_g, d->tr.dx, d->tr.dx16, M, D, 0, dp(L - 1, 3), f16, st))) return rc;
    for (int l = L - 1; l >= 0; --l) {
        const LayerW& w = d->layers[l];
        float* qkv = a16 ? nullptr : d->tr.qkv + (size_t)l * M * 3 * D;
        GemmLnFold gb{};
        gb.G16 = d->tr.ffpre16 + (size_t)l * M * 4 * D;
        if ((rc = tr_lin16(d, w.mlp_proj, true, d->tr.dx16, nullptr, nullptr, d->tr.dff16, M, 4 * D, RGRG_ACT_NONE, &gb))) return rc;
        if ((rc = tr_lin16(d, w.c_fc, true, d->tr.dff16, nullptr, nullptr, dy16, M, D))) return rc;
        if ((rc = launch_ln_backward16(nullptr, dy16, xs(2 * l + 1), w.ln2_g, d->tr.dx, d->tr.dx16, M, D, 1, dp(l, 2), f16, st))) return rc;
        if (a16) {
            if ((rc = tr_lin16(d, w.attn_proj, true, d->tr.dx16, nullptr, nullptr, d->tr.datt16, M, D))) return rc;
            if ((rc = launch_attn16_backward(d->tr.qkv16 + (size_t)l * M * 3 * D, d->tr.ukv16, LD, l * 2 * D, attention_mask, d->tr.datt16,
                                             d->tr.att16 + (size_t)l * MD, d->tr.lse + (size_t)l * M * d->H, d->tr.dqkv16, d->tr.dukv, S,
                                             d->H, T, dp(l, 1), 1.0f / s_int, f16, st)))
                return rc;
        } else {
            if ((rc = tr_lin16(d, w.attn_proj, true, d->tr.dx16, nullptr, d->tf.att, nullptr, M, D))) return rc;
            if ((rc = launch_attn_backward(qkv, d->ukv_out, LD, l * 2 * D, attention_mask, d->tf.att, d->tr.att + (size_t)l * MD,
                                           d->tr.lse + (size_t)l * M * d->H, d->tr.delta, nullptr, d->tr.dukv, S, d->H, T, dp(l, 1), st,
                                           d->tr.dqkv16, f16, 1.0f / s_int)))
                return rc;
        }
        if ((rc = tr_lin16(d, w.c_attn, true, d->tr.dqkv16, nullptr, nullptr, dy16, M, D))) return rc;
        // the gradient enters layer l - 1 through its mlp branch (site 3); below layer 0 nothing reads the 16-bit copy
        if ((rc = launch_ln_backward16(nullptr, dy16, xs(2 * l), w.ln1_g, d->tr.dx, l > 0 ? d->tr.dx16 : nullptr, M, D, 1,
                                       l > 0 ? dp(l - 1, 3) : none, f16, st)))
            return rc;
    }
    return RGRG_OK;
}
}  // namespace rgrg

extern "C" int rgrg_decoder_lm_loss_grad(rgrg_decoder* d, const float* feats, const int64_t* input_ids,
                                         const float* attention_mask, int S, int T, float loss_scale, float dropout_p,
                                         uint64_t dropout_seed, float* loss_out,
                                         float* grad_ukv_w, float* grad_ukv_b, float* grad_fst0_w, float* grad_fst0_b,
                                         float* grad_fst2_w, float* grad_fst2_b, void* stream) {
    RGRG_CHECK_ARG(d && feats && input_ids && loss_out && grad_ukv_w && grad_ukv_b && grad_fst0_w && grad_fst0_b && grad_fst2_w &&
                   grad_fst2_b);
    RGRG_CHECK_ARG(S > 0 && S <= d->max_seqs && T >= 2 && T <= TF_MAX_T);
    RGRG_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f);
    RGRG_CHECK_ARG(!d->tf.pos || d->tf.pos_rows == T || d->tf.pos_rows == S * T);   // rgrg_decoder_set_lm_positions: [T] or [S * T]
    const int D = d->D, M = S * T, L = d->n_layer, V = d->V, VP = pad256(V), Sp = pad32(S), LD = d->ld_ukv;
    int rc;
    if ((rc = check_id_error(d))) return rc;
    const bool h16 = d->bf16_gemms && M > skinny_max_rows();   // 16-bit activation flow (tr_body16)
    const bool a16 = h16 && attn16_supported(T);               // ... with the 16-bit attention kernels
    if ((rc = tf_reserve(d, (size_t)M)) || (rc = tr_reserve(d, (size_t)M, (size_t)S, h16, a16))) return rc;
    hipStream_t caller = as_stream(stream), st = d->stream;
    RGRG_HIP(hipEventRecord(d->ev_in, caller));
    RGRG_HIP(hipStreamWaitEvent(st, d->ev_in, 0));
    if ((rc = id_error_begin(d))) return rc;
    if ((rc = ensure_wT(d))) return rc;
    const long long* ids = reinterpret_cast<const long long*>(input_ids);
    const size_t MD = (size_t)M * D;
    auto xs = [&](int i) { return d->tr.xs + (size_t)i * MD; };

    // ---------------- forward, keeping what the backward needs (layer inputs, qkv, c_fc pre-activations)
    RGRG_HIP(hipMemcpyAsync(d->feats, feats, (size_t)S * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    if ((rc = linear(d, d->fst0, d->feats, nullptr, d->h1, S, D, RGRG_ACT_RELU, false))) return rc;
    if ((rc = linear(d, d->fst2, d->h1, nullptr, d->img, S, D, RGRG_ACT_NONE, false))) return rc;
    if ((rc = linear(d, d->ukv, d->img, nullptr, d->ukv_out, S, LD, RGRG_ACT_NONE, false))) return rc;
    if (h16) {
        if ((rc = tr_body16(d, ids, attention_mask, S, T, loss_scale, dropout_p, dropout_seed, loss_out))) return rc;
    } else {
    if ((rc = launch_embed_seq_ln(d->wte, ids, T, d->layers[0].ln1_g, d->layers[0].ln1_b, xs(0), d->tf.xn, D, d->V, d->id_error, d->tf.pos,
                                  d->tf.pos_rows, M, st)))
        return rc;
    d->tf.pos = nullptr; d->tf.pos_rows = 1;   // consumed (rgrg_decoder_set_lm_positions)
    if (dropout_p > 0.f) {  // self.drop on the embeddings (language_model.py:311), then ln_1 of layer 0 again
        if ((rc = launch_dropout_add(xs(0), nullptr, xs(0), MD, DropoutParams{dropout_seed, 0u, dropout_p}, st))) return rc;
        if ((rc = launch_ln_rows(xs(0), d->layers[0].ln1_g, d->layers[0].ln1_b, d->tf.xn, D, nullptr, 0, M, st))) return rc;
    }
    for (int l = 0; l < L; ++l) {
        const LayerW& w = d->layers[l];
        const float* ng = (l + 1 < L) ? d->layers[l + 1].ln1_g : d->lnf_g;
        const float* nb = (l + 1 < L) ? d->layers[l + 1].ln1_b : d->lnf_b;
        float* qkv = d->tr.qkv + (size_t)l * M * 3 * D;
        float* ffpre = d->tr.ffpre + (size_t)l * M * 4 * D;
        if ((rc = tr_lin(d, w.c_attn, false, d->tf.xn, nullptr, qkv, M, 3 * D))) return rc;
        float* att = d->tr.att + (size_t)l * MD;              // attention output and row log-sum-exp, kept per layer
        float* lse = d->tr.lse + (size_t)l * M * d->H;
        const DropoutParams dp_att{dropout_seed, (unsigned)(l * 4 + 1), dropout_p}, dp_r1{dropout_seed, (unsigned)(l * 4 + 2), dropout_p},
            dp_r2{dropout_seed, (unsigned)(l * 4 + 3), dropout_p};
        if ((rc = launch_attn_prefill(qkv, d->ukv_out, LD, l * 2 * D, attention_mask, att, S, d->H, T, lse, dp_att, st))) return rc;
        if (dropout_p > 0.f) {  // resid_dropout: x_mid = x_in + dropout(c_proj(att))
            if ((rc = tr_lin(d, w.attn_proj, false, att, nullptr, d->tr.dbig, M, D))) return rc;
            if ((rc = launch_dropout_add(d->tr.dbig, xs(2 * l), xs(2 * l + 1), MD, dp_r1, st))) return rc;
        } else if ((rc = tr_lin(d, w.attn_proj, false, att, xs(2 * l), xs(2 * l + 1), M, D))) return rc;
        if ((rc = launch_ln_rows(xs(2 * l + 1), w.ln2_g, w.ln2_b, d->tf.xn, D, nullptr, 0, M, st))) return rc;
        if ((rc = tr_lin(d, w.c_fc, false, d->tf.xn, nullptr, ffpre, M, 4 * D))) return rc;
        if ((rc = launch_gelu_apply(ffpre, d->tr.ff, (size_t)M * 4 * D, st))) return rc;
        if (dropout_p > 0.f) {  // mlp dropout: x_out = x_mid + dropout(c_proj(gelu(c_fc(.))))
            if ((rc = tr_lin(d, w.mlp_proj, false, d->tr.ff, nullptr, d->tr.dxn, M, D))) return rc;
            if ((rc = launch_dropout_add(d->tr.dxn, xs(2 * l + 1), xs(2 * l + 2), MD, dp_r2, st))) return rc;
        } else if ((rc = tr_lin(d, w.mlp_proj, false, d->tr.ff, xs(2 * l + 1), xs(2 * l + 2), M, D))) return rc;
        if ((rc = launch_ln_rows(xs(2 * l + 2), ng, nb, d->tf.xn, D, nullptr, 0, M, st))) return rc;
    }
    // ---------------- lm_head + loss + d(logits) + d(ln_f output), chunk by chunk (the logits never exist as a whole)
    if ((rc = launch_ce_valid(attention_mask, T, M, d->tf.row_loss, d->tf.row_valid, st))) return rc;
    if ((rc = launch_ce_finalize(d->tf.row_loss, d->tf.row_valid, M, nullptr, d->tr.count, nullptr, st))) return rc;
    for (int r0 = 0; r0 < M; r0 += TF_LOGIT_ROWS) {
        const int rows = (M - r0 < TF_LOGIT_ROWS) ? M - r0 : TF_LOGIT_ROWS;
        if ((rc = tr_lin(d, d->lm_head, false, d->tf.xn + (size_t)r0 * D, nullptr, d->tr.logits, rows, VP))) return rc;
        if ((rc = launch_ce_rows(d->tr.logits, (size_t)VP, V, r0, rows, ids, attention_mask, T, d->tf.row_loss, d->tf.row_valid,
                                 d->tr.row_lse, d->id_error, st)))
            return rc;
        if ((rc = launch_ce_backward(d->tr.logits, (size_t)VP, V, r0, rows, ids, d->tf.row_valid, d->tr.row_lse, d->tr.count,
                                     loss_scale, d->id_error, st)))
            return rc;
        if ((rc = tr_lin(d, d->lm_head, true, d->tr.logits, nullptr, d->tr.dxn + (size_t)r0 * D, rows, D))) return rc;
    }
    if ((rc = launch_ce_finalize(d->tf.row_loss, d->tf.row_valid, M, loss_out, nullptr, d->id_error, st))) return rc;
    if ((rc = id_error_end(d))) return rc;
    // ---------------- backward through ln_f and the 24 frozen blocks (activation gradients only)
    if ((rc = launch_ln_backward(d->tr.dxn, xs(2 * L), d->lnf_g, d->tr.dx, M, D, 0, st))) return rc;
    for (int l = L - 1; l >= 0; --l) {
        const LayerW& w = d->layers[l];
        float* qkv = d->tr.qkv + (size_t)l * M * 3 * D;
        float* ffpre = d->tr.ffpre + (size_t)l * M * 4 * D;
        // x_out = x_mid + dropout(mlp_proj(gelu(c_fc(ln_2(x_mid)))))
        const float* dbr = d->tr.dx;  // gradient entering the branch = dx * mask (same mask as the forward pass)
        if (dropout_p > 0.f) {
            if ((rc = launch_dropout_add(d->tr.dx, nullptr, d->tf.att, MD, DropoutParams{dropout_seed, (unsigned)(l * 4 + 3), dropout_p}, st)))
                return rc;
            dbr = d->tf.att;
        }
        if ((rc = tr_lin(d, w.mlp_proj, true, dbr, nullptr, d->tr.dbig, M, 4 * D))) return rc;
        if ((rc = launch_gelu_backward(d->tr.dbig, ffpre, (size_t)M * 4 * D, st))) return rc;
        if ((rc = tr_lin(d, w.c_fc, true, d->tr.dbig, nullptr, d->tr.dxn, M, D))) return rc;
        if ((rc = launch_ln_backward(d->tr.dxn, xs(2 * l + 1), w.ln2_g, d->tr.dx, M, D, 1, st))) return rc;
        // x_mid = x_in + dropout(attn_proj(attention(c_attn(ln_1(x_in)), uk(img), uv(img))))
        dbr = d->tr.dx;
        if (dropout_p > 0.f) {
            if ((rc = launch_dropout_add(d->tr.dx, nullptr, d->tr.dxn, MD, DropoutParams{dropout_seed, (unsigned)(l * 4 + 2), dropout_p}, st)))
                return rc;
            dbr = d->tr.dxn;
        }
        if ((rc = tr_lin(d, w.attn_proj, true, dbr, nullptr, d->tf.att, M, D))) return rc;
        if ((rc = launch_attn_backward(qkv, d->ukv_out, LD, l * 2 * D, attention_mask, d->tf.att, d->tr.att + (size_t)l * MD,
                                       d->tr.lse + (size_t)l * M * d->H, d->tr.delta, d->tr.dbig, d->tr.dukv, S, d->H, T,
                                       DropoutParams{dropout_seed, (unsigned)(l * 4 + 1), dropout_p}, st)))
            return rc;
        if ((rc = tr_lin(d, w.c_attn, true, d->tr.dbig, nullptr, d->tr.dxn, M, D))) return rc;
        if ((rc = launch_ln_backward(d->tr.dxn, xs(2 * l), w.ln1_g, d->tr.dx, M, D, 1, st))) return rc;
    }
    }   // fp32-activation flow
    // ---------------- uk / uv of every layer (one stacked Linear) and feature_space_transformation_nn
    if ((rc = launch_colsum(d->tr.dukv, grad_ukv_b, S, LD, st))) return rc;
    if ((rc = tr_gemm(d, d->tr.dukv, d->ukv.wT, nullptr, nullptr, d->tr.dimg, S, D, pad256(LD), D))) return rc;
    if ((rc = launch_transpose_pad(d->tr.dukv, d->tr.t1, S, LD, Sp, st))) return rc;
    if ((rc = launch_transpose_pad(d->img, d->tr.t2, S, D, Sp, st))) return rc;
    if ((rc = tr_gemm(d, d->tr.t1, d->tr.t2, nullptr, nullptr, grad_ukv_w, LD, D, Sp, D))) return rc;
    if ((rc = launch_colsum(d->tr.dimg, grad_fst2_b, S, D, st))) return rc;
    if ((rc = launch_transpose_pad(d->tr.dimg, d->tr.t1, S, D, Sp, st))) return rc;
    if ((rc = launch_transpose_pad(d->h1, d->tr.t2, S, D, Sp, st))) return rc;
    if ((rc = tr_gemm(d, d->tr.t1, d->tr.t2, nullptr, nullptr, grad_fst2_w, D, D, Sp, D))) return rc;
    if ((rc = tr_gemm(d, d->tr.dimg, d->fst2.wT, nullptr, nullptr, d->tr.dh1, S, D, pad256(D), D))) return rc;
    if ((rc = launch_relu_backward(d->tr.dh1, d->h1, (size_t)S * D, st))) return rc;
    if ((rc = launch_colsum(d->tr.dh1, grad_fst0_b, S, D, st))) return rc;
    if ((rc = launch_transpose_pad(d->tr.dh1, d->tr.t1, S, D, Sp, st))) return rc;
    if ((rc = launch_transpose_pad(d->feats, d->tr.t2, S, D, Sp, st))) return rc;
    if ((rc = tr_gemm(d, d->tr.t1, d->tr.t2, nullptr, nullptr, grad_fst0_w, D, D, Sp, D))) return rc;
    RGRG_HIP(hipEventRecord(d->ev_in, st));
    RGRG_HIP(hipStreamWaitEvent(caller, d->ev_in, 0));
    return RGRG_OK;
}

// Roofline support for BASELINE configs[4] (bench.py): the frozen-weight GEMMs of ONE training step of the 16-bit flow - per
// layer c_attn, attn_proj, c_fc, mlp_proj forward and their four activation-gradient GEMMs, lm_head forward and dgrad per
// chunk - launched back to back on the decoder's stream with the operands and epilogues of tr_body16, timed between two HIP
// events (one untimed pass in front).  The work space of the last rgrg_decoder_lm_loss_grad call at this shape is reused (its
// contents are overwritten with garbage: timing only).  flops = 2 M N K of those launches.
extern "C" int rgrg_decoder_time_train_gemms(rgrg_decoder* d, int S, int T, int iters, float* ms_per_step, double* flops_per_step,
                                             int* launches_per_step) {
    RGRG_CHECK_ARG(d && S > 0 && T >= 2 && iters > 0 && ms_per_step && flops_per_step && launches_per_step);
    const int D = d->D, M = S * T, L = d->n_layer, VP = pad256(d->V);
    if (!d->tr.h16 || (size_t)M > d->tr.rows || !d->bf16_gemms) {
        set_error("time_train_gemms: run a 16-bit training pass of this shape first (16-bit work space %d, rows %zu of %d, mode %d)",
                  (int)d->tr.h16, d->tr.rows, M, d->bf16_gemms);
        return RGRG_EINVAL;
    }
    const bool a16 = d->tr.a16;
    const size_t MD = (size_t)M * D;
    hipEvent_t e0, e1;
    RGRG_HIP(hipEventCreate(&e0));
    RGRG_HIP(hipEventCreate(&e1));
    int rc = RGRG_OK, launches = 0;
    double flops = 0.0;
    auto cnt = [&](const Lin& l) { flops += 2.0 * M * (double)l.N * l.K; ++launches; };
    for (int it = -1; it < iters && !rc; ++it) {
        if (it == 0) RGRG_HIP(hipEventRecord(e0, d->stream));
        const bool c = it == -1;
        for (int l = 0; l < L && !rc; ++l) {
            const LayerW& w = d->layers[l];
            unsigned short* att16 = a16 ? d->tr.att16 + (size_t)l * MD : d->tr.att16;
            GemmLnFold pre{}, gb{};
            pre.Ypre16 = d->tr.ffpre16 + (size_t)l * M * 4 * D;
            gb.G16 = d->tr.ffpre16 + (size_t)l * M * 4 * D;
            if (a16) rc = tr_lin16(d, w.c_attn, false, d->tr.xn16, nullptr, nullptr, d->tr.qkv16 + (size_t)l * M * 3 * D, M, 3 * D);
            else rc = tr_lin16(d, w.c_attn, false, d->tr.xn16, nullptr, d->tr.qkv + (size_t)l * M * 3 * D, nullptr, M, 3 * D);
            if (rc || (rc = tr_lin16(d, w.attn_proj, false, att16, nullptr, nullptr, d->tr.dx16, M, D))) break;
            if ((rc = tr_lin16(d, w.c_fc, false, d->tr.xn16, nullptr, nullptr, d->tr.ff16, M, 4 * D, RGRG_ACT_GELU_NEW, &pre))) break;
            if ((rc = tr_lin16(d, w.mlp_proj, false, d->tr.ff16, nullptr, nullptr, d->tr.dx16, M, D))) break;
            if ((rc = tr_lin16(d, w.mlp_proj, true, d->tr.dx16, nullptr, nullptr, d->tr.dff16, M, 4 * D, RGRG_ACT_NONE, &gb))) break;
            if ((rc = tr_lin16(d, w.c_fc, true, d->tr.dff16, nullptr, nullptr, d->tr.xn16, M, D))) break;
            if (a16) rc = tr_lin16(d, w.attn_proj, true, d->tr.dx16, nullptr, nullptr, d->tr.datt16, M, D);
            else rc = tr_lin16(d, w.attn_proj, true, d->tr.dx16, nullptr, d->tr.dxn, nullptr, M, D);
            if (rc || (rc = tr_lin16(d, w.c_attn, true, d->tr.dqkv16, nullptr, nullptr, d->tr.xn16, M, D))) break;
            if (c) { cnt(w.c_attn); cnt(w.attn_proj); cnt(w.c_fc); cnt(w.mlp_proj); cnt(w.mlp_proj); cnt(w.c_fc); cnt(w.attn_proj); cnt(w.c_attn); }
        }
        const int chunk = (int)d->tr.chunk;
        for (int r0 = 0; r0 < M && !rc; r0 += chunk) {
            const int rows = (M - r0 < chunk) ? M - r0 : chunk;
            if ((rc = tr_lin16(d, d->lm_head, false, d->tr.xn16 + (size_t)r0 * D, nullptr, d->tr.logits, nullptr, rows, VP))) break;
            if ((rc = tr_lin16(d, d->lm_head, true, d->tr.dl16, nullptr, d->tr.dxn + (size_t)r0 * D, nullptr, rows, D))) break;
            if (c) { flops += 2.0 * 2.0 * rows * (double)d->lm_head.N * d->lm_head.K; launches += 2; }
        }
    }
    float ms = 0.f;
    if (!rc) {
        RGRG_HIP(hipEventRecord(e1, d->stream));
        RGRG_HIP(hipEventSynchronize(e1));
        RGRG_HIP(hipEventElapsedTime(&ms, e0, e1));
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    *ms_per_step = ms / iters;
    *flops_per_step = flops;
    *launches_per_step = launches;
    return RGRG_OK;
}

// Test hook: the attention of the teacher-forced / training forward pass alone, on the caller's buffers, through launch_attn_prefill.
extern "C" int rgrg_debug_attn_prefill(const float* qkv, const float* ukv, int ld_ukv, int kcol, const float* am, float* out,
                                       uint16_t* out16, float* lse, int S, int H, int T, int variant, uint64_t seed,
                                       uint32_t stream_id, float p, int fp16, void* stream) {
    RGRG_CHECK_ARG(qkv && ukv && out && S > 0 && H > 0 && kcol >= 0 && ld_ukv >= kcol + 2 * H * 64 && p >= 0.f && p < 1.f);
    RGRG_CHECK_ARG(variant >= 0 && variant <= 3);
    return launch_attn_prefill(qkv, ukv, ld_ukv, kcol, am, out, S, H, T, lse, DropoutParams{seed, stream_id, p}, as_stream(stream), out16,
                               fp16 ? 1 : 0, variant);
}

// Test hooks: the cross-entropy kernels of the teacher-forced passes alone, through the launchers above.
// rgrg_debug_ce_rows: ce_valid_kernel over all M rows (as the training pass does first), then ce_rows_kernel over the chunk.
extern "C" int rgrg_debug_ce_rows(const float* logits, int64_t ld, int V, int row0, int rows, const int64_t* ids, const float* am, int T,
                                  int M, float* row_loss, int* row_valid, float* row_lse, int* id_error, void* stream) {
    RGRG_CHECK_ARG(logits && ids && row_loss && row_valid && id_error && V > 0 && ld >= V && T >= 2 && M > 0 && M % T == 0);
    RGRG_CHECK_ARG(row0 >= 0 && rows > 0 && row0 <= M - rows);
    int rc = launch_ce_valid(am, T, M, row_loss, row_valid, as_stream(stream));
    if (rc) return rc;
    return launch_ce_rows(logits, (size_t)ld, V, row0, rows, reinterpret_cast<const long long*>(ids), am, T, row_loss, row_valid, row_lse,
                          id_error, as_stream(stream));
}

extern "C" int rgrg_debug_ce_finalize(const float* row_loss, const int* row_valid, int n, float* loss, int* n_scored, const int* id_error,
                                      void* stream) {
    RGRG_CHECK_ARG(row_loss && row_valid && n > 0 && (loss || n_scored));
    return launch_ce_finalize(row_loss, row_valid, n, loss, n_scored, id_error, as_stream(stream));
}

// Test hook: embed_seq_ln_kernel alone (tests/test_gpu_step_rows.py), one workgroup per token row of S x T.
extern "C" int rgrg_debug_embed_seq_ln(const float* wte, const int64_t* ids, const int64_t* pos_ids, int pos_rows, const float* g,
                                       const float* b, float* x, float* xn, int* id_error, int S, int T, int D, int V, void* stream) {
    RGRG_CHECK_ARG(wte && ids && g && b && x && xn && id_error && S >= 1 && T >= 1 && D == 1024 && V >= 1);
    RGRG_CHECK_ARG((long long)S * T <= 0x7fffffffLL);
    RGRG_CHECK_ARG(!pos_ids || pos_rows == T || pos_rows == S * T);   // [1,T] broadcast over the sentences, or [S,T]
    return launch_embed_seq_ln(wte, reinterpret_cast<const long long*>(ids), T, g, b, x, xn, D, V, id_error,
                               reinterpret_cast<const long long*>(pos_ids), pos_ids ? pos_rows : 1, S * T, as_stream(stream));
}
