// Host functions and types of librgrg_hip.so that cross translation units.  Every .hip file that defines or calls one
// of them includes this header, so the compiler checks each definition against the one declaration (default arguments
// live here only).  No device code: device helpers are in common.h.
#pragma once
#include "common.h"

namespace rgrg {

// ------------------------------------------------------------------ gemm_f32.hip
int launch_gemm_dense(const float* A, const float* W, const float* shift, const float* R, float* Y, int M, int N, int K,
                      int ldy, int act, float* ws, size_t ws_floats, hipStream_t st);
int init_gemm_attrs();

// ------------------------------------------------------------------ gemm_bf16.hip (f16: the 16-bit type - 0 bf16, 1 IEEE fp16)
struct GemmLnFold {   // LayerNorm folded around the 16-bit GEMMs (gemm_bf16.hip: GemmBf16Params)
    void* Yb16 = nullptr;               // producer: 16-bit copy of the fp32 result (the raw residual stream) ...
    float* stats_out = nullptr;         // ... and per-row (sum, sum of squares) slots [M][16][2]
    const float* ln_stats = nullptr;    // consumer: those slots
    const float* ln_colsum = nullptr;   // consumer: column sums of the gain-scaled rounded weights
    void* Ypre16 = nullptr;             // training pass: 16-bit pre-activation copy next to the activated Y16 (c_fc)
    const void* G16 = nullptr;          // training pass: saved 16-bit pre-activations, result *= gelu_new'(G16) (mlp_proj dgrad)
    int ksplit = 0;                     // split-K over `ksplit` workgroups per tile with a last-arriver reduce (work space, tickets)
    float* sk_ws = nullptr;
    unsigned* sk_cnt = nullptr;
    float* cand_val = nullptr;          // 256 x 256 kernel: per-row (maximum, column) of every column tile instead of Y (greedy lm_head)
    int* cand_idx = nullptr;
    int kp = 0;                         // the K-parity ping-pong kernel (gemm_kp.inc), tile from (N, K) only
    // consumer, c_attn of the many-sequence decode step (N = 3 * kv_H * 64): the k / v columns go to slot *kv_step + 1 of the 16-bit
    // cache planes [rows][kv_H][kv_T][64] (already offset to the launch's first sequence), rounded to the GEMM's 16-bit type, instead
    // of to Y; the q columns go to Y as fp32.  LDS-DMA kernel only.
    void *kv_k = nullptr, *kv_v = nullptr;
    const int* kv_step = nullptr;
    int kv_H = 0, kv_T = 0;
};
int init_gemm_bf16_attrs();
bool gemm_bf16_cand_epilogue_ok(int M, int N, int K);   // would launch_gemm_bf16w_ex pick the 256 x 256 kernel for this lm_head?
int launch_gemm_bf16w_ex(const float* A, const void* A16, const void* Wb, const float* shift, const float* R, float* Y, void* Y16,
                         int M, int N, int K, int ldy, int act, hipStream_t st, int f16, const GemmLnFold* ln = nullptr);
int launch_gemm_bf16w(const float* A, const void* Wb, const float* shift, const float* R, float* Y, int M, int N, int K,
                      int ldy, int act, hipStream_t st, int f16);
int convert_f32_to_bf16(const float* src, void* dst, size_t n, hipStream_t st, int f16);

// ------------------------------------------------------------------ train_ops.hip
int launch_gelu_apply(const float* pre, float* out, size_t n, hipStream_t st);
int launch_gelu_backward(float* d, const float* pre, size_t n, hipStream_t st);
int launch_relu_backward(float* d, const float* h, size_t n, hipStream_t st);
int launch_ln_backward(const float* dy, const float* x, const float* g, float* out, int rows, int D, int accumulate, hipStream_t st);
int launch_ce_backward(float* logits, size_t ld, int V, int row0, int rows, const long long* ids, const int* row_valid,
                       const float* row_lse, const int* n_scored, float scale, const int* id_error, hipStream_t st);
int launch_transpose_pad(const float* src, float* dst, int R, int Cc, int Rp, hipStream_t st);
int launch_colsum(const float* src, float* out, int R, int Cc, hipStream_t st);
int launch_attn_backward(const float* qkv, const float* ukv, int ld_ukv, int kcol, const float* am, const float* d_att,
                         const float* att, const float* lse, float* delta, float* d_qkv, float* d_ukv, int S, int H, int T,
                         DropoutParams drop, hipStream_t st, unsigned short* d_qkv16 = nullptr, int f16 = 0, float ukv_scale = 1.0f);
int launch_resid_dropout_ln16(const float* y, const unsigned short* y16, const float* resid, float* x, const float* g, const float* b,
                              unsigned short* xn16, DropoutParams drop, int f16, int rows, int D, hipStream_t st);
int launch_ln_backward16(const float* dy, const unsigned short* dy16, const float* x, const float* g, float* out, unsigned short* out16,
                         int rows, int D, int accumulate, DropoutParams drop, int f16, hipStream_t st);
int launch_ce_backward16(const float* logits, size_t ld, int V, int row0, int rows, const long long* ids, const int* row_valid,
                         const float* row_lse, const int* n_scored, float scale, const int* id_error, unsigned short* out16, int f16,
                         hipStream_t st);
int launch_dropout_add(const float* src, const float* resid, float* out, size_t n, DropoutParams drop, hipStream_t st);

// ------------------------------------------------------------------ attn_train16.hip
bool attn16_supported(int T);
int launch_attn16_forward(const unsigned short* qkv16, const unsigned short* ukv16, int ld_ukv, int kcol, const float* am,
                          unsigned short* out16, float* lse, int S, int H, int T, DropoutParams drop, int f16, hipStream_t st);
int launch_attn16_backward(const unsigned short* qkv16, const unsigned short* ukv16, int ld_ukv, int kcol, const float* am,
                           const unsigned short* d_att16, const unsigned short* att16, const float* lse, unsigned short* d_qkv16,
                           float* d_ukv, int S, int H, int T, DropoutParams drop, float ukv_scale, int f16, hipStream_t st);


// ------------------------------------------------------------------ sample.hip (the token sampler; contract: rgrg_hip.h "Sampling")
size_t sample_params_bytes();
// validates and writes the device-side parameter block the sample step reads (so a captured step serves every call)
int enqueue_sample_params(void* prm_dev, float temperature, int top_k, float top_p, unsigned long long seed, hipStream_t st);
// one decode step's draw for rows [0, S) of logits + the greedy bookkeeping (record_step_token); lp [S][ld_lp] or null
int launch_sample_step(const float* logits, int ld, int S, int V, const void* prm_dev, long long* ids, int ld_ids, int* finished,
                       int* step, int* done_len, int* sync, float* lp, int ld_lp, hipStream_t st);

}  // namespace rgrg
