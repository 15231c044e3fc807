// Fragment-direct weight-streaming GEMMs of the fused decode plan (<= 128 token rows).  Included by decoder.hip
// inside namespace rgrg.
//
// Everything an MFMA consumes is stored in the order the MFMA consumes it:
//   * weights: pack_weights16_kernel, [column tile 16][k chunk 16][64 lanes][4] (as before);
//   * ACTIVATIONS too ("fragment-major"): a matrix X [rows][K] that is the A operand of v_mfma_f32_16x16x4_f32 lives as
//         Xf[tile = row / 32][half = (row % 32) / 16][kc = k / 16][lane = ((k % 16) / 4) * 16 + row % 16][k % 4]
//     so the 64 lanes of a wave fetch the A fragment of (tile, half, kc) as ONE contiguous 1-KiB load, straight into
//     registers.  No LDS staging, no barrier before the first MFMA; LDS only carries the 8-wave K reduction.
//     Producers (GEMM epilogues, the attention kernel) write this layout; only qkv and the logits stay row-major.
//   * LayerNorm is folded into the GEMM that consumes it (weights are frozen, language_model.py:207-213):
//         LN(x) W^T + bias = rstd * (x (g o W)^T - mean * c1) + c2,   c1[n] = sum_k g[k] W[n,k],
//                                                                     c2[n] = sum_k b[k] W[n,k] + bias[n]
//     the kernel streams the pre-scaled weights g o W over the RAW residual stream, accumulates sum(x) and sum(x^2) of
//     the fragments it holds anyway, and applies mean / rstd / c1 / c2 in the epilogue.  var = E[x^2] - mean^2 in
//     fp32 (clamped at 0); results agree with the two-pass LayerNorm to ~1e-6 relative, not bit for bit.
//   * the residual-stream sources of the consumer (DX_COMBINE4: x + the split-K sums of the previous mlp_proj,
//     DX_EMBED: wte[token] + wte[step]) are added in registers while the fragments are loaded; workgroup (0, 0)
//     writes the combined rows back (ping-pong buffer) for the later residual add.
//   * split-K (mlp_proj: 4 K slices so that the fp32 MFMA work covers all 256 CUs): slices {0,1} and {2,3} each add
//     their partial sums ATOMICALLY into one accumulator that starts at zero (attn_proj's epilogue zeroes it).  Two
//     addends on a zero are order-independent (0 + a + b == 0 + b + a bit for bit), so the result stays
//     deterministic, and the consumer reads x + acc01 + acc23 (3 streams) instead of x + 4 partial sums (5 streams):
//     every consumer workgroup re-reads these streams through its CU's 64 B/clk L2 port, 128 KiB each.
// Request order inside a wave: activation fragments first, the HBM weight stream last (vector loads return in order:
// a wait on an activation never waits for an HBM miss).
// (frag_off, the offset of one element in the fragment-major layout, and dx_rsrc are in common.h: the decode attention uses them too.)

constexpr int DX_PLAIN = 0, DX_COMBINE4 = 1, DX_EMBED = 2, DX_EMBED_TOK = 3, DX_EMBED_TOKPOS = 4;   // TOKPOS: per-row tokens AND positions
constexpr int DK_PW = 8;        // one-KiB weight chunks (16 k each) per wave; a workgroup covers 8 * 8 * 16 = 1024 k
constexpr int DK_SLICE = 1024;  // K slice of one workgroup

struct DirectArgs {
    const float* Xf;    // A operand, fragment-major, row length K (DX_PLAIN / DX_COMBINE4)
    const float* part;  // DX_COMBINE4: the two pairwise accumulators, fragment-major [tile][2][2 halves][64][64][4], of a 1024-column producer
    float* xout;        // DX_COMBINE4 / DX_EMBED*: workgroup (0,0) writes the rebuilt rows (fragment-major) here
    const float* wte;   // DX_EMBED*: embedding table [V][1024]
    const long long* ids;
    int ld_ids;
    const int* step;
    const int* tok_override;
    const int* pos_override;   // DX_EMBED_TOKPOS: embedding position of every row (forward(position_ids=...), language_model.py:293-307)
    const float* P;     // packed weights [NT][K / 16][64][4] (pre-scaled by the LayerNorm weight when LNF)
    const float* bias;  // [N] or null; LNF: the folded vector c2
    const float* c1;    // LNF: column sums of the scaled weights
    const float* Rf;    // residual, fragment-major, row length N, or null
    float* Y;           // row-major output [M][ldy] or null
    int ldy;
    float* Yf;          // fragment-major output, row length N, or null
    float* part_out;    // KS == 4: the two accumulators [tile][2][2][N / 16][64][4]; slices 2p, 2p + 1 atomically add into p (bias: slice 0)
    float* zero_acc;    // accumulators (same layout, N columns) this kernel's epilogue resets to zero, or null
    int M, K, N, NT, KS, act;
    float* cand_val;    // optional per-tile row maxima (fused arg-max of lm_head): [rows][NT]
    int* cand_idx;
};

__device__ __forceinline__ f32x4 dx_ldb(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ f32x4 dx_ldb_nt(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 2));  // aux 2 = nt
}

// 16-bit-weight variant (round 6, W16 = 1 bf16 / 2 fp16; 33-128 rows under torch.autocast): the packed weights are stored as 16 bit in
// the SAME fragment order ([column tile 16][k chunk 16][64 lanes][4], 8 bytes per lane and chunk) and a lane's 4 values of a chunk -
// k = 16 c + 4 (lane / 16) + j - are exactly the 4 consecutive k that lane feeds to v_mfma_f32_16x16x16_{bf16,f16}: ONE 16-bit
// MFMA replaces the four fp32 16x16x4 ones, the activations stay fp32 fragment-major in memory and are rounded (RNE) on their
// way into the matrix core - the rounding point of the many-sequence 16-bit GEMMs - and the weight stream halves.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
template <int W16> struct DxW { typedef u32x2 type; };
template <> struct DxW<0> { typedef f32x4 type; };
template <int W16>
__device__ __forceinline__ typename DxW<W16>::type dx_ldw_nt(__amdgpu_buffer_rsrc_t r, int lane, int chunk) {
    if constexpr (W16 == 0) return dx_ldb_nt(r, (unsigned)lane * 16u, (unsigned)chunk * 1024u);
    else return __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r, lane * 8, chunk * 512, 2));   // aux 2 = nt
}
// acc += A (this lane's 4 k of the chunk, fp32) x W (the same 4 k of its column)
template <int W16>
__device__ __forceinline__ f32x4v dx_mfma_chunk(const f32x4& x, const typename DxW<W16>::type& w, f32x4v acc) {
    if constexpr (W16 == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j], w[j], acc, 0, 0, 0);
        return acc;
    } else if constexpr (W16 == 2) {
        const h16x4 a = {(_Float16)x[0], (_Float16)x[1], (_Float16)x[2], (_Float16)x[3]};
        return __builtin_amdgcn_mfma_f32_16x16x16f16(a, __builtin_bit_cast(h16x4, w), acc, 0, 0, 0);
    } else {
        const s16x4 a = {(short)f32_to_bf16_bits(x[0]), (short)f32_to_bf16_bits(x[1]), (short)f32_to_bf16_bits(x[2]), (short)f32_to_bf16_bits(x[3])};
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(s16x4, w), acc, 0, 0, 0);
    }
}

// A fragments xa[half][c] (rows r, r + 16 of tile mt; chunks kc0 .. kc0 + 7) of this wave; `tail` (the weight
// requests) is called once after the last activation request.  kc0 / mt are wave-uniform (SGPR offsets).
template <int MODE, typename F>
__device__ __forceinline__ void dx_load_frags(f32x4 (&xa)[2][DK_PW], const DirectArgs& a, int mt, int kc0, int lane, F&& tail) {
    const unsigned voff = (unsigned)lane * 16u;
    if constexpr (MODE == DX_EMBED_TOKPOS) {
        // wte[token[row]] + wte[position[row]]: the incremental forward with caller-given position_ids (any values per row)
        const int r = lane & 15, q = lane >> 4;
        const __amdgpu_buffer_rsrc_t rw = dx_rsrc(a.wte);
        unsigned tokb[2], posb[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = mt * 32 + h * 16 + r;
            tokb[h] = (unsigned)a.tok_override[row] * 4096u + (unsigned)q * 16u;
            posb[h] = (unsigned)a.pos_override[row] * 4096u + (unsigned)q * 16u;
        }
        f32x4 pos[2][DK_PW];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < DK_PW; ++c) {
                xa[h][c] = dx_ldb(rw, tokb[h], (unsigned)(kc0 + c) * 64u);
                pos[h][c] = dx_ldb(rw, posb[h], (unsigned)(kc0 + c) * 64u);
            }
        __builtin_amdgcn_sched_barrier(0);
        tail();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < DK_PW; ++c) xa[h][c] += pos[h][c];
    } else if constexpr (MODE == DX_EMBED || MODE == DX_EMBED_TOK) {
        const int t = *a.step;
        const int r = lane & 15, q = lane >> 4;
        long long tok[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = mt * 32 + h * 16 + r;
            if constexpr (MODE == DX_EMBED_TOK) tok[h] = (long long)a.tok_override[row];  // beam search feeds the beam tokens
            else tok[h] = a.ids[(size_t)row * a.ld_ids + t];
        }
        const __amdgpu_buffer_rsrc_t rw = dx_rsrc(a.wte);
        f32x4 pos[DK_PW];
#pragma unroll
        for (int c = 0; c < DK_PW; ++c) pos[c] = dx_ldb(rw, (unsigned)q * 16u, (unsigned)t * 4096u + (unsigned)(kc0 + c) * 64u);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < DK_PW; ++c)
                xa[h][c] = dx_ldb(rw, (unsigned)tok[h] * 4096u + (unsigned)q * 16u, (unsigned)(kc0 + c) * 64u);
        __builtin_amdgcn_sched_barrier(0);
        tail();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < DK_PW; ++c) xa[h][c] += pos[c];  // wte[token] + wte[step]  (quirk language_model.py:307)
    } else {
        const int kchunks = a.K >> 4;
        const __amdgpu_buffer_rsrc_t rx = dx_rsrc(a.Xf);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < DK_PW; ++c)
                xa[h][c] = dx_ldb(rx, voff, (unsigned)(((mt * 2 + h) * kchunks + kc0 + c) * 1024));
        if constexpr (MODE == DX_PLAIN) {
            __builtin_amdgcn_sched_barrier(0);
            tail();
            __builtin_amdgcn_sched_barrier(0);
        } else {
            // + the two split-K accumulators of the producer (slice 0 carried its bias): 32 more 16-byte loads per
            // lane, all in flight together.  Per element (x + acc01) + acc23, fixed order.
            const __amdgpu_buffer_rsrc_t rp = dx_rsrc(a.part);
            f32x4 pa[2][DK_PW], pc[2][DK_PW];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < DK_PW; ++c) {
                    pa[h][c] = dx_ldb(rp, voff, (unsigned)(((((mt * 2 + 0) * 2 + h) * 64) + kc0 + c) * 1024));
                    pc[h][c] = dx_ldb(rp, voff, (unsigned)(((((mt * 2 + 1) * 2 + h) * 64) + kc0 + c) * 1024));
                }
            __builtin_amdgcn_sched_barrier(0);
            tail();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < DK_PW; ++c) xa[h][c] = (xa[h][c] + pa[h][c]) + pc[h][c];
        }
    }
}

// sum(x), sum(x^2) of the fragments of a wave -> st[row][0 / 1] (per wave); lanes of one row sit 16 apart
__device__ __forceinline__ void dx_row_stats(const f32x4 (&xa)[2][DK_PW], float (*st)[2], int lane) {
    float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < DK_PW; ++c) {
            const f32x4 x = xa[h][c];
            s1[h] += (x[0] + x[1]) + (x[2] + x[3]);
            s2[h] += (x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]);
        }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        s1[h] += __shfl_xor(s1[h], 16, 64);
        s1[h] += __shfl_xor(s1[h], 32, 64);
        s2[h] += __shfl_xor(s2[h], 16, 64);
        s2[h] += __shfl_xor(s2[h], 32, 64);
    }
    if (lane < 16) {
        st[lane][0] = s1[0];      st[lane][1] = s2[0];
        st[lane + 16][0] = s1[1]; st[lane + 16][1] = s2[1];
    }
}

__device__ __forceinline__ void dx_row_mean_rstd(const float (*st)[32][2], int lrow, int K, float& mean, float& rstd) {
    float S1 = st[0][lrow][0], S2 = st[0][lrow][1];
#pragma unroll
    for (int w2 = 1; w2 < SK_WAVES; ++w2) { S1 += st[w2][lrow][0]; S2 += st[w2][lrow][1]; }
    mean = S1 / (float)K;
    const float var = fmaxf(S2 / (float)K - mean * mean, 0.f);
    rstd = 1.0f / sqrtf(var + LN_EPS);
}

// One workgroup = one 16-column tile x one 1024-wide K slice (blockIdx.y) x up to MT row tiles of 32.
template <int MT, int MODE, bool LNF, int W16 = 0>
__global__ __launch_bounds__(512) void rgrg_skinny_direct_f32(const DirectArgs a) {
    __shared__ __attribute__((aligned(16))) float red[SK_WAVES * 8 * 64];
    __shared__ float st[MT][SK_WAVES][32][2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform: scalar offsets for the buffer loads
    const int nt = blockIdx.x, ks = blockIdx.y;
    const int kchunks = a.K >> 4;
    const int kc0 = ks * (DK_SLICE / 16) + wave * DK_PW;
    const __amdgpu_buffer_rsrc_t rw = dx_rsrc(a.P);
    typename DxW<W16>::type w[DK_PW];
    auto issue_weights = [&]() {
#pragma unroll
        for (int c = 0; c < DK_PW; ++c) w[c] = dx_ldw_nt<W16>(rw, lane, nt * kchunks + kc0 + c);
    };
    // Epilogue operands of this thread (bias / folded vectors of its column, residual of its output element): requested
    // right behind the weight stream, i.e. two HBM latencies before the epilogue needs them - loaded IN the epilogue
    // they would add a full cold miss (~1-2 us) to the tail of every launch.
    const int e_half = tid >> 8, e_rr = (tid >> 6) & 3, e_l = tid & 63;
    const int e_col = nt * 16 + (e_l & 15);
    const int e_in = (((e_l & 15) >> 2) * 16 + (e_l >> 4) * 4 + e_rr) * 4 + (e_l & 3);  // position inside a 16 x 16 fragment block
    float e_bias = 0.f, e_c1 = 0.f, e_rf[MT];
    float acc[MT][8];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        f32x4 xa[2][DK_PW];
        if (mt == 0) {
            dx_load_frags<MODE>(xa, a, mt, kc0, lane, issue_weights);
            if (e_col < a.N) {
                if (a.bias && (a.KS == 1 || ks == 0)) e_bias = a.bias[e_col];
                if constexpr (LNF) e_c1 = a.c1[e_col];
            }
#pragma unroll
            for (int m2 = 0; m2 < MT; ++m2)
                e_rf[m2] = (a.Rf && a.KS == 1) ? a.Rf[((size_t)(m2 * 2 + e_half) * (a.N >> 4) + nt) * 256 + e_in] : 0.f;
            __builtin_amdgcn_sched_barrier(0);
        } else {
            dx_load_frags<MODE>(xa, a, mt, kc0, lane, [] {});
        }
        if (MODE != DX_PLAIN && a.xout && nt == 0 && ks == 0) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < DK_PW; ++c)
                    *reinterpret_cast<f32x4*>(a.xout + ((size_t)((mt * 2 + h) * kchunks + kc0 + c) * 64 + lane) * 4) = xa[h][c];
        }
        f32x4v acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (W16 == 0) {
#pragma unroll
            for (int c = 0; c < DK_PW; ++c) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[0][c][j], w[c][j], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[1][c][j], w[c][j], acc1, 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < DK_PW; ++c) {
                acc0 = dx_mfma_chunk<W16>(xa[0][c], w[c], acc0);
                acc1 = dx_mfma_chunk<W16>(xa[1][c], w[c], acc1);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc[mt][r] = acc0[r]; acc[mt][4 + r] = acc1[r]; }
        if constexpr (LNF) dx_row_stats(xa, st[mt][wave], lane);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (mt > 0) __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r) red[(wave * 8 + r) * 64 + lane] = acc[mt][r];
        __syncthreads();
        // 32 rows x 16 cols = 512 outputs, one per thread.  C/D map of 16x16x4: col = lane & 15, row = (lane >> 4) * 4 + reg
        const int half = tid >> 8, rr = (tid >> 6) & 3, l = tid & 63;
        float v = red[(half * 4 + rr) * 64 + l];
#pragma unroll
        for (int w2 = 1; w2 < SK_WAVES; ++w2) v += red[(w2 * 8 + half * 4 + rr) * 64 + l];
        const int lrow = half * 16 + (l >> 4) * 4 + rr, row = mt * 32 + lrow, col = e_col;
        // position of (row, col) in a fragment-major matrix with N columns
        const size_t fo = ((size_t)(mt * 2 + half) * (a.N >> 4) + nt) * 256 + e_in;
        if (a.KS > 1) {  // K slices 2p, 2p + 1 -> accumulator p (starts at zero: two addends commute exactly)
            unsafeAtomicAdd(a.part_out + ((size_t)((mt * 2 + (ks >> 1)) * 2 + half) * (a.N >> 4) + nt) * 256 + e_in, v + e_bias);
            continue;
        }
        if (a.zero_acc) {
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) a.zero_acc[((size_t)((mt * 2 + pr) * 2 + half) * (a.N >> 4) + nt) * 256 + e_in] = 0.f;
        }
        const bool colok = col < a.N;
        if constexpr (LNF) {
            float mean, rstd;
            dx_row_mean_rstd(st[mt], lrow, a.K, mean, rstd);
            v = rstd * (v - mean * e_c1) + e_bias;
        } else {
            v += e_bias;
        }
        v += e_rf[mt];
        v = apply_act(v, a.act);
        if (a.Y && row < a.M && colok) a.Y[(size_t)row * a.ldy + col] = v;
        if (a.Yf) a.Yf[fo] = row < a.M ? v : 0.f;
        if (a.cand_val) {  // fused arg-max: the 16 columns of `row` in this tile are 16 adjacent lanes; first max wins
            float bv = colok ? v : -INFINITY;
            int bi = col;
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if ((l & 15) == 0 && row < a.M) {
                a.cand_val[(size_t)row * a.NT + nt] = bv;
                a.cand_idx[(size_t)row * a.NT + nt] = bi;
            }
        }
    }
}

// attn_proj' (N = 1024, K = 1024: 64 column tiles, no K split) with ONE ROW HALF per workgroup: grid (64 tiles, 2 halves) =
// 128 workgroups.  With 64 workgroups the kernel is bound by its own fp32 MFMA work - 8 waves x 64 MFMAs, two waves per
// SIMD, 4096 cycles = 2 us after the 64 KiB of weights have long arrived - so each workgroup takes the 16 rows of one
// half (32 MFMAs per wave, 1 us) and the tile's weights are read by two workgroups (4 MB more L2 traffic, free).
// DX_PLAIN, no LayerNorm fold, <= 32 rows, KS == 1: bias + residual (in place) + the accumulator reset of the main kernel.
__global__ __launch_bounds__(512) void rgrg_skinny_direct_half_f32(const DirectArgs a) {
    __shared__ __attribute__((aligned(16))) float red[SK_WAVES * 4 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = blockIdx.x, half = blockIdx.y;
    const int kchunks = a.K >> 4;
    const int kc0 = wave * DK_PW;
    const __amdgpu_buffer_rsrc_t rw = dx_rsrc(a.P), rx = dx_rsrc(a.Xf);
    f32x4 xa[DK_PW], w[DK_PW];
#pragma unroll
    for (int c = 0; c < DK_PW; ++c) xa[c] = dx_ldb(rx, (unsigned)lane * 16u, (unsigned)((half * kchunks + kc0 + c) * 1024));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < DK_PW; ++c) w[c] = dx_ldb_nt(rw, (unsigned)lane * 16u, (unsigned)((nt * kchunks + kc0 + c) * 1024));
    __builtin_amdgcn_sched_barrier(0);
    // epilogue operands of this thread (threads 0..255: one output each), requested behind the weight stream
    const int e_rr = (tid >> 6) & 3, e_l = tid & 63;
    const int e_col = nt * 16 + (e_l & 15);
    const int e_in = (((e_l & 15) >> 2) * 16 + (e_l >> 4) * 4 + e_rr) * 4 + (e_l & 3);
    const size_t fo = ((size_t)half * (a.N >> 4) + nt) * 256 + e_in;
    float e_bias = 0.f, e_rf = 0.f;
    if (tid < 256) {
        if (a.bias && e_col < a.N) e_bias = a.bias[e_col];
        if (a.Rf) e_rf = a.Rf[fo];
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DK_PW; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[c][j], w[c][j], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
    __syncthreads();
    if (tid >= 256) return;
    // 16 rows x 16 cols = 256 outputs.  C/D map of 16x16x4: col = lane & 15, row = (lane >> 4) * 4 + reg
    float v = red[e_rr * 64 + e_l];
#pragma unroll
    for (int w2 = 1; w2 < SK_WAVES; ++w2) v += red[(w2 * 4 + e_rr) * 64 + e_l];
    const int row = half * 16 + (e_l >> 4) * 4 + e_rr;
    if (a.zero_acc) {
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) a.zero_acc[((size_t)(pr * 2 + half) * (a.N >> 4) + nt) * 256 + e_in] = 0.f;
    }
    v = apply_act(v + e_bias + e_rf, a.act);
    if (a.Y && row < a.M && e_col < a.N) a.Y[(size_t)row * a.ldy + e_col] = v;
    if (a.Yf) a.Yf[fo] = row < a.M ? v : 0.f;
}

// lm_head' for <= 32 rows, round 3: ONE WAVE PER COLUMN TILE, the whole K in one accumulation chain.
// The round-2 kernel split K over the 8 waves of a workgroup and walked pairs of tiles, so every pair ended in two
// barriers, an 8-way LDS reduction and an epilogue during which the matrix pipe idled (56.5 us for 206 MB = 3.6 TB/s; the
// fp32 MFMA work alone is 24 us, the HBM stream 33 us).  Here a workgroup stages the combined activation rows ONCE into LDS (32 x 1024
// fp32 = 128 KiB, fragment-major: an A fragment is one conflict-free ds_read_b128) and computes the row statistics; after
// that its 8 waves never synchronise again: each wave walks its own column tiles (tile = wave * 256 + workgroup, + 2048 per
// round: every SIMD gets ~3 tiles), streams the tile's 64 KiB of packed weights through two 8-chunk register buffers with
// 16 KiB in flight, runs the 512 MFMAs of the tile back to back, and finishes the tile alone (folded LayerNorm, logits,
// arg-max candidate) while the next tile's weights are already arriving.  Measured: 52 us (4.0 TB/s), 126.5 vs 127.05 ms
// per image - the weight stream of 2048 concurrent 16-KiB windows tops out near 4 TB/s like the per-layer kernels'.
template <int MODE>
__global__ __launch_bounds__(512) void rgrg_lm_head_wave_f32(const DirectArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lmh_smem[];
    float* xs = lmh_smem;                                                   // [2 halves][64 chunks][64 lanes][4]
    float (*st)[32][2] = reinterpret_cast<float (*)[32][2]>(lmh_smem + 32 * DK_SLICE);  // [8 waves][32 rows][sum, sum of squares]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int KCH = DK_SLICE / 16;  // 64 chunks of 16 k
    const __amdgpu_buffer_rsrc_t rw = dx_rsrc(a.P);
    // this wave's tiles and the first two weight groups of the first one (requested before anything else: HBM)
    const int t0 = wave * 256 + (int)blockIdx.x;
    const int ntl = t0 < a.NT ? (a.NT - 1 - t0) / 2048 + 1 : 0;   // tiles of this wave
    const int ngl = ntl * 8;                                        // weight groups (8 chunks = 8 KiB per wave) of this wave
    f32x4 wa[DK_PW], wb[DK_PW];
    auto load_group = [&](f32x4(&w)[DK_PW], int g) {  // group g of this wave's stream; past the end: the last group again (never used)
        g = g < ngl ? g : ngl - 1;
        const int t = t0 + (g >> 3) * 2048;
#pragma unroll
        for (int c = 0; c < DK_PW; ++c) w[c] = dx_ldb_nt(rw, (unsigned)lane * 16u, (unsigned)((t * KCH + (g & 7) * DK_PW + c) * 1024));
    };
    if (ngl > 0) { load_group(wa, 0); load_group(wb, 1); }
    __builtin_amdgcn_sched_barrier(0);
    // stage the activation rows: linear copy of the fragment-major matrix (+ the two split-K accumulators of the producer)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {   // two passes of 8 float4 per thread and stream (register budget)
        const f32x4* X = reinterpret_cast<const f32x4*>(a.Xf) + pass * 4096;
        f32x4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = X[tid + 512 * q];
        if constexpr (MODE == DX_COMBINE4) {
            const f32x4* P0 = reinterpret_cast<const f32x4*>(a.part) + pass * 4096;
            const f32x4* P1 = P0 + 32 * DK_SLICE / 4;
            f32x4 p0[8], p1[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) { p0[q] = P0[tid + 512 * q]; p1[q] = P1[tid + 512 * q]; }
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (v[q] + p0[q]) + p1[q];   // per element (x + acc01) + acc23, as everywhere
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) reinterpret_cast<f32x4*>(xs)[pass * 4096 + tid + 512 * q] = v[q];
    }
    __syncthreads();
    {   // row statistics in the order of dx_row_stats (wave w: chunks 8w .. 8w+7 of both halves), then over the waves
        f32x4 xa[2][DK_PW];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < DK_PW; ++c) xa[h][c] = reinterpret_cast<const f32x4*>(xs)[(h * KCH + wave * DK_PW + c) * 64 + lane];
        dx_row_stats(xa, st[wave], lane);
    }
    __syncthreads();
    if (ngl == 0) return;
    // mean / rstd of the 8 rows this lane owns in the C/D map (row = half * 16 + (lane >> 4) * 4 + r)
    float mean[2][4], rstd[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) dx_row_mean_rstd(st, h * 16 + (lane >> 4) * 4 + r, a.K, mean[h][r], rstd[h][r]);
    const f32x4* xl0 = reinterpret_cast<const f32x4*>(xs) + lane;
    for (int ti = 0; ti < ntl; ++ti) {
        const int t = t0 + ti * 2048;
        // folded vectors of this lane's column: needed in the tile's epilogue, requested now (every load of the steady state
        // is unconditional - a load under a branch makes hipcc drain the weight prefetch with vmcnt(0))
        const int col = t * 16 + (lane & 15), colc = min(col, a.N - 1);
        const float c1 = a.c1[colc], c2 = a.bias[colc];
        f32x4v acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        // the A fragments are re-read from LDS for every tile: launder the base, or hipcc hoists all 128 reads out of the
        // tile loop (they are loop invariant) and spills 390 registers
        unsigned xoff = 0;
        asm volatile("" : "+v"(xoff));
        const f32x4* xl = xl0 + xoff;
#pragma unroll
        for (int gg = 0; gg < 8; gg += 2) {   // 8 weight groups per tile, two per iteration: buffers wa / wb
#pragma unroll
            for (int c = 0; c < DK_PW; ++c) {
                const int kc = gg * DK_PW + c;
                const f32x4 x0 = xl[kc * 64], x1 = xl[(KCH + kc) * 64];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[j], wa[c][j], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[j], wa[c][j], acc1, 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // the 8 refill loads go out together, right behind the buffer's last MFMA
            load_group(wa, ti * 8 + gg + 2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < DK_PW; ++c) {
                const int kc = (gg + 1) * DK_PW + c;
                const f32x4 x0 = xl[kc * 64], x1 = xl[(KCH + kc) * 64];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[j], wb[c][j], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[j], wb[c][j], acc1, 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            load_group(wb, ti * 8 + gg + 3);
            __builtin_amdgcn_sched_barrier(0);
        }
        // the tile is complete: epilogue of this wave alone (the next tile's first 16 KiB are already in flight)
        const bool colok = col < a.N;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = h * 16 + (lane >> 4) * 4 + r;
                const float sum = h ? acc1[r] : acc0[r];
                const float v = apply_act(rstd[h][r] * (sum - mean[h][r] * c1) + c2, a.act);
                if (a.Y && row < a.M && colok) a.Y[(size_t)row * a.ldy + col] = v;
                if (a.cand_val) {     // the row's 16 columns of this tile sit in the 16 lanes of a DPP row: first max wins
                    float bv = colok ? v : -INFINITY;
                    int bi = col;
#define LMH_STEP(CTRL)                                                                                   \
    {                                                                                                    \
        const float ov = dpp_get<CTRL, 0xf>(bv);                                                         \
        const int oi = __builtin_amdgcn_update_dpp(0, bi, CTRL, 0xf, 0xf, false);                        \
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }                                      \
    }
                    LMH_STEP(0xB1) LMH_STEP(0x4E) LMH_STEP(0x141) LMH_STEP(0x140)   // lanes ^1, ^2, half mirror, row mirror
#undef LMH_STEP
                    if ((lane & 15) == 0 && row < a.M) {
                        a.cand_val[(size_t)row * a.NT + t] = bv;
                        a.cand_idx[(size_t)row * a.NT + t] = bi;
                    }
                }
            }
    }
}
constexpr size_t LMH_LDS = (size_t)(32 * DK_SLICE + SK_WAVES * 32 * 2) * sizeof(float);

// ------------------------------------------------------------------ LayerNorm folding (done once, at load)
// P [NT][K/16][64][4] = (W o g) in the 16-column fragment order (g == null: plain copy - same as pack_weights16_kernel)
__global__ __launch_bounds__(256) void pack_weights16_scaled_kernel(const float* __restrict__ W, const float* __restrict__ g,
                                                                    float* __restrict__ P, int N, int K, int NT) {
    const size_t total = (size_t)NT * (K / 16) * 64;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(o & 63);
        const size_t t = o >> 6;
        const int kc = (int)(t % (K / 16));
        const int nt = (int)(t / (K / 16));
        const int n = nt * 16 + (l & 15), k = kc * 16 + (l >> 4) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (n < N) {
            v = *reinterpret_cast<const f32x4*>(W + (size_t)n * K + k);
            if (g) v *= *reinterpret_cast<const f32x4*>(g + k);
        }
        reinterpret_cast<f32x4*>(P)[o] = v;
    }
}

// c1[n] = sum_k fl(W[n,k] g[k]) (the values the MFMA multiplies), c2[n] = sum_k W[n,k] b[k] + bias[n]; one wave per
// output column, double accumulation, fixed order
__global__ __launch_bounds__(256) void ln_fold_vectors_kernel(const float* __restrict__ W, const float* __restrict__ g,
                                                              const float* __restrict__ b, const float* __restrict__ bias,
                                                              float* __restrict__ c1, float* __restrict__ c2, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    double s1 = 0.0, s2 = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float wv = W[(size_t)n * K + k];
        s1 += (double)(wv * g[k]);
        s2 += (double)wv * (double)b[k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    if (lane == 0) {
        c1[n] = (float)s1;
        c2[n] = (float)(s2 + (bias ? (double)bias[n] : 0.0));
    }
}

// c1 of the 16-bit-weight variant: c1_16[n] = sum_k of the ROUNDED scaled weights, as the matrix core multiplies them (packed16
// [NT][K / 16][64 lanes][4] 16-bit); one workgroup of 64 lanes per column tile, double accumulation, fixed order
__global__ __launch_bounds__(64) void packed16_colsum_kernel(const unsigned short* __restrict__ P16, float* __restrict__ c1, int N, int K, int f16) {
    const int nt = blockIdx.x, lane = threadIdx.x;
    const int kch = K / 16;
    double s = 0.0;
    for (int kc = 0; kc < kch; ++kc) {
        const unsigned short* q = P16 + (((size_t)nt * kch + kc) * 64 + lane) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += (double)from16_rt(q[j], f16);
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    const int n = nt * 16 + (lane & 15);
    if (lane < 16 && n < N) c1[n] = (float)s;
}
