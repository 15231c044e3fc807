// ------------------------------------------------------------------ K-parity ping-pong kernel (round 6): both operands 16-bit
// The kernel of the per-layer projections of the MANY-SEQUENCE decode step (BASELINE configs[2]: M = 923 token rows, or a row
// range of ~300; N = 1024 .. 4096, K = 1024 / 4096).  What bounded gemm_bf16_glds_kernel there (DESIGN.md 5.3, the stage sweeps
// in profiles/r03_gemm_bf16_bench_*): a GEMM of 240 .. 720 tiles of 64 x 64 puts ONE to three 4-wave workgroups on a CU, every
// wave runs   wait -> barrier -> issue its LDS-DMA pieces -> ds_read -> MFMA   strictly one after the other, and with one wave per
// SIMD nothing overlaps: mlp_proj spends ~660 cycles per K tile for 128 cycles of matrix-core work (0.17 of the CU's rate), and the
// texture-address path (64 B / clk / CU) idles two thirds of the time.  Splitting K over workgroups overlaps them but pays a
// cross-workgroup hand-off of 5-13 us (profiles/r05_splitk_decode_ab.log).  Here the two halves live in ONE workgroup:
//   * 8 waves = two GROUPS of four; group g owns the K tiles of parity g (kt = g, g + 2, ...) of the WHOLE BM x BN tile, its four
//     waves are a 2 x 2 grid of (BM / 2) x (BN / 2) sub-tiles of 32x32x16 MFMA blocks; waves w and w + 4 share a SIMD;
//   * PING-PONG: time is cut into slots by workgroup barriers.  In a slot ONE group reads the fragments of its next K tile from
//     LDS into registers (a whole tile: 4 K steps) and issues the LDS-DMA requests of a tile NST - 1 ahead, while the OTHER group
//     issues nothing but the MFMAs of the tile it read one slot earlier - every SIMD has one wave in the matrix core and one on
//     the LDS / DMA side:
//         slot      group 0                      group 1
//         2t        read tile t, request t+NST-1  multiply tile t - 1
//         2t + 1    multiply tile t               read tile t, request t+NST-1
//   * each group has its own NST LDS stages of (BM + BN) x 128 B; a stage is refilled by the reading slot AFTER the one that read
//     it (a barrier lies between), so a request has 2 (NST - 1) slots to land; the wait for tile t + 1 (`vmcnt`, counted: the
//     younger requests keep flying) sits at the end of the multiplying slot of tile t;
//   * at the end group 1 leaves its accumulators in LDS, group 0 adds them (sum of the even K tiles + sum of the odd ones: ONE
//     order, whatever M is) and runs the epilogue of the LDS-DMA kernel (shift / residual / activation / 16-bit output; producer
//     or consumer of a folded LayerNorm).
// Tile shapes (measured, profiles/r06_kp_bench_*_v1.log, r06_kp_ablation_v1.log): 64 x 64 x 4 stages is the one the decoder uses
// (attn_proj / mlp_proj: 240 workgroups at 923 rows; 4 MFMAs per wave and slot against 16 DMA pieces: a slot is ~130 cycles of
// barrier + ~280 of requests / fragment reads, ~0.3 of the CU's matrix rate where the 4-wave kernel reached 0.17; 20.7 -> 16.7 us
// for mlp_proj, 9.7 -> 7.2 / 20.9 -> 15.0 us for the two on a ~300-row range).  128 x 128 x 2 is latency bound (a request has
// two slots to land: 20.6 us for c_fc against 18.8), 128 x 64 x 3 / 64 x 128 x 3 / 64 x 64 x 3 / 64 x 64 x 2 are test and bench
// shapes.  128 KiB of LDS for the shapes that matter: one workgroup per CU.  Selected by the decoder for the many-sequence step
// only (GemmLnFold::kp); the tile is a function of the GEMM, never of M, so a row's bits do not depend on the row range it is
// launched in.
//
// WIDE (64 x 64 producer only: attn_proj / mlp_proj of the step): the epilogue goes through LDS instead of working straight from
// the C layout of the 32x32 MFMA, where a lane owns 16 single elements and every load / store instruction moves 4 (fp32) or 2
// (16-bit) bytes per lane.  Every one of the 512 threads requests 32 bytes of the residual tile (row tid / 8, 8 columns) ahead of
// the operand stream; after the K loop the stages of group 0 are free and hold two 64 x 64 fp32 tiles, residual and result;
// group 0 computes what it always computed (even + odd K tiles, + shift, + residual, to16, the statistics butterfly) but takes
// the residual from the first tile and leaves the value in the second; after the barrier of the statistics exchange all eight
// waves store whole rows, 16 bytes per lane.  ~44 vector-memory instructions per workgroup instead of ~260, same bytes, same
// bits.  The launcher takes it only without an activation (a producer writes the residual stream), so the 16 scalar switches on
// p.act per lane are gone as well - they cost as much as the narrow accesses did.  Measured (profiles/wide_epilogue_ab.md, cold
// weights): attn_proj 9.8 -> 8.8 us and mlp_proj 20.4 -> 19.3 us on a 231-row range, 10.2 -> 9.4 / 20.9 -> 20.3 us at 923 rows;
// the epilogue's share (RGRG_PP_DBG bit 8) 2.7 -> 1.7 / 2.7 -> 1.9 us; 77 -> 73 VGPRs.  RGRG_WIDE_EPI=0 (read per launch)
// keeps the C-layout epilogue.  Tile image: rows of 256 B, the 16-byte chunk c of row r sits at chunk
// c ^ (c >> 3 & 1) ^ (r >> 1 & 1): element accesses in C layout (32 lanes = 32 consecutive floats), the 16-byte writes of a row
// (8 lanes, chunks 2 i + j) and the 16-byte reads (ds_read_b128: lane groups of 4 rows x 4 chunks) are all free of bank conflicts.
__device__ __forceinline__ int kp_wide_off(int row, int chunk) {   // float index of the first element of a 16-byte chunk
    return row * 64 + ((chunk ^ ((chunk >> 3) & 1) ^ ((row >> 1) & 1)) << 2);
}
template <int BM, int BN, int NST, bool F16, int LNF, bool WIDE = false>
__global__ __launch_bounds__(512) void gemm_bf16_kp_kernel(const GemmBf16Params p, const int mtiles, const int ntiles) {
    constexpr int BK = 64;
    constexpr int MI = BM / 64, NI = BN / 64;   // 32x32 MFMA blocks per wave
    constexpr int LA = BM / 32, LB = BN / 32;   // LDS-DMA instructions (1 KiB = 8 rows) per wave per K tile
    constexpr int PPW = LA + LB;
    constexpr int STAGE = (BM + BN) * 128;
    constexpr int GROUP = NST * STAGE;          // LDS of one group
    constexpr int TAG = 2000 + (BM == 128 ? 512 : 0) + (BN == 128 ? 256 : 0) + LNF * 64 + NST * 4 + (F16 ? 1 : 0) + (WIDE ? 2000 : 0);
    static_assert(NST >= 2 && NST <= 4, "tail is written for up to 3 trailing tiles");
    static_assert((NST - 2) * PPW < 64, "counted vmcnt out of range");
    static_assert(4 * MI * NI * 4096 <= GROUP, "group 1's accumulators must fit its own stages");
    static_assert(!WIDE || (BM == 64 && BN == 64 && LNF == 1 && GROUP >= 2 * 64 * 256), "the staged epilogue is the 64 x 64 producer's");
    extern __shared__ __attribute__((aligned(16))) unsigned char kp_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wave >> 2, w4 = wave & 3;
    const int wm = w4 >> 1, wn = w4 & 1;
    const int2 tmn = grouped_tile(xcd_band_tile(blockIdx.x, mtiles * ntiles), p.gm, mtiles, ntiles);
    const int tm = tmn.x, tn = tmn.y;
    const int m0 = tm * BM, n0 = tn * BN;
    const int n = p.K / (2 * BK);               // K tiles per group (the launcher checks K % 128 == 0 and n >= NST)
    const int lda = p.lda ? p.lda : p.K, ldw = p.ldw ? p.ldw : p.K;
    // descriptors rebased to the tile and to the group's first K tile; the group's tile t starts 2 t BK elements further
    const u16* abase = p.A16 + (size_t)m0 * lda + g * BK;
    const u16* wbase = p.Wb + (size_t)n0 * ldw + g * BK;
    const int lrow = lane >> 3, lch = lane & 7;
    int va[LA], vb[LB];
#pragma unroll
    for (int j = 0; j < LA; ++j) {
        const int row = (j * 4 + w4) * 8 + lrow;
        va[j] = dma_src_off(row, p.M - 1 - m0, lda, lch);
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) {
        const int row = (j * 4 + w4) * 8 + lrow;
        vb[j] = dma_src_off(row, p.N - 1 - n0, ldw, lch);
    }
    unsigned char* const gs = kp_smem + g * GROUP;
#define KP_ISSUE(STAGE_, T_) \
    glds_issue<BM, LA, LB, TAG>(abase, wbase, gs + (STAGE_) * STAGE + w4 * 1024, va, vb, (T_) * (4 * BK), (T_) * (4 * BK))
    const int frow = lane & 31, fh = lane >> 5;
    int foff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) foff[ks] = frag_offset(frow, fh, ks);

    f32x16 acc[MI][NI];
    zero_acc(acc);

    // epilogue operands, requested ahead of the operand stream (the oldest loads: the counted waits below are unaffected).
    // Only group 0 uses them; group 1's waves request the same addresses (its twin wave's lines: L1 / L2 hits) so that no load
    // sits under a branch in front of the pipeline (hipcc would drain vmcnt(0) at the join).
    const int ccol = lane & 31, crow4 = 4 * (lane >> 5);
    float sh_pre[MI][NI], cs_pre[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int colc = min(n0 + wn * (BN / 2) + ni * 32 + ccol, p.N - 1);
            sh_pre[mi][ni] = p.shift ? p.shift[colc] : 0.f;
            cs_pre[mi][ni] = LNF == 2 ? p.ln_colsum[colc] : 0.f;
        }
    constexpr bool PRE_R = MI * NI == 1 && LNF != 2 && !WIDE;
    float rv_pre[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rv_pre[r] = 0.f;
    if constexpr (PRE_R) {
        if (p.R) {
            const int colc = min(n0 + wn * (BN / 2) + ccol, p.N - 1);
            const int rbase = m0 + wm * (BM / 2) + crow4;
#pragma unroll
            for (int r = 0; r < 16; ++r) rv_pre[r] = c_load_f32(p.R, rbase, r, colc, p.M, p.ldy);
        }
    }
    // WIDE: this thread's 32 bytes of the residual tile (the launcher checks R, N % 64 == 0 and the alignment)
    const int wrow = tid >> 3, wch = tid & 7;
    f32x4 rw0 = {0.f, 0.f, 0.f, 0.f}, rw1 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (WIDE) {
        const f32x4* rp = reinterpret_cast<const f32x4*>(p.R + (size_t)min(m0 + wrow, p.M - 1) * p.ldy + n0 + wch * 8);
        rw0 = rp[0]; rw1 = rp[1];
    }
    constexpr int TPR = 256 / BM, PER = 16 / TPR;   // consumer of a folded LayerNorm: 16 statistics slots per row
    f32x4 lsq[PER / 2];
    if constexpr (LNF == 2) {
        const int t8 = tid & 255;
        const int srow = min(m0 + t8 / TPR, p.M - 1);
        const f32x4* sp = reinterpret_cast<const f32x4*>(p.ln_stats + ((size_t)srow * 16 + (t8 % TPR) * PER) * 2);
#pragma unroll
        for (int j = 0; j < PER / 2; ++j) lsq[j] = sp[j];
    }

    bf16x8 fa[4][MI], fb[4][NI];
    const int dbg = __builtin_amdgcn_readfirstlane(p.dbg);   // measurements only (RGRG_PP_DBG): 1 no fragment reads, 2 no DMA, 4 no MFMAs, 8 no epilogue
    if (dbg) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[ks][i] = dbg_frag_a();
#pragma unroll
            for (int i = 0; i < NI; ++i) fb[ks][i] = dbg_frag_b();
        }
    }
#define KP_READ(STAGE_)                                                                                              \
    if (!(dbg & 1)) {                                                                                                                \
        const unsigned char* sa_ = gs + (STAGE_) * STAGE + wm * (BM / 2) * 128;                                      \
        const unsigned char* sw_ = gs + (STAGE_) * STAGE + BM * 128 + wn * (BN / 2) * 128;                           \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                                           \
            _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                                        \
                fa[ks][mi] = *reinterpret_cast<const bf16x8*>(sa_ + mi * 4096 + foff[ks]);                           \
            _Pragma("unroll") for (int ni = 0; ni < NI; ++ni)                                                        \
                fb[ks][ni] = *reinterpret_cast<const bf16x8*>(sw_ + ni * 4096 + foff[ks]);                           \
        }                                                                                                            \
    }
#define KP_MUL()                                                                                                     \
    if (!(dbg & 4)) {                                                                                                                \
        __builtin_amdgcn_s_setprio(1);                                                                               \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                                             \
            _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                                        \
                _Pragma("unroll") for (int ni = 0; ni < NI; ++ni)                                                    \
                    acc[mi][ni] = mfma16<F16>(fa[ks][mi], fb[ks][ni], acc[mi][ni]);                                  \
        __builtin_amdgcn_s_setprio(0);                                                                               \
    }
#define KP_BAR()                                  \
    {                                             \
        __builtin_amdgcn_sched_barrier(0);        \
        __builtin_amdgcn_s_barrier();             \
        __builtin_amdgcn_sched_barrier(0);        \
    }
    // the two slots of one K tile of a group: read (+ request tile T_ + NST - 1 into the stage read one tile ago), multiply
    // (+ wait until all but the WAIT_ youngest requests of this wave have landed: tile T_ + 1 is complete after the barrier)
#define KP_TILE(DO_ISSUE_, WAIT_)                                                   \
    {                                                                               \
        KP_READ(cur)                                                                \
        if ((DO_ISSUE_) && !(dbg & 2)) KP_ISSUE(nxt, kt + NST - 1);                               \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                          \
        KP_BAR()                                                                    \
        KP_MUL()                                                                    \
        wait_vmcnt<(WAIT_)>();                                                      \
        KP_BAR()                                                                    \
        cur = cur + 1 == NST ? 0 : cur + 1;                                         \
        nxt = nxt + 1 == NST ? 0 : nxt + 1;                                         \
    }

    // prologue: tiles 0 .. NST - 2 of the wave's own group in flight
#pragma unroll
    for (int s = 0; s < NST - 1; ++s) if (!(dbg & 2)) KP_ISSUE(s, s);
    if (g == 1) KP_BAR()                 // group 1 starts one slot later (slot 0: group 0 reads its tile 0)
    wait_vmcnt<(NST - 2) * PPW>();       // this wave's pieces of its group's tile 0 have landed
    KP_BAR()
    {
        int kt = 0, cur = 0, nxt = NST - 1;
        for (; kt + NST - 1 < n; ++kt) KP_TILE(true, (NST - 2) * PPW)
        // tail: the last NST - 1 tiles, nothing left to request
        if constexpr (NST - 1 >= 1) { KP_TILE(false, (NST - 3 > 0 ? NST - 3 : 0) * PPW) ++kt; }
        if constexpr (NST - 1 >= 2) { KP_TILE(false, (NST - 4 > 0 ? NST - 4 : 0) * PPW) ++kt; }
        if constexpr (NST - 1 >= 3) { KP_TILE(false, 0) ++kt; }
    }
    if (g == 0) KP_BAR()                 // slot 2 n: group 1 multiplies its last tile
#undef KP_TILE
#undef KP_BAR
#undef KP_MUL
#undef KP_READ
#undef KP_ISSUE

    // group 1 -> LDS (its own stages: its last read lies two barriers back) -> group 0
    {
        f32x4* dump = reinterpret_cast<f32x4*>(kp_smem + GROUP) + (size_t)w4 * (MI * NI * 4 * 64) + lane;
        if (g == 1) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        dump[((mi * NI + ni) * 4 + q) * 64] = f32x4{acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2], acc[mi][ni][4 * q + 3]};
        }
        if constexpr (WIDE) {   // all eight waves: the residual tile into group 0's stages (its last read lies two barriers back)
            if (!(dbg & 8)) {
                float* rt = reinterpret_cast<float*>(kp_smem);
                *reinterpret_cast<f32x4*>(rt + kp_wide_off(wrow, 2 * wch)) = rw0;
                *reinterpret_cast<f32x4*>(rt + kp_wide_off(wrow, 2 * wch + 1)) = rw1;
            }
        }
        __syncthreads();
        if (g == 0) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 o = dump[((mi * NI + ni) * 4 + q) * 64];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[mi][ni][4 * q + e] += o[e];
                    }
        }
    }

    if (dbg & 8) return;   // measurements only: no epilogue (nothing is written)
    // ---- epilogue: group 0's four waves, the formulas and orders of gemm_bf16_glds_kernel through the same helpers
    // (gemm_bf16_device.h); the workgroup barriers are passed by all eight waves
    float2* row_stat = reinterpret_cast<float2*>(kp_smem + 2 * GROUP);   // [BM]
    if constexpr (LNF == 2) {
        const float2 ls = ln_slot_sums<TPR, PER>(lsq);
        const float mean = ln_mean(ls.x), var = ln_var(ls.y, mean);
        if (g == 0 && tid % TPR == 0) row_stat[tid / TPR] = make_float2(mean, 1.0f / sqrtf(var + LN_EPS16));
        __syncthreads();
    }

    float blk1[MI], blk2[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) { blk1[mi] = 0.f; blk2[mi] = 0.f; }
    // WIDE: the lane's elements in the two LDS tiles (C layout: rows crow4 + dr of the wave's 32, column ccol); the row bit of
    // the chunk swizzle is bit 1 of dr
    float* const wide_res = reinterpret_cast<float*>(kp_smem);
    float* const wide_out = wide_res + 64 * 64;
    const int wide_c = wn * 8 + (ccol >> 2);
    const int wide_e0 = (wm * 32 + crow4) * 64 + ((wide_c ^ wn) << 2) + (ccol & 3);
    const int wide_e1 = (wm * 32 + crow4) * 64 + ((wide_c ^ wn ^ 1) << 2) + (ccol & 3);
    if (g == 0) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int col = n0 + wn * (BN / 2) + ni * 32 + ccol;
                const int colc = min(col, p.N - 1);
                const int rbase = m0 + wm * (BM / 2) + mi * 32 + crow4;
                const float sh = sh_pre[mi][ni];
                float rv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) rv[r] = rv_pre[r];
                if constexpr (WIDE) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) rv[r] = wide_res[((r & 2) ? wide_e1 : wide_e0) + c_row(r) * 64];
                }
                if (!PRE_R && !WIDE && LNF != 2 && p.R) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) rv[r] = c_load_f32(p.R, rbase, r, colc, p.M, p.ldy);
                }
                float vv[16];
                if constexpr (LNF == 2) {
                    const float cs = cs_pre[mi][ni];
                    const int lrow0 = wm * (BM / 2) + mi * 32 + crow4;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float2 st = row_stat[c_row(r, lrow0)];
                        vv[r] = apply_act_fast(st.y * (acc[mi][ni][r] - st.x * cs) + sh + rv[r], p.act);
                    }
                } else if constexpr (WIDE) {   // no activation (the launcher checks): 16 scalar switches on p.act less
#pragma unroll
                    for (int r = 0; r < 16; ++r) vv[r] = acc[mi][ni][r] + sh + rv[r];
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) vv[r] = apply_act_fast(acc[mi][ni][r] + sh + rv[r], p.act);
                }
                if constexpr (WIDE) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) wide_out[((r & 2) ? wide_e1 : wide_e0) + c_row(r) * 64] = vv[r];
                } else if (col < p.N) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (rbase + c_row(r) < p.M) c_store<F16, false, LNF == 1>(c_offset(rbase, r, col, p.ldy), vv[r], p.Y16, p.N, p.Y, p.Yb16);
                }
                if constexpr (LNF == 1) {
                    const float2 bs = ln_block_row_sums(vv, lane);
                    blk1[mi] += bs.x;
                    blk2[mi] += bs.y;
                }
            }
    }
    if constexpr (LNF == 1) {
        float2* xch = reinterpret_cast<float2*>(kp_smem + 2 * GROUP);   // [4 waves][MI][32 rows]
        const int lrow_s = ln_block_sum_row(lane);
        if constexpr (NI == 1) {
            if (g == 0 && wn == 1 && !(lane & 1)) ln_stats_hand_over<MI>(xch, w4, lrow_s, blk1, blk2);
            __syncthreads();
        }
        if constexpr (WIDE) {   // all eight waves: whole rows of the finished tile, 8 columns per thread
            const f32x4 o0 = *reinterpret_cast<const f32x4*>(wide_out + kp_wide_off(wrow, 2 * wch));
            const f32x4 o1 = *reinterpret_cast<const f32x4*>(wide_out + kp_wide_off(wrow, 2 * wch + 1));
            if (m0 + wrow < p.M) {
                const size_t o = (size_t)(m0 + wrow) * p.ldy + n0 + wch * 8;
                *reinterpret_cast<f32x4*>(p.Y + o) = o0;
                *reinterpret_cast<f32x4*>(p.Y + o + 4) = o1;
                u32x4 h;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    h[e] = (unsigned)(u16)to16<F16>(o0[2 * e]) | ((unsigned)(u16)to16<F16>(o0[2 * e + 1]) << 16);
                    h[2 + e] = (unsigned)(u16)to16<F16>(o1[2 * e]) | ((unsigned)(u16)to16<F16>(o1[2 * e + 1]) << 16);
                }
                *reinterpret_cast<u32x4*>(p.Yb16 + o) = h;
            }
        }
        if (g == 0 && !(lane & 1) && (NI == 2 || wn == 0))
            ln_stats_store<MI, NI>(xch, w4, lrow_s, blk1, blk2, m0 + wm * (BM / 2), NI == 2 ? (n0 + wn * 64) / 64 : n0 / 64, p.M, p.stats_out);
    }
}

template <int BM, int BN, int NST>
static gemm_kernel_t kp_kernel(const GemmVariant& v) {
#define RGRG_KP_KERNEL(...) (v.f16 ? gemm_bf16_kp_kernel<BM, BN, NST, true, __VA_ARGS__> : gemm_bf16_kp_kernel<BM, BN, NST, false, __VA_ARGS__>)
    if (v.conv || v.cact != -1) return nullptr;
    if (v.wide) {
        if constexpr (BM == 64 && BN == 64) { if (v.lnf == 1) return RGRG_KP_KERNEL(1, true); }
        return nullptr;
    }
    switch (v.lnf) {
        case 0: return RGRG_KP_KERNEL(0);
        case 1: return RGRG_KP_KERNEL(1);
        case 2: return RGRG_KP_KERNEL(2);
    }
#undef RGRG_KP_KERNEL
    return nullptr;
}
template <int BM, int BN, int NST>
constexpr int kp_lds() { return 2 * NST * (BM + BN) * 128 + BM * 16; }
template <int BM, int BN, int NST>
static int kp_attr() { return set_dynamic_lds(kp_kernel<BM, BN, NST>, kp_lds<BM, BN, NST>()); }

// plain, producer (Yb16 + stats_out) or consumer (ln_stats + ln_colsum) of a folded LayerNorm; no convolution, no 16-bit
// residual, no training epilogues, no split-K, no arg-max candidates
static bool kp_eligible(const GemmBf16Params& p, int nst) {
    return !p.cCin && !p.R16 && !p.Ypre16 && !p.G16 && !p.cand_val && p.ksplit <= 1 && p.K % 128 == 0 && p.K / 128 >= nst &&
           !(p.ln_colsum && p.R);
}

// RGRG_WIDE_EPI, read per launch like RGRG_PP_DBG (A/B runs and tests compare both epilogues in one process): unset or 1 = the
// 64 x 64 producer stages its tile in LDS and stores whole rows (WIDE above), 0 = the epilogue that works from the C layout
static std::atomic<int> kp_wide_launches{0};   // rgrg_debug_wide_epilogue_launches
static bool kp_wide_enabled() {
    const char* e = getenv("RGRG_WIDE_EPI");
    return !e || (atoi(e) & 1) != 0;
}
// the staged epilogue moves 16-byte pieces of whole 64-column rows: fp32 residual in, fp32 and 16-bit result out, no activation
// (a producer writes the residual stream)
static bool kp_wide_ok(const GemmBf16Params& p) {
    const auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    return p.Yb16 && p.stats_out && p.R && p.Y && !p.Y16 && p.act == RGRG_ACT_NONE && p.N % 64 == 0 && p.ldy % 8 == 0 && al16(p.R) && al16(p.Y) && al16(p.Yb16);
}

template <int BM, int BN, int NST>
static int launch_kp_cfg(const GemmBf16Params& p0, hipStream_t st) {
    GemmBf16Params p = p0;
    if (!kp_eligible(p, NST)) { set_error("bf16 GEMM: the K-parity kernel does not take this variant"); return RGRG_EINVAL; }
    const int mtiles = (p.M + BM - 1) / BM, ntiles = (p.N + BN - 1) / BN;
    if (p.gm == 0) p.gm = default_gm(mtiles, 16);
    p.dbg = pp_dbg_env();
    GemmVariant v;
    v.f16 = p.f16 != 0;
    if constexpr (BM == 64 && BN == 64) v.wide = kp_wide_enabled() && kp_wide_ok(p);
    if (v.wide) {
        kp_wide_launches.fetch_add(1, std::memory_order_relaxed);
        v.lnf = 1;
    }
    else if (p.Yb16) v.lnf = 1;
    else if (p.ln_colsum) v.lnf = 2;
    return launch_variant(kp_kernel<BM, BN, NST>(v), mtiles * ntiles, 512, kp_lds<BM, BN, NST>(), p, mtiles, ntiles, st);
}

// the K-parity tile of a GEMM: a function of (N, K) only - never of M (a row's bits must not depend on the row range)
// ------------------------------------------------------------------ row-split ping-pong kernel, 128 x 128 (round 6)
// c_attn / c_fc of the many-sequence decode step (N = 3072 / 4096, K = 1024): 192 / 256 tiles of 128 x 128 at 923 rows - half the
// L2 -> LDS bytes per flop of the 64 x 64 tiles these GEMMs ran on (every request sits in the CU's memory pipeline that the
// HBM-bound attention of the other row ranges needs too: profiles/r06_overlap_probe_*.log), one workgroup per CU.  The
// 256 x 256 ping-pong kernel scaled down: 8 waves = two groups; group g owns ROWS g * 64 .. + 64 of the tile, wave wq of a group the
// columns wq * 32 .. + 32 (2 x 1 blocks of 32x32x16); both groups walk ALL K tiles, one slot apart:
//         slot      group 0                               group 1
//         2kt       read tile kt, request W of kt + 3      multiply tile kt - 1
//         2kt + 1   multiply tile kt                       read tile kt, request A of kt + 3
// four shared LDS stages of (128 + 128) x 128 B; the stage of tile kt is free after slot 2kt + 1 and refilled (tile kt + 4) by
// the reading slots of tile kt + 1, so a request has 5 / 4 slots to land; the K order of a row's sum is the LDS-DMA kernel's
// (one accumulator per block, K tiles in order) - same bits - and there is no reduction at the end: all eight waves run the
// epilogue of their own 64 x 32 piece.  Plain, or consumer of a folded LayerNorm.
template <int TAG>
__device__ __forceinline__ void pr_dma4(const u16* base, unsigned char* dst, const int (&v)[4], int soff) {
    const __amdgpu_buffer_rsrc_t r = bf16_rsrc(base);
#pragma unroll
    for (int j = 0; j < 4; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)(dst + j * 4096), 16, v[j], soff, 0, 0);
}
template <bool F16, int LNF>
__global__ __launch_bounds__(512) void gemm_bf16_pr_kernel(const GemmBf16Params p, const int mtiles, const int ntiles) {
    constexpr int BM = 128, BN = 128, BK = 64, NST = 4;
    constexpr int STAGE = (BM + BN) * 128, WOFF = BM * 128;
    constexpr int TAG = 3000 + LNF * 2 + (F16 ? 1 : 0);
    static_assert(LNF == 0 || LNF == 2, "plain or consumer");
    extern __shared__ __attribute__((aligned(16))) unsigned char pr_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wave >> 2, wq = wave & 3;
    const int2 tmn = grouped_tile(xcd_band_tile(blockIdx.x, mtiles * ntiles), p.gm, mtiles, ntiles);
    const int tm = tmn.x, tn = tmn.y;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nk = p.K / BK;                    // the launcher checks nk >= 4
    const int lda = p.lda ? p.lda : p.K, ldw = p.ldw ? p.ldw : p.K;
    // group 0's waves request W rows, group 1's A rows: 4 pieces of 8 rows per wave and K tile
    const u16* obase = g == 0 ? p.Wb + (size_t)n0 * ldw : p.A16 + (size_t)m0 * lda;
    const int olim = g == 0 ? p.N - 1 - n0 : p.M - 1 - m0, old_ = g == 0 ? ldw : lda;
    const int lrow = lane >> 3, lch = lane & 7;
    int vo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (j * 4 + wq) * 8 + lrow;
        vo[j] = dma_src_off(row, olim, old_, lch);
    }
    unsigned char* const odst = pr_smem + (g == 0 ? WOFF : 0) + wq * 1024;
#define PR_ISSUE(KT_) pr_dma4<TAG>(obase, odst + ((KT_) & 3) * STAGE, vo, (KT_) * (BK * 2))
    const int frow = lane & 31, fh = lane >> 5;
    int foff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) foff[ks] = frag_offset(frow, fh, ks);
    const unsigned char* const fa_base = pr_smem + g * (64 * 128);
    const unsigned char* const fb_base = pr_smem + WOFF + wq * (32 * 128);

    f32x16 acc[2][1];   // 2 x 1 blocks per wave
    zero_acc(acc);
    // epilogue operands ahead of the operand stream
    const int ccol = lane & 31, crow4 = 4 * (lane >> 5);
    const int col = n0 + wq * 32 + ccol, colc = min(col, p.N - 1);
    const float sh = p.shift ? p.shift[colc] : 0.f;
    const float cs = LNF == 2 ? p.ln_colsum[colc] : 0.f;
    f32x4 lsq[4];
    if constexpr (LNF == 2) {   // 2 threads per row (of the first 256; the second half repeats them), 8 slots each
        const int t8 = tid & 255;
        const int srow = min(m0 + (t8 >> 1), p.M - 1);
        const f32x4* sp = reinterpret_cast<const f32x4*>(p.ln_stats + ((size_t)srow * 16 + (t8 & 1) * 8) * 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) lsq[j] = sp[j];
    }
    bf16x8 fa[4][2], fb[4];
    const int dbg = __builtin_amdgcn_readfirstlane(p.dbg);
    if (dbg) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { fa[ks][0] = fa[ks][1] = dbg_frag_a(); fb[ks] = dbg_frag_b(); }
    }
#define PR_READ(KT_)                                                                                 \
    if (!(dbg & 1)) {                                                                                \
        const unsigned char* sa_ = fa_base + ((KT_) & 3) * STAGE;                                    \
        const unsigned char* sw_ = fb_base + ((KT_) & 3) * STAGE;                                    \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                           \
            fa[ks][0] = *reinterpret_cast<const bf16x8*>(sa_ + foff[ks]);                            \
            fa[ks][1] = *reinterpret_cast<const bf16x8*>(sa_ + 4096 + foff[ks]);                     \
            fb[ks] = *reinterpret_cast<const bf16x8*>(sw_ + foff[ks]);                               \
        }                                                                                            \
    }
#define PR_MUL()                                                                                     \
    if (!(dbg & 4)) {                                                                                \
        __builtin_amdgcn_s_setprio(1);                                                               \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                           \
            acc[0][0] = mfma16<F16>(fa[ks][0], fb[ks], acc[0][0]);                                   \
            acc[1][0] = mfma16<F16>(fa[ks][1], fb[ks], acc[1][0]);                                   \
        }                                                                                            \
        __builtin_amdgcn_s_setprio(0);                                                               \
    }
#define PR_BAR()                                  \
    {                                             \
        __builtin_amdgcn_sched_barrier(0);        \
        __builtin_amdgcn_s_barrier();             \
        __builtin_amdgcn_sched_barrier(0);        \
    }
#define PR_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
    // prologue: this wave's pieces of tiles 0, 1, 2
    if (!(dbg & 2)) { PR_ISSUE(0); PR_ISSUE(1); PR_ISSUE(2); }
    wait_vmcnt<8>();
    PR_BAR()
    if (g == 0) {
        // reading slot 2kt, multiplying slot 2kt + 1 (its end: this wave's pieces of tile kt + 1 have landed)
#define PR_G0(DO_, WAIT_)                                             \
        {                                                             \
            PR_READ(kt)                                               \
            if ((DO_) && !(dbg & 2)) PR_ISSUE(kt + 3);                \
            PR_LGKM0();                                               \
            PR_BAR()                                                  \
            PR_MUL()                                                  \
            wait_vmcnt<(WAIT_)>();                                    \
            PR_BAR()                                                  \
        }
        int kt = 0;
        for (; kt < nk - 3; ++kt) PR_G0(1, 8)
        PR_G0(0, 4) ++kt;
        PR_G0(0, 0) ++kt;
        PR_G0(0, 0)
#undef PR_G0
        PR_BAR()                                  // slot 2 nk: group 1 multiplies the last tile
    } else {
        PR_BAR()                                  // slot 0: group 0 reads tile 0
        // reading slot 2kt + 1 (its end: pieces of tile kt + 1 landed), multiplying slot 2kt + 2
#define PR_G1(DO_, WAIT_)                                             \
        {                                                             \
            PR_READ(kt)                                               \
            if ((DO_) && !(dbg & 2)) PR_ISSUE(kt + 3);                \
            PR_LGKM0();                                               \
            wait_vmcnt<(WAIT_)>();                                    \
            PR_BAR()                                                  \
            PR_MUL()                                                  \
            PR_BAR()                                                  \
        }
        int kt = 0;
        for (; kt < nk - 3; ++kt) PR_G1(1, 8)
        PR_G1(0, 4) ++kt;
        PR_G1(0, 0) ++kt;
        PR_G1(0, 0)
#undef PR_G1
    }
#undef PR_LGKM0
#undef PR_BAR
#undef PR_MUL
#undef PR_READ
#undef PR_ISSUE

    float2* row_stat = reinterpret_cast<float2*>(pr_smem + NST * STAGE);   // [128]
    if constexpr (LNF == 2) {
        // 128-row tile (ln_slot_sums): a thread adds two groups of four slots, the pair of a row meets by shuffle
        const float2 ls = ln_slot_sums<2, 8>(lsq);
        const float mean = ln_mean(ls.x), var = ln_var(ls.y, mean);
        if (tid < 256 && !(tid & 1)) row_stat[tid >> 1] = make_float2(mean, 1.0f / sqrtf(var + LN_EPS16));
        __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int lrow0 = g * 64 + mi * 32 + crow4;
        const int rbase = m0 + lrow0;
        float rv[16], vv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = 0.f;
        if (LNF != 2 && p.R) {
#pragma unroll
            for (int r = 0; r < 16; ++r) rv[r] = c_load_f32(p.R, rbase, r, colc, p.M, p.ldy);
        }
        if constexpr (LNF == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float2 st = row_stat[c_row(r, lrow0)];
                vv[r] = apply_act_fast(st.y * (acc[mi][0][r] - st.x * cs) + sh + rv[r], p.act);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) vv[r] = apply_act_fast(acc[mi][0][r] + sh + rv[r], p.act);
        }
        if (col < p.N) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (rbase + c_row(r) < p.M) c_store<F16, false, false>(c_offset(rbase, r, col, p.ldy), vv[r], p.Y16, p.N, p.Y, p.Yb16);
        }
    }
}

constexpr int PR_LDS = 4 * (128 + 128) * 128 + 128 * 8;
static gemm_kernel_t pr_kernel(const GemmVariant& v) {
    if (v.conv || v.cact != -1 || v.wide) return nullptr;
    if (v.lnf == 0) return v.f16 ? gemm_bf16_pr_kernel<true, 0> : gemm_bf16_pr_kernel<false, 0>;
    if (v.lnf == 2) return v.f16 ? gemm_bf16_pr_kernel<true, 2> : gemm_bf16_pr_kernel<false, 2>;
    return nullptr;
}
static bool pr_eligible(const GemmBf16Params& p) {
    return !p.cCin && !p.R16 && !p.Ypre16 && !p.G16 && !p.cand_val && !p.Yb16 && p.ksplit <= 1 && p.K % 64 == 0 && p.K / 64 >= 4 && !(p.ln_colsum && p.R);
}
static int launch_pr(const GemmBf16Params& p0, hipStream_t st) {
    GemmBf16Params p = p0;
    if (!pr_eligible(p)) { set_error("bf16 GEMM: the row-split ping-pong kernel does not take this variant"); return RGRG_EINVAL; }
    const int mtiles = (p.M + 127) / 128, ntiles = (p.N + 127) / 128;
    if (p.gm == 0) p.gm = default_gm(mtiles, 16);
    p.dbg = pp_dbg_env();
    GemmVariant v;
    v.f16 = p.f16 != 0;
    v.lnf = p.ln_colsum ? 2 : 0;
    return launch_variant(pr_kernel(v), mtiles * ntiles, 512, PR_LDS, p, mtiles, ntiles, st);
}

// The tile of a many-sequence decode projection: a function of (N, K) only - never of M (a row's bits must not depend on the row
// range it is launched in): c_attn / c_fc (N >= 2048) on the 128 x 128 row-split kernel, attn_proj / mlp_proj (N = 1024) on the
// 64 x 64 x 4 K-parity kernel (profiles/r06_kp_bench_*.log).
static int launch_kp_auto(const GemmBf16Params& p, hipStream_t st) {
    if (p.N >= 2048 && pr_eligible(p)) return launch_pr(p, st);
    static const int nst = [] { const char* e = getenv("RGRG_KP_NST"); return e ? atoi(e) : 4; }();   // A/B runs: 2 / 3 / 4 stages per group
    if (nst == 2) return launch_kp_cfg<64, 64, 2>(p, st);
    if (nst == 3) return launch_kp_cfg<64, 64, 3>(p, st);
    return launch_kp_cfg<64, 64, 4>(p, st);
}
