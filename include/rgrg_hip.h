/* rgrg_hip.h - C ABI of librgrg_hip.so: the MI355X (gfx950) kernels behind the RGRG
 * inference hot path (ttanida/rgrg ReportGenerationModel.generate).
 *
 * The reference has no FFI of its own: its hot path sits behind a Python nn.Module
 * API and delegates the arithmetic to torch / torchvision /
 * transformers ops.  Each entry point below replaces the op (or op group) the
 * reference reaches at the cited file:line.  All pointers are DEVICE pointers
 * (fp32 unless stated), all tensors are dense row-major with the layout written
 * next to them, `stream` is a hipStream_t passed as void*, every function returns
 * 0 on success (RGRG_OK) or a negative RGRG_E* code and never allocates or
 * synchronises unless its comment says so.  Activations are NHWC ("channels
 * last"); weight repacking into the layouts named here is done once at load time
 * by the host side (rgrg_amd/engine.py: HipEngine.__init__ and its _pack_* helpers).
 */
#ifndef RGRG_HIP_H_
#define RGRG_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGRG_OK 0
#define RGRG_EINVAL (-1) /* bad shape / argument */
#define RGRG_EHIP (-2)   /* a HIP call failed; see rgrg_last_error() */
#define RGRG_ESTATE (-3) /* handle used in the wrong state */

/* activation codes for the GEMM epilogue */
#define RGRG_ACT_NONE 0
#define RGRG_ACT_RELU 1
#define RGRG_ACT_GELU_NEW 2 /* 0.5x(1+tanh(sqrt(2/pi)(x+0.044715x^3))) - HF NewGELUActivation */

const char* rgrg_last_error(void);
int rgrg_abi_version(void);
/* gfx arch name of device `dev` into buf (e.g. "gfx950"); RGRG_EHIP if no device. */
int rgrg_device_arch(int dev, char* buf, int buflen);

/* ---------------------------------------------------------------------------------
 * Dense / implicit-GEMM fp32 contraction on the f32 MFMA (v_mfma_f32_32x32x2_f32).
 *   Y[m,n] = act( (sum_k A(m,k) * W[n,k]) * scale[n] + shift[n] + R[m,n] )
 * scale may be NULL (=1), shift may be NULL (=0; it carries either the bias or the
 * folded BatchNorm shift), R may be NULL.  K % 32 == 0.  `ws` is only needed when
 * splitk > 1 (splitk*M*N floats).
 *
 * rgrg_linear_f32: A is [M,K] row-major (lda = K), W is [N,K] (nn.Linear layout).
 *   replaces F.linear / torch.addmm at: box_head fc6/fc7, box_predictor
 *   (src/object_detector/custom_roi_heads.py:235-236), dim_reduction (:264),
 *   BinaryClassifierRegionSelection.classifier
 *   (src/binary_classifier/binary_classifier_region_selection.py:32), and - when
 *   more than 32 sequences decode together - Conv1DWithTrainedWeights.forward
 *   (src/language_model/language_model.py:25-29), GPT2MLP, uk/uv (:142-143),
 *   feature_space_transformation_nn (:284) and lm_head (:366).
 * rgrg_conv2d_nhwc_f32: A is the im2col view of X[B,H,W,Cin]; W is
 *   [Cout][KH][KW][Cin]; Y is [B,OH,OW,Cout]; Cin % 32 == 0.
 *   replaces nn.Conv2d + eval BatchNorm2d + ReLU (+ residual add) of the ResNet-50
 *   trunk (src/object_detector/object_detector.py:51-62,219) and the RPNHead convs
 *   (src/object_detector/custom_rpn.py:61).
 * --------------------------------------------------------------------------------- */
int rgrg_linear_f32(const float* A, const float* W, const float* scale, const float* shift, const float* R,
                    float* Y, int M, int N, int K, int ldy, int act, int splitk, float* ws, void* stream);
int rgrg_conv2d_nhwc_f32(const float* X, const float* W, const float* scale, const float* shift, const float* R,
                         float* Y, int B, int H, int Wd, int Cin, int Cout, int KH, int KW, int stride, int pad,
                         int act, int splitk, float* ws, void* stream);

/* ResNet stem: Conv2d(1,64,7,stride 2,pad 3,bias=False) + eval BN + ReLU
 * (object_detector.py:54), X [B,H,W] (1 channel), Wt [49][64] (tap-major), Y [B,H/2,W/2,64]. */
int rgrg_stem_conv7x7_f32(const float* X, const float* Wt, const float* scale, const float* shift, float* Y,
                          int B, int H, int Wd, void* stream);
/* nn.MaxPool2d(3, stride 2, pad 1) on NHWC (resnet50 child 3).  C % 4 == 0. */
int rgrg_maxpool3x3s2_nhwc_f32(const float* X, float* Y, int B, int H, int Wd, int C, void* stream);

/* ---------------------------------------------------------------------------------
 * RPN proposal generation for a single 16x16 feature level (custom_rpn.py:62-71 +
 * torchvision 0.13.1 AnchorGenerator / BoxCoder(1,1,1,1).decode / filter_proposals):
 * per image top-`pre_nms` of the A*H*W objectness logits (ties: lower index first),
 * sigmoid, decode, clip to [0,img_w]x[0,img_h], drop w/h < min_size, greedy NMS
 * (IoU > nms_thresh), first `post_nms` survivors in score order.
 *   head_out [B, HW, 5*A]: per location A objectness logits then A*4 deltas (a*4+c)
 *   anchors  [HW*A, 4] (x1,y1,x2,y2), index = loc*A + a
 *   proposals [B, post_nms, 4] (rows >= count are zero), counts int32 [B],
 *   offsets int32 [B+1] = exclusive prefix sum of counts.
 * pre_nms <= 1000, post_nms <= pre_nms, HW*A <= 65536.
 * --------------------------------------------------------------------------------- */
int rgrg_rpn_proposals_f32(const float* head_out, const float* anchors, float* proposals, int32_t* counts,
                           int32_t* offsets, int B, int HW, int A, int pre_nms, int post_nms, float nms_thresh,
                           float min_size, float img_w, float img_h, void* stream);

/* torchvision.ops.roi_align(aligned=False, sampling_ratio=2, output 8x8) fused with
 * AvgPool2d(8) (custom_roi_heads.py:232,253): feat NHWC [B,FH,FW,C] (C % 128 == 0,
 * FH*FW*128*4 bytes of LDS <= 128 KiB), RoIs = rows [offsets[b], offsets[b+1]) of
 * image b taken from proposals[b].  out [R, 64, C] (bin-major, channel-minor: the
 * fc6 weight is repacked to match), pooled [R, C].  R_total = offsets[B] (host copy). */
int rgrg_roi_align_avgpool_f32(const float* feat, const float* proposals, const int32_t* offsets, float* out,
                               float* pooled, int B, int FH, int FW, int C, int max_props, int R_total,
                               float spatial_scale, void* stream);
/* The same with the [R, 64, C] maps stored as 16-bit values (fp16 = 0: bf16, 1: float16; round to nearest even; pooled stays
 * f32 from unrounded values): what the box head consumes under torch.autocast (generate_reports_for_images.py:108) - fc6
 * then runs on rgrg_linear_bf16_f32 with half the A bytes. */
int rgrg_roi_align_avgpool_bf16maps(const float* feat, const float* proposals, const int32_t* offsets, uint16_t* out16,
                                    float* pooled, int B, int FH, int FW, int C, int max_props, int R_total,
                                    float spatial_scale, int fp16, void* stream);

/* CustomRoIHeads.get_top_region_features_detections_class_detected
 * (custom_roi_heads.py:63-208), eval: pred [R, ldp] holds 30 class logits then 120
 * box deltas per RoI; outputs class_detected uint8 [B,29], top_scores [B,29],
 * top_boxes [B,29,4], top_feats [B,29,C] (gathered rows of pooled). */
int rgrg_top1_per_class_f32(const float* pred, int ldp, const float* proposals, const int32_t* offsets,
                            const float* pooled, uint8_t* class_detected, float* top_scores, float* top_boxes,
                            float* top_feats, int B, int C, int max_props, float img_w, float img_h, void* stream);

/* Replaces nn.BCEWithLogitsLoss(pos_weight) on `logits[class_detected]` of the two region classifiers in
 * forward() (src/binary_classifier/binary_classifier_region_selection.py:22,40-44 with pos_weight 2.2;
 * binary_classifier_region_abnormal.py:29,43-47 with 6.0): mean over the rows with mask != 0 of
 * (1-y) x - (1 + (w-1) y) log_sigmoid(x).  logits f32 [n], mask/target u8 [n], loss: one f32 (nan when no row). */
int rgrg_bce_with_logits_masked_f32(const float* logits, const uint8_t* mask, const uint8_t* target, float pos_weight,
                                    int n, float* loss, void* stream);
/* Replaces the albumentations pipeline of get_image_tensor (src/full_model/generate_reports_for_images.py:129-147;
 * SURVEY 8(f) rank 4) for a decoded 8-bit gray image already in device memory: LongestMaxSize(512, cv2.INTER_AREA)
 * [the caller passes new_h/new_w = py3round(dim * 512 / max(h, w))] -> centred zero PadIfNeeded(512, 512) ->
 * Normalize(mean, std; max_pixel_value 255) -> dst f32 [512*512] (= the [1,1,512,512] tensor).  Shrinking uses
 * OpenCV's INTER_AREA tables / integer fast paths; an image smaller than 512 px is ENLARGED the way OpenCV does it
 * for INTER_AREA with an enlarged axis (its 8-bit fixed-point bilinear path with the area coordinate rule).
 * OpenCV / albumentations are third-party and absent here: arithmetic restated from their published sources,
 * parity unpinned (oracle/preprocess.py). */
int rgrg_preprocess_u8_f32(const uint8_t* src, int h, int w, int src_stride, int new_h, int new_w, float mean, float std,
                           float* dst, void* stream);
/* BinaryClassifierRegionSelection threshold + mask + row-major compaction
 * (binary_classifier_region_selection.py:53-61): selected = (logit > thr) & detected;
 * sel_rows int32 [n] lists the selected flat (image*29+region) indices in order,
 * *n_selected (device int32) their number; feats_out [S,D] = feats[sel_rows]. */
int rgrg_select_regions_f32(const float* logits, const uint8_t* class_detected, float thr, uint8_t* selected,
                            int32_t* sel_rows, int32_t* n_selected, int n, void* stream);
int rgrg_gather_rows_f32(const float* src, const int32_t* rows, float* dst, int n_rows, int D, void* stream);

/* ---------------------------------------------------------------------------------
 * Greedy decoder (LanguageModel.generate num_beams=1 -> greedy_search,
 * src/language_model/language_model.py:401-447,609-652, with forward :258-366 and
 * GPT2PseudoAttention :124-180).  The decoder object keeps pointers to the (caller
 * owned, device resident) weights, owns its KV cache / activations workspace and a
 * captured hipGraph of one decode step per sequence count.
 * --------------------------------------------------------------------------------- */
typedef struct rgrg_decoder_layer_weights {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    const float *c_attn_w, *c_attn_b;     /* [3072,1024] (transposed Conv1D), [3072] */
    const float *attn_proj_w, *attn_proj_b; /* [1024,1024], [1024] */
    const float *c_fc_w, *c_fc_b;         /* [4096,1024], [4096] */
    const float *mlp_proj_w, *mlp_proj_b; /* [1024,4096], [1024] */
} rgrg_decoder_layer_weights;

typedef struct rgrg_decoder_weights {
    int n_layer, d_model, n_head, vocab; /* 24, 1024, 16, 50257 */
    const float* wte;                    /* [vocab,1024]; also the tied lm_head */
    const float *lnf_g, *lnf_b;
    const float *fst0_w, *fst0_b, *fst2_w, *fst2_b; /* feature_space_transformation_nn */
    const float *ukv_w, *ukv_b; /* [n_layer*2*1024, 1024] rows = (layer, uk|uv, out), [n_layer*2*1024] */
    const rgrg_decoder_layer_weights* layers; /* host array of n_layer entries */
} rgrg_decoder_weights;

typedef struct rgrg_decoder rgrg_decoder;

/* Allocates device memory (weights repacked into MFMA-fragment tiles for the
 * <=32-sequence path - LayerNorm gains folded in -, workspace for max_seqs sequences x max_len
 * positions).  SYNCHRONISES THE DEVICE on entry and before returning: the weights are packed on the
 * decoder's own stream and this entry has no stream argument, so it first waits for whatever is still
 * producing them on the caller's streams.  Not on the hot loop.   max_seqs < 65536 (16-bit row tickets of the arg-max bookkeeping). */
int rgrg_decoder_create(const rgrg_decoder_weights* w, int max_seqs, int max_len, rgrg_decoder** out);
/* The same with the K/V cache in CALLER-owned memory: kv_cache = device buffer of rgrg_decoder_kv_cache_bytes(n_layer,
 * max_seqs, max_len) bytes, zero-filled by the caller, which must outlive the decoder; rgrg_decoder_destroy does not free it.
 * The host mirror allocates it as a torch tensor, so that the `presents` of LanguageModel.forward(use_cache=True)
 * (language_model.py:396-399) are ordinary views whose lifetime torch manages - they stay valid when the decoder is replaced. */
int rgrg_decoder_create_with_cache(const rgrg_decoder_weights* w, int max_seqs, int max_len, void* kv_cache, size_t kv_cache_bytes,
                                   rgrg_decoder** out);
/* Bytes of the cache [n_layer][K | V][max_seqs][16 heads][max_len + 1 slots][64] in fp32. */
size_t rgrg_decoder_kv_cache_bytes(int n_layer, int max_seqs, int max_len);
void rgrg_decoder_destroy(rgrg_decoder* d);
/* feats [S,1024] (selected region features); out_ids int64 [S,max_length] is filled
 * with the leading BOS, the generated ids, and PAD (50256) after a row finished;
 * *out_len (host) = L' = 1 + number of forward passes the reference would have run
 * (stops when every row has emitted EOS or at max_length).  max_length <= 0 means
 * "until all rows finished" bounded by the decoder's max_len.  Synchronises `stream`
 * before returning.  use_graph=0 launches the kernels eagerly (debug/profiling). */
int rgrg_decoder_generate(rgrg_decoder* d, const float* feats, int S, int max_length, int64_t* out_ids,
                          int out_ld, int* out_len, int use_graph, void* stream);
/* LanguageModel.greedy_search with a prompt (language_model.py:609-652): rgrg_decoder_generate that continues input_ids int64 [S,T]
 * (any ids inside the vocabulary; an EOS inside the prompt finishes nothing) instead of a BOS column.  Slot 0 of the cache is the
 * image as in rgrg_decoder_generate; ONE teacher-forced pass over the S x T prompt rows in the current precision mode stores the
 * keys / values of every prompt token in slots 1 .. T of the decode cache (fp32, or the 16-bit type where the decode steps of S rows
 * keep a 16-bit cache) and yields the first generated token from the S last-position rows (no [S,T,V] logits exist); the decode
 * loop runs from step T on.  attention_mask f32 [S,T] of zeros and ones, or NULL = all ones: zeros are LEFT padding; padded slots
 * stay out of every later step (the reference's additive -1e4, :316-334), the image key and generated tokens never do, and row s
 * embeds its tokens at cumsum(mask) - 1 continued per row (prepare_inputs_for_generation, :498-520), padded slots at 1.
 * max_length is the reference's: cur_len starts at T, one token is always produced, the loop ends at cur_len >= max_length or when
 * every row has emitted EOS among its GENERATED tokens; <= 0 = bounded by the decoder's max_len.  out_ids [S,out_ld] receives the
 * prompt, the generated ids and PAD behind a row's EOS; *out_len = L' >= T + 1.  A mask of ones replays the captured step of
 * rgrg_decoder_generate, a padded prompt its own.  Afterwards rgrg_decoder_copy_last_logits works as after rgrg_decoder_generate.
 *   RGRG_EINVAL (with a message): T + 1 > max_len of the decoder; max_length > max_len; a mask row of zeros only; a zero behind a
 *   one (not left padding); mask values other than 0 and 1; the e4m3 K/V cache in use for S rows (rgrg_decoder_set_kv_format).
 * There is no flag for "no mask given": the reference's greedy_search cannot run without one (its forward dereferences the mask,
 * :281), so the host mirror refuses that call and NULL here simply means ones. */
int rgrg_decoder_generate_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask, int S,
                                   int T, int max_length, int64_t* out_ids, int out_ld, int* out_len, int use_graph, void* stream);
/* Rolling-batch greedy decoding: the S sequences of feats [S,1024] flow through R decoder rows (1 <= R <= max_seqs of the decoder; S
 * is not bounded by it).  Every step runs the R rows; a row whose sequence has ended - EOS, or max_length tokens with the BOS - takes
 * the next pending sequence in the same step (pending sequences go to the free rows in ascending row order), starting again from BOS
 * at position 0 with that sequence's image key / value in slot 0 of the row; rows without a sequence idle.  Every row keeps its own
 * step: its attention reads the keys of ITS sequence only.  Sequence s produces the tokens rgrg_decoder_generate produces for it.
 * ids_out int64 [S][max_length] on the device: BOS, the tokens, PAD behind the last one; lens_out int32 [S] on the device: tokens
 * of every sequence, the BOS and the EOS included; *steps_out (host, optional): steps in which at least one row held a sequence.
 * The step plan, the precision and the cache format are those of a decode step of R rows.  Synchronises `stream` before returning;
 * use_graph = 0 launches the kernels eagerly.
 *   RGRG_EINVAL (with a message): R outside 1 .. max_seqs; max_length outside 2 .. max_len; the e4m3 K/V cache in use for R rows.
 *   RGRG_EHIP: sequences unfinished after (ceil(S / R) + 1) * (max_length - 1) steps - the bound of any schedule; the loop stops there. */
int rgrg_decoder_generate_rolling(rgrg_decoder* d, const float* feats, int S, int R, int max_length, int64_t* ids_out, int* lens_out,
                                  int* steps_out, int use_graph, void* stream);
/* Test hook: ONE retire-and-refill step of rgrg_decoder_generate_rolling (the kernels behind the arg-max of its step) on the caller's
 * state, all on the device.  int32 [R]: row_seq (the sequence a row holds, -1 = idle), row_len (its tokens so far), row_tok / row_pos
 * / row_step (token, embedding position and step of the row's next step), arg (the arg-max of the step just run); shared int32 [4]
 * = {next pending sequence, unfinished sequences, refills of this step, steps that had an active row}; ids int64 [S][ld_ids], lens
 * int32 [S].  ukv f32 [S][ld_ukv >= n_layer * 2 * H * 64] and the cache kv [n_layer][K | V][R][H][T_slots][64] (kv16 = 0 fp32, 1 the
 * 16-bit type of fp16; layer_stride / kv_stride in elements) are given together or both NULL (no refill launch): slot 0 of a
 * refilled row receives the sequence's image key / value in the cache's rounding.  Synchronises `stream`. */
int rgrg_debug_roll_step(int* row_seq, int* row_len, int* row_tok, int* row_pos, int* row_step, int* shared, const int* arg,
                         int64_t* ids, int ld_ids, int* lens, int S, int R, int max_length, const float* ukv, int ld_ukv, void* kv,
                         size_t layer_stride, size_t kv_stride, int H, int T_slots, int n_layer, int kv16, int fp16, void* stream);
/* Rolling-batch sampling: rgrg_decoder_generate_rolling with every arg-max replaced by the draw of "Sampling" below.  feats [S,1024];
 * every feature row s has n hypotheses, sequences q = s * n + j (j < n), S * n sequences in all, which flow through the R rows in
 * the order of q.  The n sequences of a feature row share its image key / value: the prefill runs over the S feature rows only.
 * Sequence q draws the token of column c under the Philox counter (q, c - 1) - the counter of rgrg_decoder_sample for its row q at
 * step c - 1; neither the decoder row that holds q nor the step of the call enters it, so the result does not depend on R beyond
 * what the step plan of R rows does to the logits.  ids_out int64 / logprobs_out f32 (or NULL) [S*n][max_length] and lens_out int32
 * [S*n] on the device: BOS, the tokens, PAD behind the last one; the log-prob of every drawn token, 0 in the BOS column and under
 * PAD.  top_k = 1 gives the ids of rgrg_decoder_generate_rolling.  *steps_out, use_graph, `stream` and the refusals are those of
 * rgrg_decoder_generate_rolling (the bound with S * n sequences), the parameter refusals those of rgrg_decoder_sample.  One captured
 * step per (R, plan) serves every seed and parameter set. */
int rgrg_decoder_sample_rolling(rgrg_decoder* d, const float* feats, int S, int n, int R, int max_length, float temperature, int top_k,
                                float top_p, uint64_t seed, int64_t* ids_out, float* logprobs_out, int* lens_out, int* steps_out,
                                int use_graph, void* stream);
/* Test hook: the rolling sampler of rgrg_decoder_sample_rolling (the launch behind the logits of its step) on the caller's state, all
 * on the device.  logits f32 [R][ld] (V <= 53248 of every row are the logits; 16-byte loads when ld % 4 == 0 and logits is 16-byte
 * aligned); row_seq / row_len int32 [R]: the sequence a row holds (-1 = idle) and its tokens so far (>= 1).  An active row r draws
 * under the counter (row_seq[r], row_len[r] - 1) and writes the token to arg[r] and - lp not NULL - the log-prob to
 * lp[row_seq[r] * ld_lp + row_len[r]]; nothing else is written, nothing at all for an idle row.  Synchronises `stream`. */
int rgrg_debug_roll_sample(const float* logits, int64_t ld, int V, int R, const int* row_seq, const int* row_len, float temperature,
                           int top_k, float top_p, uint64_t seed, int* arg, float* lp, int ld_lp, void* stream);
/* ---- Rolling session: rolling-batch greedy decoding / sampling over an OPEN list.  One session per decoder; it owns the decoder's
 * cache rows until it is closed.  Sequences are numbered q = 0, 1, 2, ... over the life of the session, n per submitted feature
 * row (q / n is the feature row); the sampler's Philox counter stays (q, c - 1).  The session holds `capacity` feature rows, C =
 * capacity * n sequences: output rows live in rings the decoder owns (ids / log-probs [C][max_length], lengths [C], row q % C; image
 * key / value rows [capacity], row (q / n) % capacity).  The host keeps a watermark, the lowest sequence number not yet released.
 * Every other decode entry on the decoder works as without a session and makes the session stale: its calls then fail with
 * RGRG_EINVAL and a message containing "stale"; rgrg_decoder_roll_close still works.
 *
 * open: R rows, max_length, use_graph and the refusals of rgrg_decoder_generate_rolling (at open, the e4m3 cache included); sample != 0:
 *   steps draw under (temperature, top_k, top_p, seed) as rgrg_decoder_sample_rolling, refusals of rgrg_decoder_sample.
 *   RGRG_EINVAL: a session is open already; capacity < 1 or capacity * n >= 0x7fffffff / 1024.
 * submit: m feature rows feats [m][1024] (device, `stream`'s) -> sequences *first_out .. *first_out + m * n - 1, in stream order behind the
 *   steps already queued: the prefill GEMMs into the ukv ring, the new output rows (BOS, PAD, log-probs 0, length 0), S and the
 *   unfinished count, one hand-out-only pass (idle rows take pending sequences in ascending row order; a row that holds a sequence is
 *   not touched) and its refill.  RGRG_EINVAL before anything is enqueued, the session intact: the last new sequence at or beyond
 *   watermark + C (the message names the capacity and the room left); sequence numbers at or beyond 0x7fffffff / 1024 (open a new
 *   session).  Does not synchronise.
 * advance: up to max_steps steps (< 0: until nothing is unfinished, bounded by (ceil(unfinished / R) + 1) * (max_length - 1), RGRG_EHIP
 *   beyond), polled every 16 steps and 16 steps late as rgrg_decoder_generate_rolling; nothing is launched when the last poll said 0
 *   and no submit has come since.  Synchronises.  *launched_out: steps launched; *unfinished_out: sequences pending or in a row;
 *   *steps_out: the device's count of steps that had an active row, over the session.
 * collect: sequences first .. first + count - 1 (watermark <= first, first + count <= submitted) -> ids_out int64 / logprobs_out f32
 *   [count][max_length] on the device (either may be NULL) and lens_out int32 [count] on the HOST: the length of a finished sequence, 0
 *   for one that has not finished as of the last advance.  Synchronises.
 * release: the new watermark; RGRG_EINVAL when it moves backwards, beyond what was submitted, or past a sequence that has not
 *   finished as of the last advance.
 * close: synchronises, frees the rings.  No session open: RGRG_OK. */
int rgrg_decoder_roll_open(rgrg_decoder* d, int R, int capacity, int n, int max_length, int sample, float temperature, int top_k,
                           float top_p, uint64_t seed, int use_graph, void* stream);
int rgrg_decoder_roll_submit(rgrg_decoder* d, const float* feats, int m, long long* first_out, void* stream);
int rgrg_decoder_roll_advance(rgrg_decoder* d, int max_steps, int* launched_out, int* unfinished_out, int* steps_out);
int rgrg_decoder_roll_collect(rgrg_decoder* d, long long first, int count, int64_t* ids_out, float* logprobs_out, int* lens_out,
                              void* stream);
int rgrg_decoder_roll_release(rgrg_decoder* d, long long watermark);
int rgrg_decoder_roll_close(rgrg_decoder* d);
/* ---- Requests of a rolling session: every submit may carry its own decoding parameters, and a submitted sequence can be cancelled.
 * Request ring: the decoder keeps one 40-byte entry per ring row (entry q % C for sequence q), written at submit and read by the
 * retire pass and the sampler of every step for the sequence a row holds.  Layout (little endian, what the two _req hooks take):
 *   0 uint64 seed | 8 float 1 / temperature | 12 int32 top_k | 16 float top_p | 20 int32 max_length | 24 int32 q0 |
 *   28 uint16 stop[4] (65535 = unused) | 36 uint32 flags (bit 0: cancelled)
 * rgrg_decoder_roll_submit writes the session's own values with q0 = 0 - its results are those of a session without requests.
 *
 * submit_req: rgrg_decoder_roll_submit with a request for all m * n new sequences.  max_length 0: the session's, else 2 .. the
 *   session's: the sequence retires when its max_length-th token is written (the ring rows keep the session's width).  temperature 0,
 *   top_k < 0, top_p 0, has_seed 0: the session's value; anything else is accepted in a sampling session only and validated as
 *   rgrg_decoder_sample does.  top_k = 1 is a greedy request inside a sampling session.  Counter rule: without a seed sequence q draws
 *   column c under the session's seed and the Philox counter (q, c - 1); with has_seed under `seed` and (q - q0, c - 1), q0 being the
 *   first sequence of the submit - what rgrg_decoder_sample_rolling gives for these feature rows alone under that seed.  stop_ids
 *   (host, n_stop <= 4 token ids < 65535): tokens that end a sequence as EOS does - appended, the last token.  RGRG_EINVAL before
 *   anything is enqueued, the session intact: the refusals of submit, a value out of range, a sampling value in a greedy session.
 * cancel: sets the cancel flag of sequences first .. first + count - 1 (watermark <= first, first + count <= submitted; RGRG_EINVAL
 *   otherwise) on the decoder's stream, without synchronising.  Cancel rule: the retire pass of the next step launched after the call
 *   CUTS a flagged sequence that holds a row: the token of that step is not appended, the row is free in the same pass and takes the
 *   next pending sequence.  A flagged sequence still pending takes a row as usual and is cut in that row's first retire pass: BOS
 *   alone, one row-step.  A sequence that has ended is not touched.
 * Length word: lens_out of rgrg_decoder_roll_collect is > 0 for a sequence that has ended (its tokens), < 0 for one that was cut
 *   (minus its tokens, BOS included; no EOS is added) and 0 for one that has not finished.  release accepts both non-zero kinds. */
int rgrg_decoder_roll_submit_req(rgrg_decoder* d, const float* feats, int m, int max_length, float temperature, int top_k, float top_p,
                                 int has_seed, uint64_t seed, const int* stop_ids, int n_stop, long long* first_out, void* stream);
int rgrg_decoder_roll_cancel(rgrg_decoder* d, long long first, int count);
/* Test hook: what a session enqueues around one step, on the caller's state with a ring, all on the device.  Arrays as
 * rgrg_debug_roll_step, but ids int64 / lp f32 (or NULL) [C][ld_ids], lens [C] and ukv [C / n][ld_ukv] are rings: sequence q uses row
 * q % C and ukv row (q / n) % (C / n).  In this order: submit > 0: the new sequences S_before .. S_before + submit - 1 get their
 * output rows (BOS, PAD, log-probs 0, length 0 - no other row is written), S and shared[1] grow by submit; handout != 0: the
 * hand-out-only pass; retire != 0: a whole retire pass on arg.  Each pass is followed by its refill launch when ukv / kv are given.
 * S_before is the sequence count before the submit.  Synchronises `stream`. */
int rgrg_debug_roll_session_step(int* row_seq, int* row_len, int* row_tok, int* row_pos, int* row_step, int* shared, const int* arg,
                                 int64_t* ids, float* lp, int ld_ids, int* lens, int C, int n, int S_before, int submit, int handout,
                                 int retire, int R, int max_length, const float* ukv, int ld_ukv, void* kv, size_t layer_stride,
                                 size_t kv_stride, int H, int T_slots, int n_layer, int kv16, int fp16, void* stream);
/* Test hook: rgrg_debug_roll_session_step with the caller's request ring req [C] on the device ("Request ring" above; NULL: exactly
 * that hook).  The retire pass takes the limit, the stop ids and the cancel flag of a row's sequence from entry row_seq[r] % C; a cut
 * writes lens[row_seq[r] % C] = -row_len[r].  The submit-init does not write the ring.  RGRG_EINVAL: an entry whose max_length is not
 * 2 .. max_length or whose sampling values rgrg_decoder_sample would refuse (the ring is read back and checked first). */
int rgrg_debug_roll_session_step_req(int* row_seq, int* row_len, int* row_tok, int* row_pos, int* row_step, int* shared, const int* arg,
                                     int64_t* ids, float* lp, int ld_ids, int* lens, int C, int n, int S_before, int submit, int handout,
                                     int retire, int R, int max_length, const float* ukv, int ld_ukv, void* kv, size_t layer_stride,
                                     size_t kv_stride, int H, int T_slots, int n_layer, int kv16, int fp16, const void* req, void* stream);
/* Test hook: rgrg_debug_roll_sample with the caller's request ring req [C] on the device (NULL: exactly that hook, C unused).  An
 * active row draws with the values of entry row_seq[r] % C under the counter (row_seq[r] - q0, row_len[r] - 1); lp is [C][ld_lp], the
 * log-prob goes to lp[(row_seq[r] % C) * ld_lp + row_len[r]].  (temperature, top_k, top_p, seed) fill the step's parameter block, which
 * is not read then.  RGRG_EINVAL: C < 1, an entry rgrg_decoder_sample would refuse, q0 < 0. */
int rgrg_debug_roll_sample_req(const float* logits, int64_t ld, int V, int R, const int* row_seq, const int* row_len, float temperature,
                               int top_k, float top_p, uint64_t seed, const void* req, int C, int* arg, float* lp, int ld_lp,
                               void* stream);
/* ---- Prompts in a rolling session: a submit's sentences continue a prompt of P tokens (greedy_search's semantics with a mask of
 * ones: no padding, ever; one submit has one P).
 * open_prompt: rgrg_decoder_roll_open with max_prompt_length = MP.  0 is exactly rgrg_decoder_roll_open: no memory, the same step.
 *   1 .. max_length - 1 (RGRG_EINVAL otherwise) allocates, at open, a token ring int32 [capacity][MP], a length ring [capacity], a prompt
 *   K/V ring in the cache's element format for R rows with planes [layer][2][capacity][H][MP][64], and the work space of a
 *   teacher-forced pass over 512 prompt rows (at least MP - 1); RGRG_EHIP with the ring's size when that does not fit.  The step of
 *   such a session has one more launch, the prompt refill, and a graph of its own.
 * submit_prompt: rgrg_decoder_roll_submit_req (same request arguments) with prompt_ids int64 [m][P] on the HOST, row i for feature row
 *   i; the n hypotheses of a feature row share it.  Ids are any tokens 0 .. vocabulary - 1: an EOS or stop token inside the prompt
 *   ends nothing.  1 <= P <= MP and P + 1 <= the sequence's max_length, which counts the prompt.  Enqueued in front of the
 *   hand-out pass: the prompt's tokens and length into ring row (q / n) % capacity, rows 0 .. P - 2 of the prompt as teacher-forced
 *   passes (at most 512 token rows each) that attend to the submit's ukv ring rows and leave their keys / values in slots 1 .. P - 1 of
 *   the K/V ring row.  The output row starts with the P prompt tokens (log-probs 0).  A row that takes the sequence gets len = P,
 *   tok = prompt[P - 1], pos = step = P - 1, and the prompt refill copies ring slots 1 .. P - 1 to its cache row next to slot 0; the
 *   last prompt token runs through the row's ordinary decode step.  A prompted sequence cut before its first step has the length
 *   word -P.  rgrg_decoder_roll_submit / _submit_req in such a session are P = 1, the BOS column.  Does not synchronise or allocate.
 *   RGRG_EINVAL before anything is enqueued, the session intact: the refusals of submit_req; a session opened without
 *   max_prompt_length; a rolling beam session; P out of range; an id outside the vocabulary. */
int rgrg_decoder_roll_open_prompt(rgrg_decoder* d, int R, int capacity, int n, int max_length, int max_prompt_length, int sample,
                                  float temperature, int top_k, float top_p, uint64_t seed, int use_graph, void* stream);
int rgrg_decoder_roll_submit_prompt(rgrg_decoder* d, const float* feats, int m, const int64_t* prompt_ids, int P, int max_length,
                                    float temperature, int top_k, float top_p, int has_seed, uint64_t seed, const int* stop_ids, int n_stop,
                                    long long* first_out, void* stream);
/* Test hook: rgrg_debug_roll_session_step_req with prompt rings on the device: ptok int32 [C / n][MP], plen int32 [C / n] (1 .. MP; MP <
 * max_length, MP + 1 <= T_slots) and pkv [n_layer][2][C / n][H][MP][64] in the cache's element format (NULL together with kv).  The
 * submit-init writes the prompt of feature row (q / n) % (C / n) into the id row of sequence q; a seating pass gives the row len = P,
 * tok = prompt[P - 1], pos = step = P - 1 and is followed by the refill and the prompt refill (ring slots 1 .. P - 1 -> the row's cache
 * slots 1 .. P - 1, every layer, plane and head; nothing else is written).  RGRG_EINVAL: a ring row the product would refuse (the rings
 * are read back and checked first). */
int rgrg_debug_roll_prompt_step(int* row_seq, int* row_len, int* row_tok, int* row_pos, int* row_step, int* shared, const int* arg,
                                int64_t* ids, float* lp, int ld_ids, int* lens, int C, int n, int S_before, int submit, int handout,
                                int retire, int R, int max_length, const float* ukv, int ld_ukv, void* kv, size_t layer_stride,
                                size_t kv_stride, int H, int T_slots, int n_layer, int kv16, int fp16, const void* req, const int* ptok,
                                const int* plen, const void* pkv, int MP, void* stream);
/* Rolling-batch beam search: rgrg_decoder_beam_search over the S regions of feats [S,1024] with the regions flowing through
 * G = min(R / num_beams, S) SLOTS of num_beams consecutive decoder rows (num_beams <= R <= max_seqs of the decoder; S is not bounded
 * by it; rows behind G * num_beams are not used, and the step plan, precision and cache format are those of a step of G * num_beams
 * rows).  Every slot has its own cur_len, heap and `done` flag.  A region leaves its slot when its scorer is done or when its cur_len
 * reaches max_length; it is finalized then and the slot takes the next pending region in the same step - fresh rows at step 0 with
 * beam scores 0, -1e9, ..., token BOS and the region's image key / value in slot 0 of the slot's first row; free slots take pending
 * regions in ascending slot order, slots without a region idle.  The scorer is the one of rgrg_decoder_beam_search, on the host, with
 * one synchronisation per step.  out_ids int64 [S * num_return_sequences][out_ld >= max_length] on the device and *out_len = L are
 * what rgrg_decoder_beam_search returns for the same arguments: the same ids in the same order, the width L computed over all regions
 * at the end.  *steps_out (host, optional): steps run, each with at least one occupied slot.  The prefill runs once over the S feature
 * rows.  Synchronises `stream` before returning; use_graph = 0 launches the kernels eagerly.  More than 16 beams take the wide ranking
 * kernels, as in lock step.
 *   RGRG_EINVAL (with a message): R < num_beams or R > max_seqs; max_length outside 2 .. max_len; the e4m3 K/V cache in use for the rows.
 *   RGRG_EHIP: regions unfinished after (ceil(S / G) + 1) * (max_length - 1) steps - the bound of any schedule; the loop stops there. */
int rgrg_decoder_beam_search_rolling(rgrg_decoder* d, const float* feats, int S, int num_beams, int R, int max_length,
                                     int early_stopping, float length_penalty, int num_return_sequences, int64_t* out_ids, int out_ld,
                                     int* out_len, int* steps_out, int use_graph, void* stream);
/* ---- Rolling beam session: rgrg_decoder_beam_search_rolling over an OPEN list.  One session per decoder, and never next to a
 * rgrg_decoder_roll_* session: opening either kind while the other is open fails with RGRG_EINVAL and a message.  G = R / num_beams
 * slots, fixed for the life of the session; every step runs on G * num_beams rows (step plan, precision and cache format are those
 * of that many rows in the modes in force at open), idle slots included.  Regions are numbered q = 0, 1, 2, ... over the life of the
 * session, one per submitted feature row.  The session holds `capacity` regions: image key / value rows live in a ring [capacity] the
 * decoder owns, row q % capacity; heaps and finished hypotheses live on the host for regions watermark .. submitted - 1.  Every other
 * decode entry on the decoder works as without a session and makes the session stale: its calls then fail with RGRG_EINVAL and a
 * message containing "stale"; rgrg_decoder_beam_roll_close still works.
 *
 * open: the arguments of rgrg_decoder_beam_search_rolling.  Refused, in this order and before any device work: num_beams and
 *   num_return_sequences as there; R < num_beams; the refusals of rgrg_decoder_generate_rolling for G * num_beams rows (the e4m3 cache
 *   included); capacity < 1; a session of either kind open on this decoder.  Every slot starts idle.
 * submit: m feature rows feats [m][1024] (device, `stream`'s) -> regions *first_out .. *first_out + m - 1, pending: the prefill GEMMs
 *   into the ring rows, in two passes where the ring wraps, in stream order behind the steps already run.  RGRG_EINVAL before anything
 *   is enqueued, the session intact: the last new region at or beyond watermark + capacity (the message names the capacity and the
 *   room left).  Does not synchronise: feats must stay valid until the next advance has synchronised.
 * advance: up to max_steps steps (< 0: until nothing is unfinished, bounded by (ceil(unfinished / G) + 1) * (max_length - 1), RGRG_EHIP
 *   beyond).  In front of every step free slots take the pending regions in ascending slot order - a slot is seated only in front of
 *   a step that is launched -, then the step of rgrg_decoder_beam_search_rolling with its one synchronisation; a region that is done,
 *   or has reached max_length, is finalized and frees its slot.  Nothing is launched when no slot is occupied and nothing is pending.
 *   A region left mid-flight is continued by the next advance.  *launched_out: steps launched; *unfinished_out: regions pending or
 *   seated; *steps_out: steps run over the session, each with an occupied slot.
 * collect: regions first .. first + count - 1 (watermark <= first, first + count <= submitted).  finished_out int32 [count] on the HOST
 *   (or NULL): 1 for a region finalized as of the last advance.  out_ids == NULL: only this query.  Otherwise every region of the range
 *   must be finished (RGRG_EINVAL), and out_ids int64 [count * num_return_sequences][out_ld >= max_length] on the device and *out_len
 *   are what rgrg_decoder_beam_search_rolling returns for a call over exactly these regions (the width over the range).  Synchronises.
 * release: the new watermark; the heaps below it are dropped.  RGRG_EINVAL when it moves backwards, beyond what was submitted, or
 *   past a region that has not finished as of the last advance.
 * close: synchronises, drops the session.  No session open: RGRG_OK. */
int rgrg_decoder_beam_roll_open(rgrg_decoder* d, int R, int num_beams, int capacity, int max_length, int early_stopping,
                                float length_penalty, int num_return_sequences, int use_graph, void* stream);
int rgrg_decoder_beam_roll_submit(rgrg_decoder* d, const float* feats, int m, long long* first_out, void* stream);
int rgrg_decoder_beam_roll_advance(rgrg_decoder* d, int max_steps, int* launched_out, int* unfinished_out, int* steps_out);
int rgrg_decoder_beam_roll_collect(rgrg_decoder* d, long long first, int count, int64_t* out_ids, int out_ld, int* out_len,
                                   int* finished_out, void* stream);
int rgrg_decoder_beam_roll_release(rgrg_decoder* d, long long watermark);
int rgrg_decoder_beam_roll_close(rgrg_decoder* d);
/* Test hook: the turn kernel of rgrg_decoder_beam_search_rolling (beam_roll_turn_kernel: ancestor table and per-row step of the next
 * step, one launch) on the caller's state, all int32 on the device.  src_old / src_new [R][T] are two buffers; parent [R]: the row of
 * the row's slot (rows r / nb * nb .. + nb - 1) whose beam row r continues, -1 = fresh (the slot takes a new region), -2 = idle;
 * step [R], updated in place, one value per slot among its continuing rows.  Continuing row r at step t: src_new[r][0..t] =
 * src_old[parent][0..t], src_new[r][t + 1] = parent, step[r] = t + 1.  Fresh: src_new[r][0] = r / nb * nb, step[r] = 0.  Idle:
 * step[r] = 0.  No other cell of src_new is written.  parent and step are read back and checked first (RGRG_EINVAL: a parent outside
 * the slot, rows of a slot at different steps, a step outside 0 .. T - 2).  Synchronises `stream`. */
int rgrg_debug_beam_roll_turn(const int* src_old, int* src_new, const int* parent, int* step, int T, int nb, int R, void* stream);
/* ---- Sampling.  The sampler is a pure function of one fp32 logits row x[0..V), temperature > 0, top_k >= 0 (0 = off),
 * 0 < top_p <= 1 (1 = off), a 64-bit seed, a row counter r and a step t:
 *   temperature  z_i = x_i * inv_T, inv_T = 1.0f / temperature computed once on the host in fp32.
 *   top-k        HF 4.19.2 TopKLogitsWarper: keep every token whose logit is >= the k-th largest logit (raw x, exact compare);
 *                ties with the k-th value are all kept; k >= V is a no-op.
 *   top-p        after top-k, on the distribution re-normalised over the top-k set: keep token i iff the total probability of
 *                the kept tokens with a STRICTLY GREATER logit is <= top_p (TopPLogitsWarper with min_tokens_to_keep = 1,
 *                stated through a threshold).  Tokens with equal logits are therefore kept or dropped TOGETHER; HF breaks
 *                such ties by the order its sort happens to return.
 *   draw         w = first output word of Philox4x32-10 with key = seed (low word, high word) and counter = (r, t, 0, 0);
 *                u = (w >> 8) * 2^-24; the token is the first kept index j in VOCABULARY order whose running sum of
 *                exp(z_i - max z) over the kept i <= j exceeds u times the kept total.  top_k = 1: the first kept index -
 *                the first-occurrence arg-max, exactly what greedy returns.
 *   log-prob     log q(token) under the distribution the token was drawn from (after temperature and filters), fp32.
 * Deterministic: the same inputs give the same bits (masses are accumulated as 64-bit fixed-point integers, sample.hip).
 *
 * Rolling counter rule (rgrg_decoder_sample_rolling): the row counter r is the SEQUENCE q, not the decoder row that happens to
 * decode it, and t = c - 1 for the token of column c of that sequence, not the step of the call: which row decodes a sequence,
 * and when, does not enter the draw.
 *
 * rgrg_decoder_sample: rgrg_decoder_generate with the arg-max replaced by that draw, row counter r = the row, t = the step
 * (0 for the first generated token).  Same prefill, same out_ids / *out_len semantics (PAD after a row's EOS); out_logprobs
 * f32 [S,out_ld] or NULL: log-prob of every generated token, 0 in the BOS column and for the PAD of finished rows.  Runs on
 * every step plan and precision mode; the step is captured once per S and serves every seed and parameter set.  Afterwards
 * rgrg_decoder_copy_last_logits returns the logits the last draw was made from. */
int rgrg_decoder_sample(rgrg_decoder* d, const float* feats, int S, int max_length, float temperature, int top_k, float top_p,
                        uint64_t seed, int64_t* out_ids, int out_ld, float* out_logprobs, int* out_len, int use_graph,
                        void* stream);
/* LanguageModel.sample_from_prompt: rgrg_decoder_generate_prompted with every arg-max replaced by the draw of rgrg_decoder_sample -
 * the same prompt pass, mask rules, max_length and refusals; the token behind the prompt is drawn from the logits of the S
 * last-position rows.  The Philox counter of row r for the token in column c is (r, c - 1) - the device step word - so a [S,1] BOS
 * prompt with a mask of ones uses the counters of rgrg_decoder_sample.  out_logprobs f32 [S,out_ld] or NULL: 0 in the prompt
 * columns and for the PAD of finished rows.  A mask of ones replays the captured sampling step, a padded prompt its own. */
int rgrg_decoder_sample_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask, int S, int T,
                                 int max_length, float temperature, int top_k, float top_p, uint64_t seed, int64_t* out_ids, int out_ld,
                                 float* out_logprobs, int* out_len, int use_graph, void* stream);
/* The same sampler on caller-provided logits [S][ld] (V <= 53248; 16-byte loads when ld % 4 == 0 and logits is 16-byte
 * aligned): row s is drawn with the counter (row0 + s, step).  out_tok int32 [S], out_logprob f32 [S] or NULL. */
int rgrg_sample_logits_f32(const float* logits, int64_t ld, int S, int V, float temperature, int top_k, float top_p,
                           uint64_t seed, int step, int row0, int* out_tok, float* out_logprob, void* stream);
/* Beam search (LanguageModel.generate num_beams > 1 -> beam_search, language_model.py:450-475,
 * :529-607, with transformers 4.19.2 BeamSearchScorer semantics; 1 <= num_return_sequences <= num_beams).
 * The decoder must have been created with max_seqs >= S*num_beams.  Any num_beams, as in the reference (up to 16 the row / item
 * rankings keep per-thread candidate lists in registers; wider beams rank in 2*num_beams rounds over the row - same winners).
 * Device side: one decode step over the S*num_beams beam rows (KV cache never re-ordered:
 * per-slot ancestor table), per-row log-sum-exp + top-2*num_beams, per-item merge.  Host
 * side (one small D2H/H2D per step, like the reference's scorer): hypothesis bookkeeping.
 * out_ids int64 [S * num_return_sequences, out_ld] receives the best hypotheses of every item (best first),
 * *out_len their padded length. */
int rgrg_decoder_beam_search(rgrg_decoder* d, const float* feats, int S, int num_beams, int max_length,
                             int early_stopping, float length_penalty, int num_return_sequences, int64_t* out_ids,
                             int out_ld, int* out_len, void* stream);
/* LanguageModel.beam_search with a prompt (language_model.py:529-607): rgrg_decoder_beam_search that continues input_ids int64 [S,T],
 * ONE prompt per item (the num_beams rows the reference expands an item into are equal).  attention_mask f32 [S,T] or NULL, with
 * the rules and refusals of rgrg_decoder_generate_prompted.  The prompt runs as ONE teacher-forced pass over S x T token rows - not
 * S x num_beams x T -: its keys / values live once, in cache row s * num_beams, and every beam row reaches them through the
 * per-slot ancestor table.  The first ranking is the reference's first iteration on num_beams identical rows: the logits of the
 * item's last prompt position with beam scores [0, -1e9, ...].  A mask of ones then replays the captured beam steps of
 * rgrg_decoder_beam_search, a padded prompt steps of its own (per-item positions, padded slots left out of every later step).
 * Hypothesis lengths and the is_done length count the prompt, padding included (hyp.shape[-1] and cur_len of the reference).
 *   RGRG_EINVAL (with a message): max_length < T + 1 (finalize cannot hold a longer hypothesis) or > max_len of the decoder; the
 *   mask refusals of rgrg_decoder_generate_prompted; the e4m3 K/V cache in use for S * num_beams rows. */
int rgrg_decoder_beam_search_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask, int S,
                                      int T, int num_beams, int max_length, int early_stopping, float length_penalty,
                                      int num_return_sequences, int64_t* out_ids, int out_ld, int* out_len, void* stream);
/* Diverse beam search (transformers 4.19.2 group_beam_search with its HammingDiversityLogitsProcessor; the reference's generate()
 * refuses num_beam_groups > 1, LanguageModel.group_beam_search is this build's own entry).  G = num_beam_groups groups of
 * gs = num_beams / G beam rows per item: group g of item s owns rows s * num_beams + g * gs .. + gs - 1 and starts with beam score
 * 0 in its first row, -1e9 in the others.  Every step runs ONE decode step over the S * num_beams rows, beam_row_topk_kernel with
 * K = 2 * num_beams candidates per row, and ONE launch of beam_group_merge_kernel (one workgroup per item) that ranks the groups
 * in order: group g's candidates are penalised by the tokens that groups 0 .. g-1 of the item took IN THIS STEP - the first gs
 * non-EOS candidates of each in rank order - a token taken by two beams counting twice.
 *   Arithmetic contract (fp32, every operation rounded once, the multiply never contracted into the subtract):
 *     score = ((v - row_max) - row_logsum) - round(diversity_penalty * (float)freq) + beam_score
 *   ranked per group over its gs * 2 num_beams row candidates: score descending, ties to the lower flat index
 *   beam_in_group * V + token; the top 2 gs of group g go to candidate slots g * 2 gs .. of the item's 2 num_beams slots.
 * The penalty is read from a device word written before the loop: the captured step (keyed on num_beams AND num_beam_groups, never
 * shared with a plain beam step) serves every penalty.  Host side: BeamSearchScorer.process per item and group with group_size gs.
 * HF's quirks are kept: the hypothesis heap (capacity num_beams) and the `done` flag belong to the ITEM and are shared by its
 * groups, is_done takes the group's best candidate score, so `done` can flip between two groups of a step - the later groups of
 * that item then take PAD with score 0 and finalize skips the item; cur_len is the same for all groups of a step; finalize returns
 * the num_return_sequences best hypotheses of the item's heap overall, not one per group.  num_beam_groups = 1 applies no penalty
 * and IS rgrg_decoder_beam_search (same ids).
 *   RGRG_EINVAL (with a message): num_beams % num_beam_groups != 0; num_beam_groups > num_beams; num_beam_groups > 1 with a
 *   diversity_penalty that is not a finite float > 0; num_beams > 16 (the K-round ranking kernels of wider beams have no group
 *   form); num_return_sequences outside 1 .. num_beams. */
int rgrg_decoder_group_beam_search(rgrg_decoder* d, const float* feats, int S, int num_beams, int num_beam_groups,
                                   float diversity_penalty, int max_length, int early_stopping, float length_penalty,
                                   int num_return_sequences, int64_t* out_ids, int out_ld, int* out_len, void* stream);
/* ... from a prompt: the prompt arguments, mask rules and refusals of rgrg_decoder_beam_search_prompted (max_length < T + 1, the
 * mask refusals, the e4m3 K/V cache in use for S * num_beams rows) on top of the refusals above.  The first ranking is the group
 * ranking of the item's last prompt position on num_beams identical rows. */
int rgrg_decoder_group_beam_search_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask,
                                            int S, int T, int num_beams, int num_beam_groups, float diversity_penalty, int max_length,
                                            int early_stopping, float length_penalty, int num_return_sequences, int64_t* out_ids,
                                            int out_ld, int* out_len, void* stream);
/* ---- Beam-search sampling (transformers' beam_sample; the reference's generate() refuses do_sample with num_beams > 1,
 * LanguageModel.beam_sample is this build's own entry).  rgrg_decoder_beam_search whose ranking DRAWS the item's 2 num_beams
 * candidates without replacement from the joint distribution over its num_beams x V continuations.  The order of operations is that
 * of transformers' later releases: the row's log-probabilities are warped, THEN the beam score is added (4.19.2 warped the sum,
 * which multiplies the running beam score by 1 / temperature at every step).  Contract of the ranking, for beam row r (item r / nb,
 * beam j = r % nb) with fp32 logits x[0..V), beam_score[r], temperature > 0, top_k >= 0, 0 < top_p <= 1, a 64-bit seed and step t:
 *   log-prob     lp_i = (x_i - max x) - log(sum exp(x - max x)), fp32, fixed summation order.
 *   temperature  w_i = lp_i * inv_T, inv_T = 1.0f / temperature computed once on the host.
 *   kept set     top-k, then top-p, exactly as in "Sampling" above, on x with inv_T (the softmax of w IS the softmax of x * inv_T),
 *                with min_tokens_to_keep = 2 (transformers' rule for num_beams > 1): top_k = 1 acts as 2, and top-p always keeps
 *                the two largest logits and everything tied with the second.  A -inf logit is never kept.  A row with two
 *                finite logits therefore keeps >= 2 tokens and an item has >= 2 num_beams candidates.  NaN: outside the contract.
 *   score        s_i = beam_score[r] + w_i for kept i, fp32, every operation rounded once.
 *   noise        g_i = -log(-log u_i), u_i = ((word >> 8) + 0.5) * 2^-24 - a 25-bit dyadic number, used EXACTLY (never rounded to
 *                fp32: below 1/2 it is an fp32 number, above it 1 - u_i is, and -log u_i = -log1p(-(1 - u_i))); word = output word
 *                i & 3 of Philox4x32-10 with key = seed (low word, high word) and counter (r, t, i >> 2, 1) - the trailing 1 keeps
 *                the stream apart from the token sampler's (r, t, 0, 0).
 *   key          key_i = s_i + g_i, fp32.
 *   selection    per item: the K = 2 num_beams kept entries of its num_beams rows with the largest keys, equal keys to the lower
 *                flat index j * V + i; emitted in the order s descending, equal s to the lower flat index:
 *                cand_score = s, cand_tok = i, cand_beam = j.
 * Independent Gumbel noise on the scores and the K largest keys are K sequential draws without replacement from softmax(s)
 * (Plackett-Luce) - what torch.multinomial(probs, 2 * num_beams) gives beam_sample.  Everything behind the ranking is
 * rgrg_decoder_beam_search's: BeamSearchScorer.process / finalize, the ancestor table, early stopping, the length penalty,
 * num_return_sequences.  t is the device step word (0 for the first generated token).  Runs on every step plan, precision mode and
 * K/V cache format; the step is captured once per (rows, num_beams) under a key of its own - never shared with a plain or grouped
 * beam step - and reads seed and parameters from a device block, so it serves every seed and parameter set.  Deterministic: the
 * same inputs give the same ids.
 *   RGRG_EINVAL (with a message): num_beams < 2 or > 16 (the row candidate lists hold 32 entries); num_return_sequences outside
 *   1 .. num_beams; temperature not a finite float > 0; top_k < 0; top_p outside (0, 1]. */
int rgrg_decoder_beam_sample(rgrg_decoder* d, const float* feats, int S, int num_beams, int max_length, int early_stopping,
                             float length_penalty, int num_return_sequences, float temperature, int top_k, float top_p, uint64_t seed,
                             int64_t* out_ids, int out_ld, int* out_len, void* stream);
/* ... from a prompt: the prompt arguments, mask rules and refusals of rgrg_decoder_beam_search_prompted (max_length < T + 1, the mask
 * refusals, the e4m3 K/V cache in use for S * num_beams rows) on top of the refusals above.  The first ranking, of the item's last
 * prompt position on num_beams identical rows with beam scores [0, -1e9, ...], uses t = T - 1: a [S,1] BOS prompt with a mask of
 * ones returns the ids of rgrg_decoder_beam_sample. */
int rgrg_decoder_beam_sample_prompted(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask, int S,
                                      int T, int num_beams, int max_length, int early_stopping, float length_penalty,
                                      int num_return_sequences, float temperature, int top_k, float top_p, uint64_t seed,
                                      int64_t* out_ids, int out_ld, int* out_len, void* stream);
/* Test hook: the two launches of that ranking alone on caller buffers, through the decoder's launcher.  logits f32 [S * nb][ld]
 * (2 <= V <= 53248, ld >= V; 16-byte loads when ld % 4 == 0 and logits is 16-byte aligned), beam_scores f32 [S * nb]; row s * nb + j
 * draws with the counter row row0 + s * nb + j at step `step` -> out_score f32 / out_tok i32 / out_beam i32 [S][2 nb]; row_key /
 * row_s f32 and row_tok i32 [S * nb][32], all three or none: the 2 nb largest keys of every row, key descending, with their s and
 * token ((-inf, -inf, 0) where a row keeps fewer than 2 nb tokens).  nb <= 16.  Synchronizes the stream. */
int rgrg_debug_beam_sample_rank(const float* logits, int64_t ld, int V, int S, int nb, const float* beam_scores, float temperature,
                                int top_k, float top_p, uint64_t seed, int step, int row0, float* out_score, int* out_tok, int* out_beam,
                                float* row_key, float* row_s, int* row_tok, void* stream);
/* Test hook: beam_group_merge_kernel alone on caller buffers.  row_max / row_logsum / beam_scores f32 [S * nb], top_val f32 /
 * top_tok i32 [S * nb][32] (rows as wide as in the decoder, the first 2 nb entries used) -> out_score f32 / out_tok i32 /
 * out_beam i32 [S][2 nb] (out_beam: the row within the item).  nb <= 16, G divides nb.  Synchronizes the stream. */
int rgrg_debug_beam_group_merge(const float* row_max, const float* row_logsum, const float* top_val, const int* top_tok,
                                const float* beam_scores, int S, int nb, int G, float penalty, int V, float* out_score, int* out_tok,
                                int* out_beam, void* stream);
/* Test hooks: the rank and arg-max kernels of greedy and plain beam search alone on caller buffers.  Each goes through the launch
 * the decoder makes (the beam hooks through the decoder's own choice of kernel), synchronizes the stream, and refuses with
 * RGRG_EINVAL, before any launch, what would let a kernel leave the caller's buffers: a NULL pointer and the cases named below.
 *
 * rgrg_debug_beam_row_topk: per row of logits f32 [rows][ld] (columns V .. ld - 1 are never read), K = 2 num_beams:
 *   row_max [rows] = the maximum; row_logsum [rows] = log(sum(exp(x - max))) in fp32 (fixed summation order; a -inf logit counts
 *   as zero mass - at least one logit of the row must be finite); top_val / top_tok = the K best (value descending, ties to the
 *   lower token; +0.0 and -0.0 are equal), the value bits as read.  K <= 32: beam_row_topk_kernel<8,1024> (K <= 8), <16,1024>
 *   (K <= 16), <32,512>, candidate rows 32 wide (entries K .. 31 untouched); K > 32: beam_row_topk_wide_kernel, rows K wide.
 *   A -inf logit is never listed, so a row needs K logits above -inf.  With RGRG_DEBUG_BEAM_WIDE=1 in the environment (read by
 *   these two hooks only, at every call) the wide kernels run at K <= 32 as well, on rows K wide.
 *   RGRG_EINVAL: V < 1, ld < V, rows < 1, K < 2, K odd, K > V.
 * rgrg_debug_beam_merge: per item s of S, from the nb rows s * nb .. of such lists (K = 2 nb): score = ((v - row_max) - row_logsum)
 *   + beam_score per candidate, fp32, each operation rounded once; the K best by (score descending, flat index beam * V + token
 *   ascending) -> out_score f32 / out_tok i32 / out_beam i32 [S][K] (beam: the row within the item).  nb <= 16: beam_merge_kernel on
 *   rows 32 wide; wider: beam_merge_wide_kernel on rows K wide with score_scratch f32 [S][nb * K] (required, unused when nb <= 16).
 *   RGRG_EINVAL: S outside 1 .. 65535, nb < 1, V < 2 nb.
 * rgrg_debug_logits_candidates: logits_candidates_kernel as the tiled greedy step launches it, NT = ceil(V / 32) and a (4, rows) grid:
 *   cand_val f32 / cand_idx i32 [rows][NT] = maximum and first column holding it of every 32-column tile, columns >= V left out.
 *   The kernel reads whole tiles with 16-byte loads: RGRG_EINVAL for ld < V, ld < 32 NT, ld % 4 != 0, logits not 16-byte aligned,
 *   V < 1, rows outside 1 .. 65535.
 * rgrg_debug_argmax_update: argmax_update_kernel over cand_val / cand_idx [S][NT] - the row's token is the cand_idx of its largest
 *   cand_val, ties to the lower cand_idx (a row of -inf candidates is such a tie: its lowest cand_idx, which is column 0 behind
 *   logits_candidates_kernel) - with the bookkeeping of a greedy step at t = *step: a
 *   finished row takes PAD; ids[s][t + 1] = token; EOS finishes the row; the last row to arrive sets *done_len = t + 2 if every row
 *   is finished and *done_len was 0, *step = t + 1 and sync[0] = 0 (sync[0] must be 0 at the call).  ids int64 [S][ld_ids].
 *   RGRG_EINVAL: NT < 1, S outside 1 .. 65535, *step (read back before the launch) outside 0 .. ld_ids - 2. */
int rgrg_debug_beam_row_topk(const float* logits, int ld, int V, int rows, int K, float* row_max, float* row_logsum, float* top_val,
                             int* top_tok, void* stream);
int rgrg_debug_beam_merge(const float* row_max, const float* row_logsum, const float* top_val, const int* top_tok,
                          const float* beam_scores, int S, int nb, int V, float* score_scratch, float* out_score, int* out_tok,
                          int* out_beam, void* stream);
int rgrg_debug_logits_candidates(const float* logits, int ld, int V, int rows, float* cand_val, int* cand_idx, void* stream);
int rgrg_debug_argmax_update(const float* cand_val, const int* cand_idx, int NT, int64_t* ids, int ld_ids, int* finished, int* step,
                             int* done_len, int* sync, int S, void* stream);
/* Opt-in reduced precision for MANY sequences (BASELINE configs[2], batch 32): mode 1 (bfloat16) / 2 (float16) makes the
 * > 128-row paths run their projections on the 16-bit MFMA (16-bit weights and GEMM inputs, fp32 accumulate / LayerNorm /
 * softmax / residual) and keep the decode K/V cache in that type (what the reference's torch.autocast does to `present`);
 * 0 = fp32.  NOT bit-exact with the fp32 reference; the <= 128-sequence decode path (launch-latency bound) always stays
 * fp32.  May allocate and synchronise (a change of the 16-bit type re-converts the weight copies). */
int rgrg_decoder_set_precision(rgrg_decoder* d, int mode);
/* Opt-in 8-bit K/V cache for the many-sequence decode step: fmt 1 keeps the cache as plain OCP e4m3fn bytes (no scales)
 * WHEREVER THE 16-BIT CACHE WOULD BE USED - precision mode 1 / 2 with more rows than rgrg_decoder_row_limit(), in
 * rgrg_decoder_generate / _sample / _beam_search; fmt 0 (default): the cache follows the precision mode.  Anything else is
 * RGRG_EINVAL.  fp32 mode, the fused plans of <= row-limit rows, rgrg_decoder_forward_cached and the teacher-forced passes are
 * not affected by the setting.  k / v (and the image key / value of slot 0) are clamped to +-448 and rounded ONCE from fp32 to
 * nearest even; the softmax, the accumulation and the output stay as in the 16-bit mode (what the reference's
 * GPT2PseudoAttention does with `present`, src/language_model/language_model.py:162-166, in a narrower storage type).  The setting
 * survives rgrg_decoder_set_precision; a change drops the captured step graphs and invalidates rgrg_decoder_copy_last_logits. */
int rgrg_decoder_set_kv_format(rgrg_decoder* d, int fmt);
/* The cache format a decode step over `rows` token rows uses in the decoder's current modes: 0 fp32, 1 bf16, 2 fp16, 3 e4m3
 * (-1 for a null handle or rows <= 0). */
int rgrg_decoder_kv_format_in_use(rgrg_decoder* d, int rows);
/* Replaces LanguageModel.forward(input_ids, attention_mask, image_hidden_states, return_loss, use_cache=False)
 * in eval mode (src/language_model/language_model.py:258-399): one teacher-forced pass over
 * T tokens per sequence - feature_space_transformation_nn, wte[ids] + wte[arange(T)] (:298-307), 24 blocks of
 * pseudo self-attention without cache (image key/value first, future columns -1e4, additive padding mask
 * (1 - [1|attention_mask]) * -10000, :84-160,:325-334), final LayerNorm, lm_head.
 *   feats [S,1024] f32, input_ids [S,T] int64 (every id in [0, vocab)), attention_mask [S,T] f32 or NULL (= ones),
 *   S <= max_seqs of the decoder, T <= 1023 (T + 1 keys <= GPT-2's 1024 positions; beyond 256 keys the attention
 *   recomputes its score tiles instead of holding them in registers).
 *   logits_out: NULL or f32 [S,T,vocab] (return_loss=False);
 *   loss_out:   NULL or one f32 = CrossEntropyLoss(ignore_index=-100) of logits[:, :-1] against input_ids[:, 1:]
 *               with the labels of attention_mask == 0 positions ignored (:368-396); nan when no label is scored.
 * Runs on the decoder's stream between two event edges with `stream`; does not synchronise the host.  Work space
 * for S*T token rows is grown on demand (first call of a larger size allocates). */
/* position_ids of the teacher-forced passes (src/language_model/language_model.py:293-307 embeds whatever it is given; the
 * default is arange(T)): int64 device array of S * T entries (per sentence) or T entries (one row, broadcast over the
 * sentences), consumed by the NEXT rgrg_decoder_lm_forward / rgrg_decoder_lm_loss_grad call; NULL restores the default.  Like the
 * reference's, they index the TOKEN table (wte[position_ids], :307) and are range-checked on the device with the token ids. */
int rgrg_decoder_set_lm_positions(rgrg_decoder* d, const int64_t* pos, int64_t n);
int rgrg_decoder_lm_forward(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask,
                            int S, int T, float* logits_out, float* loss_out, void* stream);
/* Replaces `language_model_loss.backward()` of the training loop (src/full_model/train_full_model.py:172-208) for the
 * decoder: the same teacher-forced pass as rgrg_decoder_lm_forward, keeping the activations, followed by the backward
 * pass.  Only what the reference trains in the language model receives a gradient: uk / uv of every
 * GPT2PseudoAttention (src/language_model/language_model.py:50-57) and feature_space_transformation_nn (:230-236);
 * every other GPT-2 tensor is frozen there (:207-213), so the 24 blocks only propagate activation gradients
 * (dX = dY W on transposed weight copies made at the first call).
 *   loss_scale    d(total_loss)/d(language_model_loss), e.g. the loss weight (and an AMP scale)
 *   dropout_p     0 = deterministic pass.  > 0: GPT-2's four dropout sites of train mode (embedding `drop` :311,
 *                 attn_dropout on the probabilities :116, resid_dropout :178, the MLP's dropout) with a counter-based
 *                 generator: mask = f(dropout_seed, layer*4 + site, element index) (Philox4x32-7: counter = index / 4,
 *                 word index % 4), recomputed by the backward pass; torch's generator stream cannot be reproduced, so
 *                 the masks differ from the reference's (rgrg_dropout_mask_f32 exports them for checks).
 *   dropout_seed  a fresh value per call
 *   loss_out      one f32, the unscaled loss
 *   grad_ukv_w    f32 [n_layer*2*1024, 1024]  rows = [uk_0; uv_0; uk_1; uv_1; ...]      grad_ukv_b  f32 [n_layer*2*1024]
 *   grad_fst0_w/b, grad_fst2_w/b   f32 [1024,1024] / [1024]  (Linear 0 and 2 of feature_space_transformation_nn)
 * Gradients are WRITTEN (not accumulated).  T <= 1023 (the reference's own limit).  Allocates work space on demand (~0.9 MB per token row). */
int rgrg_decoder_lm_loss_grad(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const float* attention_mask,
                              int S, int T, float loss_scale, float dropout_p, uint64_t dropout_seed, float* loss_out,
                              float* grad_ukv_w, float* grad_ukv_b, float* grad_fst0_w, float* grad_fst0_b, float* grad_fst2_w,
                              float* grad_fst2_b, void* stream);
/* Measurement hook of bench.py's BASELINE configs[4] leg: the frozen-weight GEMMs of ONE training step of the 16-bit
 * (torch.autocast) flow - forward and activation-gradient GEMMs of the 24 blocks, lm_head forward / dgrad - launched back to
 * back on the decoder's stream between two HIP events, on the work space of the last rgrg_decoder_lm_loss_grad call of this
 * shape (overwritten: timing only).  flops_per_step = 2 M N K of those launches. */
int rgrg_decoder_time_train_gemms(rgrg_decoder* d, int S, int T, int iters, float* ms_per_step, double* flops_per_step,
                                  int* launches_per_step);
/* The dropout mask of one site as the training pass computes it: out[i] = 0 (dropped, probability p) or 1/(1-p), for the
 * flat element index i of the site's tensor ([S*T,1024] for sites 0/2/3, [S,16,T,T+1] for the attention probabilities);
 * stream_id = layer*4 + site; row_len = T + 1 for the attention probabilities (their generator index pads a row of keys to
 * a multiple of 4), 0 otherwise. */
int rgrg_dropout_mask_f32(uint64_t seed, uint32_t stream_id, float p, int64_t n, int row_len, float* out, void* stream);
/* Replaces the INCREMENTAL form of LanguageModel.forward - use_cache=True with or without past_key_values
 * (src/language_model/language_model.py:258-366, :396-399), the call the reference's own generate loop makes every step -
 * over this decoder's pre-allocated K/V cache instead of concatenated tensors.  past_len = number of tokens already in the
 * cache (0: feats [S,1024] must be given, the image key / value goes to slot 0, :135-157; > 0: feats must be NULL).  The T
 * tokens input_ids [S,T] (int64) go to cache slots past_len + 1 .. past_len + T; their embedding is wte[token] +
 * wte[position] with position = position_ids[s][j] (int64 [S,T] on the device, any values in [0, vocab): :293-307) or, when
 * position_ids is NULL, past_len + j (what prepare_inputs_for_generation passes, :498-520); each appends its key / value;
 * logits_out f32 [S,T,vocab] receives lm_logits of every fed position.  past_len + T <= the decoder's max_len.
 * attention_mask: NULL (all ones: generation) or f32 [S][past_len + T] over ALL token keys so far - the reference adds
 * (1 - mask) * -1e4 to the scores of a masked key for every query, the image key is never masked (:316-334).  The mask is
 * applied by the fp32 attention kernel only: in precision mode 1 / 2 (rgrg_decoder_set_precision) with S above
 * rgrg_decoder_row_limit() the step would read the 16-bit K/V cache, whose kernel has no mask operand, so a non-NULL
 * attention_mask then FAILS with RGRG_EINVAL (rgrg_last_error() says so) before anything is launched - it never returns
 * unmasked logits.  Set precision mode 0 first (the Python layer does).  Runs on the decoder's stream between two event edges
 * with `stream`. */
int rgrg_decoder_forward_cached(rgrg_decoder* d, const float* feats, const int64_t* input_ids, const int64_t* position_ids,
                                const float* attention_mask,
                                int S, int T, int past_len, float* logits_out, void* stream);
/* Device address and geometry of one cache plane (layer, kv = 0 key / 1 value): f32 [max_seqs][16][slots][64]; the host
 * wraps rows [:S], slots [:1 + tokens] as the `presents` views of forward(use_cache=True) - no copy. */
int rgrg_decoder_cache_plane(rgrg_decoder* d, int layer, int kv, void** ptr, int* max_seqs, int* slots, int* is_bf16);
/* Token ids of the two teacher-forced entries above are validated ON THE DEVICE (no host round trip per call): an id
 * outside [0, vocab) is clamped for every load (embedding row, cross-entropy label), the loss AND the gradients of that
 * pass come out as NaN, and the NEXT decoder call that finds the (asynchronously mirrored) error word set fails with
 * "index out of range in self" (torch.nn.Embedding's IndexError in the Python layer).  This entry synchronises the
 * decoder's stream and hands the pending error over (*pending = 1, cleared) - the host calls it before it destroys a
 * decoder so that the report is not lost with the object. */
int rgrg_decoder_take_id_error(rgrg_decoder* d, int* pending);
/* After an optimizer step changed the trainable decoder weights IN PLACE (the fst0/fst2/ukv pointers given to
 * rgrg_decoder_create): rebuild the kernel-side copies derived from them (packed skinny layouts, transposes). */
int rgrg_decoder_refresh_trainable(rgrg_decoder* d, void* stream);
/* Building blocks of the two region classifiers' backward pass (the autograd of
 * src/binary_classifier/binary_classifier_region_selection.py:32-44 and binary_classifier_region_abnormal.py:32-47
 * inside train_full_model.py:208 `backward()`); the GEMMs are rgrg_linear_f32 on transposed operands.
 *   rgrg_transpose_pad_f32: dst[c][r] = src[r][c], r < rows; 0 for rows <= r < rows_padded  (dst [cols, rows_padded])
 *   rgrg_colsum_f32:        out[c] = sum_r src[r][c]                                      (bias gradients)
 *   rgrg_relu_backward_f32: d[i] = 0 where h[i] <= 0                                      (h = post-ReLU activation)
 *   rgrg_bce_with_logits_masked_backward_f32: d(mean BCEWithLogits(pos_weight) over mask != 0)/d logits * scale,
 *                           written to dlogits[i*ld] (0 on unmasked rows) */
int rgrg_transpose_pad_f32(const float* src, float* dst, int rows, int cols, int rows_padded, void* stream);
int rgrg_colsum_f32(const float* src, float* out, int rows, int cols, void* stream);
int rgrg_relu_backward_f32(float* d, const float* h, int64_t n, void* stream);
int rgrg_bce_with_logits_masked_backward_f32(const float* logits, const uint8_t* mask, const uint8_t* target, float pos_weight,
                                             int n, float scale, float* dlogits, int ld, void* stream);
/* Replaces torch.optim.AdamW.step() for one parameter tensor (train_full_model.py:409, decoupled weight decay):
 *   p *= 1 - lr*wd; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * with g = grad * grad_scale (1/AMP-scale, 1/accumulation steps).  All arrays f32 [n]; step t >= 1. */
int rgrg_adamw_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);
/* The same update for n_items tensors in ceil(n_items / 64) launches (hyper-parameters and step shared): `items` = a HOST array
 * of records of five 64-bit words {param, grad, exp_avg, exp_avg_sq (device pointers to f32), element count}; the records
 * travel in the kernel arguments. */
int rgrg_adamw_multi_step_f32(const void* items, int n_items, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int step, float grad_scale, void* stream);
/* The 16-bit entry points below (names say bf16 for history) take `fp16`: 0 = bfloat16, 1 = IEEE float16 - the dtype of the
 * caller's torch.autocast (the reference's scripts use float16: generate_reports_for_images.py:108, train_full_model.py:172).
 * Storage is uint16_t bits either way; the matrix core runs v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x16_f16 (same rate),
 * fp32 accumulate; conversions round to nearest even, fp16 overflows to inf beyond 65504 as torch's does.
 * fp32 -> 16 bit, and Y = act(r16(A) Wb^T + shift + R) (A fp32 [M,K], Wb 16-bit [N,K], K % 64 == 0). */
int rgrg_f32_to_bf16(const float* src, uint16_t* dst, int64_t n, int fp16, void* stream);
int rgrg_bf16_to_f32(const uint16_t* src, float* dst, int64_t n, int fp16, void* stream);   /* exact widening */
/* Replaces nn.Conv2d + eval BatchNorm2d (+ residual add) + ReLU of the ResNet-50 bottlenecks and the RPNHead convs
 * (src/object_detector/object_detector.py:51-62,219; custom_rpn.py:61) WHEN THE CALLER RUNS UNDER torch.autocast
 * (generate_reports_for_images.py:108: the reference's detector then computes in half precision): implicit GEMM on
 * v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogue.
 *   X16 [B,H,W,Cin] bf16 NHWC, Cin % 64 == 0, with 128 ZERO elements in front of it in memory (X16[-128..-1] == 0:
 *       the line padding taps read); Wb [Cout][KH][KW][Cin] bf16 with the BatchNorm scale folded in; shift f32 [Cout] or
 *       NULL; R16 bf16 [B,OH,OW,Cout] or NULL; the result goes to Y (f32) or Y16 (bf16), exactly one non-NULL. */
int rgrg_conv2d_nhwc_bf16(const uint16_t* X16, const uint16_t* Wb, const float* shift, const uint16_t* R16, float* Y,
                          uint16_t* Y16, int B, int H, int Wd, int Cin, int Cout, int KH, int KW, int stride, int pad,
                          int act, int fp16, void* stream);
int rgrg_linear_bf16w_f32(const float* A, const uint16_t* Wb, const float* shift, const float* R, float* Y, int M,
                          int N, int K, int ldy, int act, int fp16, void* stream);
/* The same product with BOTH operands already bf16 in device memory (A16 [M,K], Wb [N,K], K % 256 == 0): the
 * LDS-DMA kernel of the opt-in bf16 decode / box-head paths (operands go HBM -> LDS without touching registers, 4 LDS
 * stages in flight across the barriers).  fp32 accumulate; epilogue shift [N] / residual R fp32 [M,ldy] / activation
 * in fp32; the result is stored as fp32 (Y) or as bf16 (Y16, feeds the next GEMM) - exactly one of them non-NULL. */
int rgrg_linear_bf16_f32(const uint16_t* A16, const uint16_t* Wb, const float* shift, const float* R, float* Y,
                         uint16_t* Y16, int M, int N, int K, int ldy, int act, int fp16, void* stream);
/* Measurement hook (tools/gemm_bf16_bench.py): the LDS-DMA kernel with a forced configuration: tile = shape + 16 * stages
 * (shape 0 heuristic, 1 128x128, 2 64x64, 3 128x64, 4 64x128, 5 the 256x256 ping-pong kernel; stages 0 = 4, or 2 / 3 / 4 LDS
 * stages) and operand row
 * pitches lda / ldw in elements (0 = K). */
int rgrg_debug_linear_bf16_tile(const uint16_t* A16, const uint16_t* Wb, const float* shift, const float* R, float* Y,
                                int M, int N, int K, int ldy, int act, int tile, int lda, int ldw, int fp16, void* stream);
/* Test hook: rgrg_conv2d_nhwc_bf16 on a forced configuration of the LDS-DMA kernel (tile = shape + 16 * stages as above).  Shapes
 * 0 .. 4 only: no other kernel family has a convolution instantiation, every other shape is RGRG_EINVAL.  A K of fewer than
 * stages - 1 tiles of 64 runs with 2 stages, as in every launch. */
int rgrg_debug_conv2d_nhwc_bf16_tile(const uint16_t* X16, const uint16_t* Wb, const float* shift, const uint16_t* R16, float* Y,
                                     uint16_t* Y16, int B, int H, int Wd, int Cin, int Cout, int KH, int KW, int stride,
                                     int pad, int act, int fp16, int tile, void* stream);
/* Test hook: the configuration (shape + 16 * stages, the 2-stage fall-back of a short K applied) the launcher's heuristic picks on
 * the LDS-DMA kernel for a plain or convolution launch of M x N x K (convolution: M = B OH OW, N = Cout, K = KH KW Cin).  For a
 * plain GEMM this is the choice before the 256 x 256 kernel takes the large shapes.  Launches nothing and needs no device. */
int rgrg_debug_bf16_tile_choice(int M, int N, int K);
/* Test / measurement hook for the 16-bit training pass (torch.autocast around the reference's training step,
 * src/full_model/train_full_model.py:172-237): the same GEMM on a forced tile (as above; 5 = the 256 x 256 ping-pong kernel
 * of the large shapes) with the training epilogues - Y (f32) or Y16 (16 bit) = act(A16 Wb^T + shift + R); Ypre16 (optional):
 * the 16-bit value BEFORE the activation (c_fc keeps it for gelu_new'); G16 (optional, no R / act): the result is multiplied
 * by gelu_new'(G16[m, n]) - the activation gradient of GPT2MLP lands directly as d(c_fc output). */
int rgrg_debug_linear_bf16_train(const uint16_t* A16, const uint16_t* Wb, const float* shift, const float* R, float* Y,
                                 uint16_t* Y16, uint16_t* Ypre16, const uint16_t* G16, int M, int N, int K, int ldy, int act,
                                 int tile, int fp16, void* stream);
/* Test hook for the greedy lm_head of the many-sequence 16-bit decode step (src/language_model/language_model.py:420-428:
 * next_token_logits.argmax(-1)): the 256 x 256 GEMM leaves, per row and 256-column tile, the maximum of A16 Wb^T + shift and
 * its column (first maximum wins, like torch.argmax) in cand_val / cand_idx [M][ceil(N / 256)] instead of the logits. */
int rgrg_debug_linear_bf16_argmax(const uint16_t* A16, const uint16_t* Wb, const float* shift, int M, int N, int K,
                                  float* cand_val, int* cand_idx, int fp16, void* stream);
/* Test hooks for the LayerNorm folded around the 16-bit decode GEMMs (transformers GPT2Block: ln_1 -> c_attn, ln_2 -> c_fc;
 * src/language_model/language_model.py:338-366 runs them as separate modules).  rgrg_debug_ln_fold16: wb[n][k] =
 * round16(gain[k] w[n][k]), colsum[n] = sum_k wb[n][k] (of the ROUNDED values), shift[n] = bias[n] + sum_k beta[k] w[n][k].
 * rgrg_debug_linear_bf16_ln: the LDS-DMA GEMM as PRODUCER of the residual stream (Yb16 [M, ldy] = the fp32 result as 16 bit,
 * stats_out [M][16][2] = per-row (sum, sum of squares) of every 64-column block; N == 1024) or as CONSUMER (A16 = the raw
 * 16-bit rows, Wb = the scaled weights, ln_stats = those slots, ln_colsum; K == 1024, no residual):
 * Y = act(rstd_m (A16 Wb^T - mean_m colsum) + shift). */
int rgrg_debug_ln_fold16(const float* w, const float* gain, const float* beta, const float* bias, uint16_t* wb, float* colsum,
                         float* shift, int N, int K, int fp16, void* stream);
int rgrg_debug_linear_bf16_ln(const uint16_t* A16, const uint16_t* Wb, const float* shift, const float* R, float* Y,
                              uint16_t* Yb16, float* stats_out, const float* ln_stats, const float* ln_colsum, int M, int N,
                              int K, int ldy, int act, int fp16, void* stream);
/* rgrg_debug_linear_bf16_ln_kv: the CONSUMER as the many-sequence decode step launches c_attn (N = 3 * H * 64, K == 1024): the q
 * columns go to Y [M, ldy] as fp32; the k / v columns (GPT2PseudoAttention's `present`, :162-166) are rounded to the 16-bit type
 * and stored to slot *step_dev + 1 of kcache / vcache [rows][H][T_slots][64] (row m of the GEMM = cache row m), not to Y. */
int rgrg_debug_linear_bf16_ln_kv(const uint16_t* A16, const uint16_t* Wb, const float* shift, float* Y, const float* ln_stats,
                                 const float* ln_colsum, uint16_t* kcache, uint16_t* vcache, const int* step_dev, int M, int H,
                                 int T_slots, int K, int ldy, int fp16, void* stream);
/* The same GEMM variants (plus the plain one with a 16-bit output Y16; exactly one of Y / Y16) on the K-parity ping-pong kernel
 * (csrc/gemm_kp.inc, round 6) when kp != 0 - the kernel the decoder selects for the per-layer projections of the many-sequence
 * 16-bit decode step (GPT2Block's c_attn / c_proj / c_fc / mlp.c_proj, src/language_model/language_model.py:338-366): its tile
 * is a function of (N, K) only, so a row's result does not depend on M.  kp == 0: the LDS-DMA kernel's heuristic. */
int rgrg_debug_linear_bf16_ln_kp(const uint16_t* A16, const uint16_t* Wb, const float* shift, const float* R, float* Y,
                                 uint16_t* Y16, uint16_t* Yb16, float* stats_out, const float* ln_stats, const float* ln_colsum,
                                 int M, int N, int K, int ldy, int act, int fp16, int kp, void* stream);
/* How many GEMM launches of this process took the staged epilogue (csrc/gemm_kp.inc, WIDE: the 64 x 64 producer leaves its tile in
 * LDS and stores whole rows, 16 bytes per lane).  RGRG_WIDE_EPI=0, read per launch, keeps the epilogue that stores from the MFMA's
 * C layout; a test that compares the two reads this counter to know which one a launch ran. */
int rgrg_debug_wide_epilogue_launches(void);
/* How many GEMM launches of this process took a consumer instantiation that knows its activation at compile time (csrc/gemm_bf16.hip,
 * gemm_bf16_glds_kernel CACT: c_fc and c_attn of the many-sequence 16-bit decode step on the 64 x 64 tile; the per-element switch
 * on the run-time `act` is not hoisted by the compiler and costs ~1 us of a 9.5 us launch).  The launcher takes it for a consumer
 * with act NONE or GELU_NEW (NONE with the K/V-cache epilogue), N % 64 == 0, ldy % 8 == 0, 16-byte aligned Y / Y16 / shift /
 * ln_colsum and 8-byte aligned cache planes - the launches of the decode step; everything else keeps the instantiation with the
 * run-time switch.  RGRG_CONS_EPI, read per launch: unset or 1 = as described, 0 = never.  The arithmetic and the bits are the
 * same either way; a test that compares the two reads this counter to know which one a launch ran. */
int rgrg_debug_cons_epilogue_launches(void);
/* Test hooks for the attention kernels (GPT2PseudoAttention, src/language_model/language_model.py: _attn :84-122 - scores / 8,
 * future token columns replaced by -1e4, the additive padding mask (1 - [1 | attention_mask]) * -1e4 of :316-334, softmax,
 * attn_dropout :116, the product with V - and forward :124-160, which puts the image key / value uk(img) / uv(img) in front of
 * the token keys).  Each entry launches the kernels of the product path on the caller's device buffers through the product's own
 * launcher (same instantiation and grid rules); none needs a decoder object.
 * rgrg_debug_attn_decode: ONE decode step of the incremental form (layer_past given, :162-166; greedy_search / beam_search
 * :420-428, _reorder_cache :492-496).  qkv [S][ld_qkv] = q | k | v of the new token; kcache / vcache [S][H][T_slots][64];
 * *step_dev = t: keys are slots 0 .. t + 1, the new key / value is written to slot t + 1 of the row.  src [S][T_slots] (or
 * NULL): the cache row that holds slot j of row s (beam search).  kmask [S][T_slots] (or NULL): additive mask per slot.
 *   kv16 = 0: fp32 cache, attn_decode_kernel<src, ni, kmask>; ni = 9 / 2 keys per group and chunk, 0 = the product's rule
 *             (S * H <= 4096 ? 9 : 2); frag_out = 1: `out` in the fragment-major layout of the fused plan's attn_proj.
 *   kv16 = 1: 16-bit cache (fp16 = 0 bf16 / 1 IEEE half), attn_decode_kv16_wave_kernel<src, fp16>; the result goes to out16
 *             when given, else to out; max_workgroups > 0 caps the grid (RGRG_ATTN_WGS_PER_CU does that in the product).
 *   RGRG_EINVAL: kmask with src, kmask with kv16, H % 4 with kv16, ni outside {0, 2, 9}. */
int rgrg_debug_attn_decode(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* step_dev, float* out,
                           uint16_t* out16, int S, int H, int T_slots, const int* src, const float* kmask, int kv16, int fp16,
                           int ni, int frag_out, int max_workgroups, void* stream);
/* rgrg_debug_attn_decode_qonly: the 16-bit kernel's q-only variant, attn_decode_kv16_wave_kernel<false, fp16, true> - the step behind
 * rgrg_debug_linear_bf16_ln_kv: q [S][ld_q] fp32 (ld_q >= H * 64); the keys are slots 0 .. t + 1 of the cache, slot t + 1 included;
 * nothing is stored to the cache. */
int rgrg_debug_attn_decode_qonly(const float* q, int ld_q, const void* kcache, const void* vcache, const int* step_dev, float* out,
                                 uint16_t* out16, int S, int H, int T_slots, int fp16, int max_workgroups, void* stream);
/* rgrg_debug_attn_decode_first: the 16-bit kernel's padded-prompt variant, attn_decode_kv16_wave_kernel<false, fp16, q_only, true> - the
 * steps of rgrg_decoder_generate_prompted behind a left-padded prompt: first int32 [S], cache slots 1 .. first[s] of row s are left
 * out of the softmax (slot 0, the image, and every later slot are not).  q_only = 0: qkv [S][ld_qkv >= 3*H*64] as in
 * rgrg_debug_attn_decode (the new k / v are stored to slot t + 1); q_only = 1: q [S][ld_qkv >= H*64] as in rgrg_debug_attn_decode_qonly. */
int rgrg_debug_attn_decode_first(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* step_dev, float* out,
                                 uint16_t* out16, int S, int H, int T_slots, const int* first, int fp16, int q_only,
                                 int max_workgroups, void* stream);
/* rgrg_debug_attn_decode_rowstep: the per-row-step variants, attn_decode_kernel<false, ni, false, true> (kv16 = 0) and
 * attn_decode_kv16_wave_kernel<false, fp16, false, false, true> (kv16 = 1) - the steps of rgrg_decoder_generate_rolling: row_step int32
 * [S] on the device replaces *step_dev, row s has the keys of slots 0 .. row_step[s] + 1 and stores its new k / v to slot
 * row_step[s] + 1 of its own row.  A row at step t computes the bits rgrg_debug_attn_decode computes for it at *step_dev = t.
 * Everything else as rgrg_debug_attn_decode (no src, no kmask, no frag_out).  row_step is read back and checked first (the call
 * synchronises `stream`): RGRG_EINVAL for a value outside 0 .. T_slots - 2. */
int rgrg_debug_attn_decode_rowstep(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* row_step, float* out,
                                   uint16_t* out16, int S, int H, int T_slots, int kv16, int fp16, int ni, int max_workgroups,
                                   void* stream);
/* rgrg_debug_attn_decode_rowstep_src: the per-row-step variants WITH the ancestor table, attn_decode_kernel<true, ni, false, true>
 * (kv16 = 0) and attn_decode_kv16_wave_kernel<true, fp16, false, false, true> (kv16 = 1) - the steps of
 * rgrg_decoder_beam_search_rolling: row s reads slot j <= row_step[s] from cache row src[s][j] and stores its new k / v to slot
 * row_step[s] + 1 of its own row.  A row at step t computes the bits rgrg_debug_attn_decode computes for it with the same src at
 * *step_dev = t.  Everything else as rgrg_debug_attn_decode_rowstep.  row_step and src are read back and checked first (the call
 * synchronises `stream`): RGRG_EINVAL for a step outside 0 .. T_slots - 2 and for a table entry of slots 0 .. row_step[s] + 1 outside
 * 0 .. S - 1. */
int rgrg_debug_attn_decode_rowstep_src(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* row_step, const int* src,
                                       float* out, uint16_t* out16, int S, int H, int T_slots, int kv16, int fp16, int ni,
                                       int max_workgroups, void* stream);
/* rgrg_debug_attn_decode_beam_first: a beam step behind a left-padded prompt (rgrg_decoder_beam_search_prompted) - ancestor table
 * src [S][T_slots] AND first int32 [S] together (first is constant inside a beam group in the product; any values in [0, t] here).
 *   kv16 = 1: attn_decode_kv16_wave_kernel<true, fp16, false, true>, slots 1 .. first[s] left out of the softmax;
 *   kv16 = 0: attn_decode_kernel<true, ni, true> on the additive mask the product builds from `first` (-1e4 on slots
 *             1 .. first[s], 0 elsewhere), held in a buffer this call allocates and frees (it synchronises `stream`).
 * Everything else as rgrg_debug_attn_decode (no frag_out).  RGRG_EINVAL: no src, no first, H % 4 with kv16, ni outside {0, 2, 9}. */
int rgrg_debug_attn_decode_beam_first(const float* qkv, int ld_qkv, void* kcache, void* vcache, const int* step_dev, float* out,
                                      uint16_t* out16, int S, int H, int T_slots, const int* src, const int* first, int kv16, int fp16,
                                      int ni, int max_workgroups, void* stream);
/* rgrg_debug_attn_decode_kv8: the same step on an e4m3 cache (rgrg_decoder_set_kv_format), attn_decode_kv8_wave_kernel<src, fp16>:
 * kcache / vcache [S][H][T_slots][64] BYTES; the new k / v are stored to slot t + 1 as clamp(+-448) + one rounding to nearest even;
 * the result goes to out16 (fp16 = 0 bf16 / 1 IEEE half) when given, else to out (fp32); max_workgroups > 0 caps the grid.
 *   RGRG_EINVAL: kmask, H % 4, a plane of 2 GiB or more. */
int rgrg_debug_attn_decode_kv8(const float* qkv, int ld_qkv, uint8_t* kcache, uint8_t* vcache, const int* step_dev, float* out,
                               uint16_t* out16, int S, int H, int T_slots, const int* src, const float* kmask, int fp16,
                               int max_workgroups, void* stream);
/* rgrg_debug_attn_prefill: the attention without layer_past over T tokens (:135-157, :84-122) of rgrg_decoder_lm_forward and
 * the forward half of rgrg_decoder_lm_loss_grad.  qkv [S*T][3*H*64]; ukv [S][ld_ukv], image key at column kcol, image value at
 * kcol + H*64; am [S][T] or NULL; out f32 [S*T][H*64]; out16 (optional) the same as 16 bit; lse (optional) [S*T][H];
 * dropout (seed, stream_id, p) as rgrg_dropout_mask_f32 with row_len = T + 1.  variant 0: the product's rule; 1 / 2:
 * attn_prefill_kernel<3> / <8> (T + 1 <= 96 / 256 keys in registers); 3: attn_prefill_stream_kernel.  RGRG_EINVAL when T + 1
 * keys do not fit the forced variant. */
int rgrg_debug_attn_prefill(const float* qkv, const float* ukv, int ld_ukv, int kcol, const float* am, float* out, uint16_t* out16,
                            float* lse, int S, int H, int T, int variant, uint64_t seed, uint32_t stream_id, float p, int fp16,
                            void* stream);
/* rgrg_debug_attn_backward_f32: the autograd of that attention (loss.backward() of train_full_model.py:208 through :84-160) in
 * fp32: attn_delta_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel.  d_att / att [S*T][H*64] (gradient and value of the forward
 * output), lse from the forward; delta [S*T][H] (written); d_qkv [S*T][3*H*64] or, when d_qkv16 is given, that tensor as 16 bit
 * only; d_ukv [S][ld_ukv]: the image key / value gradient at kcol .. kcol + 2*H*64, times ukv_scale.  H == 16. */
int rgrg_debug_attn_backward_f32(const float* qkv, const float* ukv, int ld_ukv, int kcol, const float* am, const float* d_att,
                                 const float* att, const float* lse, float* delta, float* d_qkv, float* d_ukv, uint16_t* d_qkv16,
                                 int S, int H, int T, uint64_t seed, uint32_t stream_id, float p, int fp16, float ukv_scale,
                                 void* stream);
/* rgrg_debug_attn_train16: the same attention on 16-bit operands (torch.autocast around the training step,
 * train_full_model.py:172-237): backward = 0 runs attn16_fwd_kernel (qkv16, ukv16, am -> att16, lse), backward = 1
 * attn16_bwd_kernel (+ d_att16, att16, lse -> d_qkv16, d_ukv f32 times ukv_scale).  RGRG_EINVAL for T + 1 > 128 keys. */
int rgrg_debug_attn_train16(int backward, const uint16_t* qkv16, const uint16_t* ukv16, int ld_ukv, int kcol, const float* am,
                            uint16_t* att16, float* lse, const uint16_t* d_att16, uint16_t* d_qkv16, float* d_ukv, int S, int H,
                            int T, uint64_t seed, uint32_t stream_id, float p, float ukv_scale, int fp16, void* stream);
/* Test hooks for the row kernels of the training pass (loss.backward() of train_full_model.py:208 through the frozen GPT-2 blocks,
 * src/language_model/language_model.py:338-399).  As above: the product's own launchers on the caller's device buffers, no decoder
 * object; rows are 1024 floats.  Dropout (seed, stream_id, p) as rgrg_dropout_mask_f32 with row_len = 0, indexed by flat element.
 * rgrg_debug_resid_dropout_ln16: resid_dropout_ln16_kernel - x = (resid or 0) + y * mask stored fp32 (y fp32, or y16 in the 16-bit
 *   type; exactly one of them; y may alias x), xn16 = round16(LayerNorm(x) * g + b).
 * rgrg_debug_ln_backward: out = (accumulate ? out : 0) + d(LayerNorm input) for the output gradient dy (fp32) or dy16 (exactly one).
 *   wave_kernel = 0: ln_backward_kernel of the fp32 flow (dy16, out16 or p > 0: RGRG_EINVAL); 1: ln_backward16_kernel, which also
 *   writes out16 = round16(out * mask) when out16 is given.
 * rgrg_debug_ce_rows: the shifted cross entropy (:368-396) on rows [row0, row0 + rows) of M = S * T token rows - ce_valid_kernel over
 *   all M rows, then ce_rows_kernel over the chunk.  logits [rows][ld] = the chunk; ids int64 [M]; am [M] or NULL; row_loss,
 *   row_valid [M]; row_lse [M] or NULL; *id_error is OR-ed with 1 when a label lies outside [0, V).
 * rgrg_debug_ce_finalize: loss = sum(row_loss) / sum(row_valid) (NaN when *id_error), *n_scored = sum(row_valid); either may be NULL.
 * rgrg_debug_ce_backward: d(logits) = (softmax - onehot) * scale / *n_scored on the scored rows of the chunk, 0 on the others, NaN
 *   when *id_error; out16 == NULL: ce_backward_kernel, in place on logits; else ce_backward16_kernel into out16 [rows][ld] (ld % 4 == 0).
 *   Columns [V, ld) are never written.
 * rgrg_debug_gelu: out given: out = gelu_new(pre); d given: d *= gelu_new'(pre); exactly one; n % 4 == 0.
 * rgrg_debug_dropout_add: out = (resid or 0) + src * mask. */
int rgrg_debug_resid_dropout_ln16(const float* y, const uint16_t* y16, const float* resid, float* x, const float* g, const float* b,
                                  uint16_t* xn16, int rows, uint64_t seed, uint32_t stream_id, float p, int fp16, void* stream);
int rgrg_debug_ln_backward(const float* dy, const uint16_t* dy16, const float* x, const float* g, float* out, uint16_t* out16, int rows,
                           int accumulate, uint64_t seed, uint32_t stream_id, float p, int fp16, int wave_kernel, void* stream);
int rgrg_debug_ce_rows(const float* logits, int64_t ld, int V, int row0, int rows, const int64_t* ids, const float* am, int T, int M,
                       float* row_loss, int* row_valid, float* row_lse, int* id_error, void* stream);
int rgrg_debug_ce_finalize(const float* row_loss, const int* row_valid, int n, float* loss, int* n_scored, const int* id_error,
                           void* stream);
int rgrg_debug_ce_backward(float* logits, int64_t ld, int V, int row0, int rows, const int64_t* ids, const int* row_valid,
                           const float* row_lse, const int* n_scored, float scale, const int* id_error, uint16_t* out16, int fp16,
                           void* stream);
int rgrg_debug_gelu(const float* pre, float* out, float* d, int64_t n, void* stream);
int rgrg_debug_dropout_add(const float* src, const float* resid, float* out, int64_t n, uint64_t seed, uint32_t stream_id, float p,
                           void* stream);
/* Test hooks for the kernels that start a decode step and for the bookkeeping kernels between steps (embedding + LayerNorm, the cache
 * writes of the image slot and of a prompt, positions and masks of src/language_model/language_model.py:298-334 and :498-527, the
 * ancestor tables of beam search).  As above: the product's own launchers - its grids, grid-stride loops included - on the caller's
 * device buffers, no decoder object; rows are D == 1024 floats where a D is passed.  Token ids and positions that index a table are the
 * caller's to keep inside it unless the kernel is documented to clamp.  RGRG_EINVAL with rgrg_last_error() set for a missing operand,
 * rows / S / R < 1, D != 1024, fp16 != 0 where no 16-bit output or cache is selected, and what each entry names below.
 * rgrg_debug_ln_rows: ln_rows_kernel - LayerNorm(x[row]) * g + b into xn16 (bf16; fp16 != 0: IEEE half) when it is given, else into xn
 *   (fp32); with both given, as the decode step gives them, xn is not written.
 * rgrg_debug_embed_ln: embed_ln_kernel - x[s] = wte[token] + wte[position] (fp32), token = tok_override[s] or ids[s][*step], position
 *   = pos_override[s] or *step.  Then one of three outputs: stats given: xn16 = round16(x) and stats f32 [rows][16][2] = (sum x, sum
 *   x^2) in slot 0, zeros in slots 1 .. 15; else xn16 given: round16(LayerNorm(x)); else xn (fp32).  An output of another mode that is
 *   given as well is not written.
 * rgrg_debug_embed_seq_ln: embed_seq_ln_kernel over S x T token rows - x = wte[ids] + wte[position], xn = LayerNorm(x); position =
 *   t, or pos_ids[row % pos_rows] with pos_rows == S * T ([S,T]) or T ([1,T] broadcast; anything else: RGRG_EINVAL).  An id or a
 *   position outside [0, V) is clamped (negative: 0, else V - 1) and *id_error is OR-ed with 1; clean inputs leave it alone.
 * rgrg_debug_kv_slot0: kv_slot0_kernel - ukv f32 [S][ld], column (l * 2 + kv) * H * 64 + d -> slot 0 of head d / 64 of cache row
 *   s * row_mul, plane kv of layer l at element l * layer_stride + kv * kv_stride of kv, planes [rows][H][slots][64].  kv_bytes 4: fp32
 *   copy; 2: one rounding to bf16 / fp16; 1: clamp to +-448 and one rounding to e4m3.  RGRG_EINVAL: another kv_bytes, fp16 != 0 unless
 *   kv_bytes == 2, ld < L * 2 * H * 64, strides that let the planes the launch writes overlap.
 * rgrg_debug_decode_reset: decode_reset_kernel - ids [S][ld_ids >= L]: column 0 = BOS, columns 1 .. L - 1 = PAD (both 50256);
 *   finished [S] = 0, *step = 0, *done_len = 0, sync [2] = 0.
 * rgrg_debug_beam_first_mask: kmask f32 [R][slots] = -1e4 on slots 1 .. first[r], 0 elsewhere.
 * rgrg_debug_key_mask: key_mask_kernel - kmask f32 [S][slots] = (1 - am[s][j - 1]) * -1e4 on slots 1 .. L of am f32 [S][L], 0 on the
 *   image slot 0 and behind L (:316-334).
 * rgrg_debug_forward_cached_tokens: tok [S] = ids[s][j] and, with pos_ids, row_pos [S] = pos_ids[s][j] of int64 [S][T], both clamped
 *   into [0, V); *step = position.  Without pos_ids row_pos is not written.
 * rgrg_debug_prompt_mask_scan: pad [S] = the zeros in front of row s of am f32 [S][T]; *flags |= 1 a row of zeros only, 2 a zero
 *   behind a one, 4 some row is padded, 8 a value other than 0 and 1.  The caller clears *flags.
 * rgrg_debug_prompt_setup: prompt_setup_kernel - ids [S][ld_ids >= T] columns 0 .. T - 1 = the prompt clamped into [0, V); *step =
 *   T - 1; with pad [S]: pos int64 [S][T] = t - pad[s], 1 where t < pad[s] (cumsum(mask) - 1, masked_fill 1, :506-509); with kmask
 *   f32 [S][slots]: -1e4 on slots 1 .. pad[s], 0 elsewhere.  RGRG_EINVAL: kmask without pad, pad without pos, kmask with slots <= T.
 * rgrg_debug_prompt_kv_store: prompt_kv_store_kernel - the k and v thirds of qkv f32 [S * T][3 * H * 64] -> slots 1 .. T of cache row
 *   s * row_mul of kplane / vplane [rows][H][slots][64]; kv_bytes 4 (copy) or 2 (one rounding; fp16 as above).  RGRG_EINVAL: slots <= T.
 * rgrg_debug_prompt_last_rows: xn [R][D] (and xn16, when given) = row (r / row_div) * T + T - 1 of xn_all f32 [..][D].
 * rgrg_debug_prompt_step_rows: tok [S] = (int) ids[s][*step], row_pos [S] = *step - pad[s].
 * rgrg_debug_beam_prompt_init: slots 0 .. T of rows 0 .. R - 1 of src_a and src_b int32 [R][slots] = (r / nb) * nb; beam_pad [R] =
 *   pad[r / nb], or 0 without pad.  RGRG_EINVAL: R % nb != 0, slots <= T.
 * rgrg_debug_beam_row_pos: row_pos [R] = *step - beam_pad[r].
 * rgrg_debug_beam_init: slot 0 of every row of src int32 [R][T] = (r / nb) * nb; *step = 0.
 * rgrg_debug_beam_advance: beam_advance_kernel - src_new[r][0 .. t] = src_old[parent[r]][0 .. t], src_new[r][t + 1] = parent[r], t =
 *   *step; tables int32 [R][T].  *step and parent are read back and checked first (the call synchronises): 0 <= *step <= T - 2 and
 *   0 <= parent[r] < R, else RGRG_EINVAL; so is src_old == src_new. */
int rgrg_debug_ln_rows(const float* x, const float* g, const float* b, float* xn, uint16_t* xn16, int fp16, int rows, int D, void* stream);
int rgrg_debug_embed_ln(const float* wte, const int64_t* ids, int ld_ids, const int* step, const int* tok_override, const int* pos_override,
                        const float* g, const float* b, float* x, float* xn, uint16_t* xn16, float* stats, int fp16, int rows, int D,
                        void* stream);
int rgrg_debug_embed_seq_ln(const float* wte, const int64_t* ids, const int64_t* pos_ids, int pos_rows, const float* g, const float* b,
                            float* x, float* xn, int* id_error, int S, int T, int D, int V, void* stream);
int rgrg_debug_kv_slot0(const float* ukv, int ld, void* kv, int64_t layer_stride, int64_t kv_stride, int S, int H, int slots, int L,
                        int row_mul, int kv_bytes, int fp16, void* stream);
int rgrg_debug_decode_reset(int64_t* ids, int ld_ids, int* finished, int* step, int* done_len, int* sync, int S, int L, void* stream);
int rgrg_debug_beam_first_mask(const int* first, int R, int slots, float* kmask, void* stream);
int rgrg_debug_key_mask(const float* am, int L, int S, int slots, float* kmask, void* stream);
int rgrg_debug_forward_cached_tokens(const int64_t* ids, const int64_t* pos_ids, int T, int j, int S, int V, int* tok, int* row_pos,
                                     int* step, int position, void* stream);
int rgrg_debug_prompt_mask_scan(const float* am, int S, int T, int* pad, int* flags, void* stream);
int rgrg_debug_prompt_setup(const int64_t* in, int S, int T, int V, int64_t* ids, int ld_ids, int* step, const int* pad, int64_t* pos,
                            float* kmask, int slots, void* stream);
int rgrg_debug_prompt_kv_store(const float* qkv, void* kplane, void* vplane, int S, int H, int T, int slots, int row_mul, int kv_bytes,
                               int fp16, void* stream);
int rgrg_debug_prompt_last_rows(const float* xn_all, int T, int D, float* xn, uint16_t* xn16, int fp16, int R, int row_div, void* stream);
int rgrg_debug_prompt_step_rows(const int64_t* ids, int ld_ids, const int* step, const int* pad, int* tok, int* row_pos, int S,
                                void* stream);
int rgrg_debug_beam_prompt_init(int* src_a, int* src_b, int slots, int nb, int R, int T, const int* pad, int* beam_pad, void* stream);
int rgrg_debug_beam_row_pos(const int* step, const int* beam_pad, int* row_pos, int R, void* stream);
int rgrg_debug_beam_init(int* src, int T, int nb, int R, int* step, void* stream);
int rgrg_debug_beam_advance(const int* src_old, int* src_new, const int* parent, int* step, int T, int R, void* stream);
/* ---- test hooks of the weight-streaming ("skinny") GEMMs of <= 128 token rows: the fused decode plan (skinny_direct.inc) and the
 * prefill GEMMs (decoder.hip).  No decoder object: device pointers of the caller, launched on `stream`, through the shape rules,
 * packing steps and kernel dispatch of the product path.  Every argument is validated first: RGRG_EINVAL with rgrg_last_error() set
 * for M < 1 or M > 128, an unsupported K, N % 16 != 0 with a fragment-major output / residual / accumulator, a mode / lnf pair the
 * plan does not have, a missing operand, or w16 != 0 on one row tile.
 *
 * Layouts.  Fragment-major [rows][L] (L % 16 == 0): element (row, k) at
 *   ((((row / 32) * 2 + (row % 32) / 16) * (L / 16) + k / 16) * 64 + ((k % 16) / 4) * 16 + row % 16) * 4 + k % 4.
 * Accumulators of a split-K GEMM with N columns: [row tile][2 accumulators][2 row halves][N / 16][64][4] - accumulator p of tile t is
 * the fragment-major block of 32 rows at ((t * 2 + p) * 32 * N) floats.  Packed weights [NT = ceil(N / 16)][K / 16][64 lanes][4]:
 * lane l of (tile, chunk) holds W[tile * 16 + l % 16][chunk * 16 + (l / 16) * 4 .. + 3], zero for rows >= N; 16-bit: same order.
 * Buffer contract: every fragment-major buffer covers ceil(M / 32) * 32 rows; ids (rows of ld_ids) / tok_override / pos_override
 * cover that many entries too and EVERY entry, pad rows included, is a valid row of wte (the kernels read them); the row-major X of
 * rgrg_debug_skinny_linear covers ceil(M / 32) * 32 rows of K floats.  Values in pad rows never reach a stored row < M.
 *
 * rgrg_debug_direct_pack: the one-time packing of make_lin's fused branch and of set_precision's 16-bit copies.  W [N][K]; ln_g / ln_b
 *   (both or neither): the LayerNorm folded into the GEMM; bias [N] or NULL; w16: 0 fp32, 1 bf16, 2 fp16.  K = 1024, or K = 4096 with
 *   N = 1024 and no LayerNorm.  packed (always): fp32 fragments of W o ln_g.  ln_g given: c1 [N] = sum_k fl32(g W), c2 [N] = sum_k
 *   beta W + bias.  w16: packed16 = packed rounded to the type (nearest even); with ln_g also c1_16 [NT * 16] = column sums of the
 *   ROUNDED values.
 * rgrg_debug_direct_linear: ONE launch of the plan's kernel choice (lm_head wave kernel / row-half kernel / generic kernel) on the
 *   operands of rgrg_direct_args; NT and KS follow from N and K as in make_lin.  mode: 0 plain (Xf), 1 combine (Xf + the two
 *   accumulators `part` of a 1024-column producer, (x + acc01) + acc23), 2 / 3 / 4 embedding (wte[ids[row][*step]] + wte[*step];
 *   wte[tok_override[row]] + wte[*step]; wte[tok_override[row]] + wte[pos_override[row]]); modes 1-4 need lnf.  lnf: P holds the
 *   gain-scaled weights, bias = c2 and c1 are required.  w16 != 0: P = packed16 and, with lnf, c1 = c1_16; more than 32 rows only.
 *   K = 4096: the four K slices add into part_out (slices 2p, 2p + 1 into accumulator p, slice 0 with the bias), which the caller
 *   zeroes beforehand; no other output.  Otherwise Y (row-major, ldy >= N) and / or Yf (fragment-major; rows >= M are written as 0)
 *   = act(X W^T + bias + Rf); zero_acc: accumulators (N columns) the epilogue resets; xout (modes 1-4): the rebuilt rows, written
 *   by workgroup (0, 0); cand_val / cand_idx [M][NT]: per 16-column tile the row maximum and its lowest column.  The lm_head wave
 *   kernel (lnf, mode 1, NT > 512, <= 32 rows) writes Y and the candidates only.  *kernel_ran (optional): 0 generic, 1 row half,
 *   2 lm_head wave.
 * rgrg_debug_skinny_linear: Y[:M] = act(X W^T + bias + R) through pack_weights_kernel, launch_skinny_any and (K split over
 *   workgroups) skinny_reduce_kernel with KS / chunks per wave as make_lin derives them; R and Y have row stride ldy >= N.  The
 *   packed weights and partial sums are temporaries of the call, freed after a stream synchronise. */
typedef struct rgrg_direct_args {
    const float* Xf;
    const float* part;
    float* xout;
    const float* wte;
    const int64_t* ids;
    int ld_ids;
    const int* step;
    const int* tok_override;
    const int* pos_override;
    const void* P;
    const float* bias;
    const float* c1;
    const float* Rf;
    float* Y;
    int ldy;
    float* Yf;
    float* part_out;
    float* zero_acc;
    int K, N, act;
    float* cand_val;
    int* cand_idx;
} rgrg_direct_args;
int rgrg_debug_direct_pack(const float* W, const float* ln_g, const float* ln_b, const float* bias, int N, int K, int w16,
                           float* packed, uint16_t* packed16, float* c1, float* c2, float* c1_16, void* stream);
int rgrg_debug_direct_linear(const rgrg_direct_args* args, int mode, int lnf, int w16, int M, int* kernel_ran, void* stream);
int rgrg_debug_skinny_linear(const float* X, const float* W, const float* bias, const float* R, float* Y, int M, int N, int K,
                             int ldy, int act, void* stream);
/* ---- detector targets and losses: ObjectDetector.forward(images, targets), the detector half of
 * ReportGenerationModel.forward(images, image_targets, ...) (src/full_model/report_generation_model.py:55,91 ->
 * src/object_detector/object_detector.py:216-224 -> custom_rpn.py:74-83, custom_roi_heads.py:225-242, and underneath
 * torchvision 0.13.1 det_utils.Matcher / BoxCoder.encode / RegionProposalNetwork.compute_loss / fastrcnn_loss).
 * Matching, the BalancedPositiveNegativeSampler, add_gt_proposals, the gathers of the sampled rows and the losses are all
 * kernels; the caller allocates and passes pointers. */
/* Matcher: gt [B][G][4] (gt_count[b] valid rows), boxes [N][4] per image at boxes + b * box_image_stride floats
 * (stride 0: one shared set, the anchors), box_count[b] valid boxes (NULL: N).  matched [B][N] = index of the best gt
 * (first maximum), -1 below `low`, -2 between; allow_low_quality restores the arg-max of every box that ties a gt's
 * best IoU.  ws_best_per_gt: B * G ints of work space. */
int rgrg_box_match_f32(const float* gt, const int* gt_count, int G, const float* boxes, int64_t box_image_stride,
                       const int* box_count, int B, int N, float high, float low, int allow_low_quality, int* matched,
                       int* ws_best_per_gt, void* stream);
/* det_utils.BalancedPositiveNegativeSampler for B images at once (custom_rpn.py:79: batch 256, half positive;
 * custom_roi_heads.py:225: batch 512, a quarter positive).  The candidates' labels come from the match codes: matched
 * [B][n] (rgrg_box_match_f32), gt_labels [B][G] (NULL: RPN - matched >= 0 is a positive; else the matched box's class:
 * >= 1 positive, 0 negative, < 0 ignored), box_count[b] candidates per image (NULL: n).  Per image num_pos = min(#positive,
 * max_pos), num_neg = min(#negative, batch - num_pos); taken are the candidates with the SMALLEST keys of each class, lower
 * index first on ties: keys [B][n] fp32 when given (tests replay the reference's draws this way), else Philox4x32-10 words
 * of (seed, stage, image, index) - a uniformly random subset like torchvision's randperm()[:k].  ws_keys: B * n words of
 * work space.  mask [B][n]: 0 / 1 sampled positive / 2 sampled negative; list [B][batch]: the sampled indices ascending
 * (torch.where(pos | neg)), zero filled; count [B]. */
int rgrg_balanced_sample(const int* matched, const int64_t* gt_labels, int G, const int* box_count, const float* keys,
                         uint64_t seed, int stage, int B, int n, int batch, int max_pos, uint32_t* ws_keys, uint8_t* mask,
                         int* list, int* count, void* stream);
/* RegionProposalNetwork.compute_loss on the fused head output rpn_out [B * cells][ld] (anchors_per_cell objectness columns,
 * then 4 deltas per anchor) from the sampler's outputs: anchors [A][4] shared by the images, gt [B][G][4]; labels and
 * regression targets (BoxCoder.encode, weights 1) of the sampled anchors are derived in the kernel from mask / matched.
 * out2[0] = loss_objectness (BCE over the sampled anchors, mean), out2[1] = loss_rpn_box_reg (smooth-L1 beta 1/9 over the
 * sampled positives / #sampled); nan when nothing is sampled.  A must be a multiple of anchors_per_cell (RGRG_EINVAL). */
int rgrg_rpn_loss_sampled_f32(const float* rpn_out, int ld, int anchors_per_cell, const int* matched, const float* gt, int G,
                              const float* anchors, const uint8_t* mask, const int* list, const int* count, int B, int A,
                              int batch, float* out2, void* stream);
/* RoIHeads.add_gt_proposals with static shapes: boxes [B][P + G][4] = props[b][:counts[b]], gt[b][:gt_count[b]], zeros;
 * box_count[b] = counts[b] + gt_count[b]. */
int rgrg_roi_add_gt_f32(const float* props, const int* counts, int P, const float* gt, const int* gt_count, int G, int B,
                        float* boxes, int* box_count, void* stream);
/* The sampled rows of RoIHeads.select_training_samples from (boxes, matched, list, count): props_s [B][K][4] zero padded,
 * offsets [B + 1], and in RoI order (row offsets[b] + k) labels_flat [B * K] and reg_targets [B * K][4] =
 * BoxCoder(wx, wy, ww, wh).encode(matched gt box, proposal); rows from offsets[B] on are left untouched. */
int rgrg_roi_gather_samples_f32(const float* boxes, const int* matched, const float* gt, const int64_t* gt_labels,
                                const int* gt_count, int G, const int* list, const int* count, int B, int N, int K, float wx,
                                float wy, float ww, float wh, float* props_s, int* offsets, int64_t* labels_flat,
                                float* reg_targets, void* stream);
/* fastrcnn_loss on pred [N][ld] = num_classes logits | num_classes x 4 deltas.  out2[0] = loss_classifier,
 * out2[1] = loss_box_reg. */
int rgrg_fastrcnn_loss_f32(const float* pred, int ld, int num_classes, const int64_t* labels, const float* reg_targets, int N,
                           float* out2, void* stream);

/* Debug/parity taps: logits of the LAST executed step [S, vocab] -> dst (device). */
int rgrg_decoder_copy_last_logits(rgrg_decoder* d, float* dst, int S, void* stream);
/* bench.py roofline, any sequence count / precision mode: `iters` replays of (a) the projection GEMM launches of one
 * decode step for S token rows as the step would launch them, (b) its 24 single-query attention launches at `nkeys`
 * keys per sequence, each family between one pair of HIP events on the decoder's stream.  Returns total ms of each,
 * the algorithmic flops and weight bytes of the GEMMs of ONE step, the K/V cache bytes ONE step reads at `nkeys`
 * keys (24 x 2 x S x 1024 x nkeys x element size - 1 byte when the e4m3 cache is in force), and the GEMM launches per step.  Call after a generate() so that
 * the decoder exists in the wanted precision mode.  one_range != 0: every launch covers all S rows (each kernel alone on the
 * GPU at the step's full size - what a serialising profiler sees of a 1-range step); 0: as the step launches them (the
 * many-sequence 16-bit step runs as concurrent row ranges on forked streams, whose launches overlap). */
int rgrg_decoder_time_step_parts(rgrg_decoder* d, int S, int nkeys, int iters, int one_range, float* ms_gemm, float* ms_attn,
                                 double* gemm_flops, double* gemm_weight_bytes, double* kv_bytes, int* gemm_launches);
/* Measurement hook: `iters` + 1 eagerly enqueued many-sequence decode steps at `nkeys` keys (state of the last generate() of S
 * sequences), the last one with an event behind every launch on the stream it was launched on.  recs [max_recs][3] = (first row
 * of the launch's row range, tag, ms since the step's first launch); tag = layer * 8 + {0 c_attn, 1 attention, 2 attn c_proj,
 * 3 c_fc, 4 mlp c_proj} (GPT2Block, src/language_model/language_model.py:338-366), 1000 embedding, 1001 ln_f, 1002 lm_head,
 * 1003 arg-max + bookkeeping (:629-650). */
int rgrg_decoder_trace_step(rgrg_decoder* d, int S, int nkeys, int iters, float* recs, int max_recs, int* n_out);
/* Measurement hook: `iters` x n_layer single-query attention launches (GPT2PseudoAttention, language_model.py:124-180) of the
 * many-sequence step at `nkeys` keys, asynchronously on `stream` (state of the last generate() of S sequences). */
int rgrg_decoder_attention_only(rgrg_decoder* d, int S, int nkeys, int iters, void* stream);
/* Token rows (sequences x beams) up to which a decode step of d runs the fused fragment-direct plan in its CURRENT precision mode
 * (128 in fp32; under autocast 64: <= 32 rows bit-exact fp32, 33-64 on 16-bit weights); more rows take the many-sequence path.
 * -1 for a null handle.  (No reference counterpart: the reference has one code path, HF GPT-2 modules under torch.autocast.) */
int rgrg_decoder_row_limit(rgrg_decoder* d);
/* Measurement helper (tools/microbench.py; not on the product path): host wall
 * microseconds per kernel of a dependent chain of n trivial kernels; mode 0 = eager on a
 * private stream, 1 = one hipGraph replay, 2 = eager on the null stream. */
int rgrg_debug_chain(int n, int mode, int blocks, float* us_per_kernel);

#ifdef __cplusplus
}
#endif
#endif /* RGRG_HIP_H_ */
