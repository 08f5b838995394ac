/* libovmr_hip.so -- C ABI of the MI355X (gfx950) implementation of OVMR's hot path.
 *
 * The reference (Zehong-Ma/OVMR) has no FFI: its boundary for this path is a set of Python
 * nn.Module methods.  Each entry point below replaces the arithmetic of one of them; the Python
 * layer in ovmr_amd/modules.py keeps the reference's module API on top (INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add).  Paths are relative to the reference root.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless stated otherwise (PyTorch
 *     allocates, passes tensor.data_ptr()); the library owns only its weight arena and workspace;
 *   - every compute call is asynchronous on the caller's hipStream_t, performs no allocation and
 *     no host synchronisation (graph-capturable), and may be called with any batch size up to
 *     what ovmr_finalize() sized the workspace for (larger batches are processed in chunks);
 *   - return value: 0 = ok, otherwise an OVMR_E_* code or a positive hipError_t;
 *     ovmr_last_error(h) returns a message for the last failure on that handle;
 *   - one handle per (device, model, stream user): thread-compatible, not thread-safe.  Calls on ONE handle must be ordered on ONE
 *     stream (or by events): the workspace and the device-side phase counters of ovmr_fused_logits belong to the handle, and two
 *     launches on it in flight at once would corrupt both.  Concurrency = several handles (CustomCLIP.forward_batches uses two);
 *   - fp16 = IEEE binary16 ("half"), the reference's only working OVMR precision
 *     (configs/trainers/MM_CLS_OP/vit_b16_c4_ep50_imagenet21k_pretrain.yaml:42).
 */
#ifndef OVMR_HIP_H
#define OVMR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ovmr_handle ovmr_handle;
typedef void* ovmr_stream;              /* hipStream_t */

enum { OVMR_F16 = 0, OVMR_F32 = 1, OVMR_I64 = 2, OVMR_I32 = 3 };
enum { OVMR_MODE_FUSION = 0, OVMR_MODE_TEXT = 1, OVMR_MODE_VISION = 2, OVMR_MODE_MULTIMODAL = 3 };
enum {
    OVMR_OK = 0,
    OVMR_E_ARG = -1,         /* bad argument / shape            */
    OVMR_E_SHAPE = -2,       /* unsupported dimension           */
    OVMR_E_STATE = -4,       /* weights missing / not finalized */
    OVMR_E_NOMEM = -5,
    OVMR_E_NAME = -6         /* unknown weight name             */
};

/* Architecture, exactly the constructor arguments of CLIP (clip/model.py:717-731) that
 * build_model() infers from a state dict (clip/model.py:899-928), plus the prompt learner's
 * n_ctx (trainers/mm_classifier_one_prompt.py:99) and its fixed 4 aggregator layers (:140). */
typedef struct {
    int embed_dim;            /* 512 (ViT-B), 768 (ViT-L)        */
    int image_resolution;     /* 224 / 336                       */
    int vision_layers;
    int vision_width;         /* heads = width / 64              */
    int vision_patch_size;
    int context_length;       /* 77                              */
    int vocab_size;           /* 49408                           */
    int transformer_width;    /* heads = width / 64              */
    int transformer_layers;
    int n_ctx;                /* visual tokens per class         */
    int agg_layers;           /* 4                               */
} ovmr_model_desc;

int  ovmr_create(const ovmr_model_desc* desc, ovmr_handle** out);
void ovmr_destroy(ovmr_handle* h);
const char* ovmr_last_error(const ovmr_handle* h);
const char* ovmr_version(void);

/* Kernel-variant switch used by tests/bench to A/B implementations: key in {"gemm","attn","ln_fold","xval_fused","gelu_exact","fuse_im2col","enc_chunk","last_q_cls","fused_head","head_max_grid","agg_max_len","gemm_persist"}.
 * "gemm" (default 8): which fp16 GEMM kernel a launch runs, and with which K loop, tile height and cache hints (gemm_f16_route in
 *   csrc/gemm_f16.hip, exported as ovmr_debug_gemm_route):
 *   8 = 256-row LDS-DMA tiles with the ping-pong K loop (half-tile staging, counted waits) and, for latency-bound shapes
 *   (at most one round -- 256 -- of 64 x 64 tiles: the text tower on a few dozen prompts, CLS-row chains), the 64 x 64 kernel that splits K
 *   over its waves; 7 = 8 without that kernel (A/B); 6 = the 256-row tiles with the double-buffered K loop; 9 = the 64 x 64 split-K kernel wherever it takes the shape (tests);
 *   0 = the 128x128 register-staged kernel everywhere (LayerNorm-folding and fused-argmax launches still take the tile kernel).
 *   + 100 (debug hooks): QuickGELU epilogues in the one-rounding form, as "gelu_exact" = 0.
 * "attn" (default 3): which fp16 attention kernel a launch of L tokens and Lq <= L query rows runs (route() in csrc/attention.hip, exported
 *   as ovmr_debug_attention_route; the first line that applies):
 *     every value >= 1, Lq == L <= 32 (truncated text prompts)      the one-wave-per-(sequence, head) kernel, bit-equal to variant 0;
 *     3, no mask, Lq == L, 192 < L <= 208 (ViT-B/16)                the single-pass persistent kernel;
 *     3 or 5, no mask, L >= 256, Lq >= 32 (ViT-L)                   the 32x32x16 flash kernel;
 *     1, 3 or 5, L >= 128                                           the flash-style LDS-DMA kernel;
 *     otherwise, and 0 everywhere                                   the plain flash-style kernel.
 *   4, the number of a retired kernel, is an alias of 3.
 * "ln_fold" (default 1): ln_1 / ln_2 of the fp16 towers are folded into the consuming GEMM where the shape allows
 *   (width % 256 == 0 and >= 256 token rows); 0 runs the separate LayerNorm kernel everywhere.
 * "xval_fused" (default 1): ovmr_xval_counts takes the row argmax inside the logits GEMM's epilogue (the [R, C] logits are never
 *   written); 0 materialises fp16 logits in workspace chunks and runs a row-argmax kernel on them.  Identical counters.
 * "gelu_exact" (default 0): QuickGELU of the c_fc epilogue (clip/model.py:162-164).  1 keeps the three fp16 rounding points of the
 *   reference's fp16 tensors (h(1.702 u), h(sigmoid), h(u s)); 0 evaluates x / (1 + exp(-1.702 x)) in fp32 on the unrounded
 *   linear output and rounds once -- closer to the real function, within a few fp16 steps of the reference's value, and 5 % off
 *   the c_fc launch.
 * "gemm_persist" (default 1): in_proj and c_fc with the LayerNorm folded in, on launches of more 256-row tiles than the 256 CUs, run as a
 *   tile loop of one workgroup per CU (csrc/gemm_f16_v5.hip "Tile loop": the next tile's operands are requested before a tile's results are
 *   converted and stored); 0 launches one workgroup per tile.  Bit-identical.  (The library also exports three test hooks that are not part
 *   of this ABI: ovmr_debug_gemm_plan -- ovmr_debug_gemm_route with this option as an argument and the plan's eleventh field, persist --,
 *   ovmr_debug_gemm_persist and ovmr_debug_gemm_tile_walk; csrc/gemm_f16.hip and csrc/gemm_f16_v5.hip document them.)
 * "fuse_im2col" (default 1): conv1 on fp16 images with 16 x 16 patches -- the patch-embedding GEMM gathers its A rows from the image
 *   tensor inside its K loop; 0 writes the patch matrix out first (what fp32 images and other patch sizes always do).  Bit-identical.
 * "last_q_cls" (default 1): the last vision block (whose output is read at the CLS row only, clip/model.py:423) projects K and V for every
 *   token and Q for the CLS rows alone when a launch sequence holds at least 256 images; 0 projects Q for every token.  Bit-identical.
 * "fused_head" (default 1): ovmr_fused_logits / ovmr_zeroshot_logits as ONE launch (csrc/head_fused.hip: scaled features staged once, the up
 *   to three products on the matrix pipe, both fp16 rounding points of trainers/mm_classifier_one_prompt.py:357-363, softmax and weighted
 *   sum) for up to 256 query rows, or up to 512 rows x 2048 classes; larger calls run scale + GEMMs + softmax as separate launches.
 *   2 = one launch at any size; 0 = never.  The two implementations sum K in different orders: a logit may land on the neighbouring fp16
 *   value (tests/test_hip_parity.py:test_fusion_head_vs_oracle holds both to the oracle).
 * "head_max_grid" (default 0 = one workgroup per tile): caps the one-launch head's grid (tests: workgroups then take several tiles).
 * "agg_max_len" (default 128): the most aggregator rows, n_ctx + shots, one class may bring to ovmr_generate_tokens /
 *   ovmr_generate_tokens_ragged.  128 .. OVMR_AGG_MAX_LEN_CEILING; any other value returns OVMR_E_ARG and leaves the option as it was.  A
 *   chunk whose longest class has at most 128 rows runs attn_f32_small whatever the option says; a longer one runs attn_f32_long (csrc/attention.hip)
 *   for all its classes, each to the same bits.  Set before ovmr_finalize, the aggregator's workspace holds at least one class of that
 *   length; raised afterwards, a class that does not fit the workspace is refused (OVMR_E_SHAPE) before anything launches. */
#define OVMR_AGG_MAX_LEN_CEILING 4096   /* rows per class: keeps a launch's row arithmetic in int and its grid (classes x heads x 32 query tiles) small */
int ovmr_set_option(ovmr_handle* h, const char* key, int value);

/* Weight ingestion -- replaces build_model()/convert_weights()/load_state_dict
 * (clip/model.py:852-873,899-936) and PromptLearner.load_state_dict
 * (trainers/mm_classifier_one_prompt.py:461-493).  `name` is the reference state-dict key
 * ("visual.conv1.weight", "transformer.resblocks.3.attn.in_proj_weight", "text_projection",
 * "logit_scale", ... and, prefixed "prompt_learner.", "cls_token" /
 * "aggregator.resblocks.N.*").  Data is copied (and converted to the reference's dtype policy:
 * Linear/Conv/MHA/proj fp16, LayerNorm + embeddings fp32, aggregator fp32) on `stream`. */
int ovmr_set_weight(ovmr_handle* h, const char* name, const void* data, int dtype,
                    int ndim, const int64_t* shape, ovmr_stream stream);
/* Validates that every tensor is present, builds derived layouts (transposed projections,
 * fp16 positional tables) and sizes the workspace for `max_images` images / `max_prompts`
 * text sequences / `max_classes` classes per call.  Synchronises `stream` once. */
int ovmr_finalize(ovmr_handle* h, int max_images, int max_prompts, int max_classes, ovmr_stream stream);

/* VisionTransformer.forward (clip/model.py:411-428) [+ x / x.norm() when normalize != 0,
 * trainers/mm_classifier_one_prompt.py:244,307].  image: [B,3,R,R] fp16 or fp32 (cast to fp16 on
 * device like image.type(self.dtype), :243/:306); out: [B, embed_dim] fp16. */
int ovmr_encode_image(ovmr_handle* h, const void* image, int image_dtype, int B,
                      void* out_f16, int normalize, ovmr_stream stream);

/* The launch sequences ovmr_encode_image splits a batch of B images into (diagnostics / bench accounting; no reference
 * counterpart: the reference encodes a loader batch in one piece, trainers/mm_classifier_one_prompt.py:243-245): writes up to
 * max_sizes image counts into sizes, returns the number of sequences (-1 before ovmr_finalize). */
int ovmr_encode_plan(const ovmr_handle* h, int B, int* sizes, int max_sizes);

/* TextEncoder.forward (trainers/mm_classifier_one_prompt.py:80-91).  prompts: [N, context_length,
 * transformer_width] fp16 (already embedded); index: [N] int32 row that is projected (EOS for mm
 * prompts, 1+n_ctx for vision prompts, :163-165); seq_len: number of leading positions that must
 * be computed (max(index)+1 <= seq_len <= context_length; the mask is causal so truncation is
 * exact); normalize: 0 = raw, 1 = x/x.norm(), 2 = the double normalisation of get_mm_v_feats
 * (:204,210).  out: [N, embed_dim] fp16. */
int ovmr_encode_text_embedded(ovmr_handle* h, const void* prompts_f16, const int32_t* index, int N,
                              int seq_len, void* out_f16, int normalize, ovmr_stream stream);

/* CLIP.encode_text (clip/model.py:820-833): ids [N, context_length] int64; the projected row is
 * ids.argmax(-1).  normalize as above (the zero-shot text classifier uses 1, :118-126). */
int ovmr_encode_text_ids(ovmr_handle* h, const int64_t* ids, int N, int seq_len,
                         void* out_f16, int normalize, ovmr_stream stream);

/* Several prompt families through the text transformer in ONE pass.  The reference encodes the multimodal prompts, the vision
 * prompts (get_mm_v_feats, trainers/mm_classifier_one_prompt.py:200-212) and the zero-shot text prompts (:118-126) as three
 * separate TextEncoder / encode_text calls; the arithmetic of a sequence does not depend on its neighbours, so here the token
 * rows of all groups share the GEMM launches of every block and only attention, the read-out gather and the projection run per
 * group (each group keeps its own seq_len: truncation to the last needed row is exact under the causal mask, clip/model.py:802-809).
 * A group is EITHER embedded prompts + read-out rows (as ovmr_encode_text_embedded) OR token ids (as ovmr_encode_text_ids).
 * Rows that do not fit the workspace fall back to one pass per group.  Results equal the per-group entry points up to the
 * kernel choice the larger row count implies (1 - cos ~ 1e-6). */
typedef struct {
    const void* prompts_f16;   /* [n, context_length, transformer_width] fp16, or NULL when ids is given */
    const int64_t* ids;        /* [n, context_length] int64, or NULL */
    const int32_t* index;      /* [n] read-out rows (embedded prompts only) */
    int n, seq_len, normalize; /* as the single-group entry points */
    void* out_f16;             /* [n, embed_dim] fp16 */
} ovmr_text_group;
int ovmr_encode_text_groups(ovmr_handle* h, const ovmr_text_group* groups, int n_groups, ovmr_stream stream);

/* ZeroshotCLIP2.build_model (trainers/zsclip.py:85-96): the prompt-ensembled zero-shot text classifier.  ids: [T, C, context_length]
 * int64, template-major (the reference's loop order, :89-91).  seq_lens: HOST array [T], each template's exact length (max EOT
 * position + 1), or NULL for context_length.  out: [C, embed_dim] fp16 = normalise(mean_t normalise(encode_text(ids[t]))) with the
 * reference's fp16 rounding points (:92-96; csrc/text_ensemble.hip lists them).  Per chunk of classes, all T templates go through ONE
 * pass of the text tower as T groups (as ovmr_encode_text_groups with normalize = 0: bit-identical raw rows), then one launch
 * ensembles them; the chunk is sized so that the tower's rows plus a [T, chunk, embed_dim] scratch fit the workspace, so any
 * vocabulary runs without allocation.  OVMR_E_SHAPE when one class's T prompts do not fit; C == 0 returns 0. */
int ovmr_encode_text_ensemble(ovmr_handle* h, const int64_t* ids, int T, int C, const int32_t* seq_lens,
                              void* out_f16, ovmr_stream stream);

/* token_embedding(ids).type(fp16) (trainers/mm_classifier_one_prompt.py:129-130): ids [N, L] int64
 * -> out [N, L, transformer_width] fp16. */
int ovmr_embed_tokens(ovmr_handle* h, const int64_t* ids, int N, int L, void* out_f16, ovmr_stream stream);

/* PromptLearner.forward, visual-token generator part (trainers/mm_classifier_one_prompt.py:167-169):
 * feats [Cb, S, embed_dim] fp16 -> tokens [Cb, n_ctx, embed_dim] fp32 (aggregator in fp32).  The arithmetic mode of the sequence
 * table ovmr_generate_tokens_ragged reads (AggSeqs, csrc/common.h): the same generator, the same kernels (agg_input_kernel,
 * attn_f32_small or, beyond 128 rows per class, attn_f32_long; agg_output_kernel), class c's rows at c * (n_ctx + S) computed, no device
 * array loaded.  OVMR_E_SHAPE before any launch when n_ctx + S exceeds option "agg_max_len" (default 128, at most
 * OVMR_AGG_MAX_LEN_CEILING), or when a chunk's rows do not fit the workspace. */
int ovmr_generate_tokens(ovmr_handle* h, const void* feats_f16, int Cb, int S,
                         float* tokens_f32, ovmr_stream stream);

/* The same generator for classes with their OWN exemplar counts.  trainers/mm_classifier_one_prompt.py:167-169 runs the aggregator
 * over cat([cls_token, feats]) of a [num_cls, num_ins, D] tensor: the reference has no counterpart for unequal counts, it takes
 * num_ins rows of every class by position (:238-245).  Here class c of the call owns shots[c] consecutive rows of feats [R, embed_dim]
 * fp16 (class after class, R = sum of the shots) and the aggregator runs over its n_ctx + shots[c] tokens, no padding and no
 * duplicates.  shots_host: HOST int32 [Cb], read before the call returns (the library plans its chunks -- runs of whole classes whose
 * packed rows fit the aggregator's workspace, at least one class each -- and its grids from it); offsets_dev: DEVICE int32 [Cb + 1],
 * the exclusive prefix sum of the same shots (the kernels index from it; every index made from it is clamped to the call's rows, so
 * two views that disagree give wrong values, never an access outside the buffers).  Asynchronous, allocation-free, capturable.
 * THE CONTRACT: tokens[c] is bit-identical to what ovmr_generate_tokens returns for class c alone with S = shots[c] on the same
 * handle, whatever else shares the call and wherever the chunk boundaries fall; a call whose counts are all S equals the uniform call.
 * OVMR_E_SHAPE before any launch, naming the class: a count < 1, n_ctx + shots[c] above option "agg_max_len" (default 128, at most
 * OVMR_AGG_MAX_LEN_CEILING), a class whose rows do not fit the workspace; also when the shots do not add up to R.
 * Cb == 0 returns 0. */
int ovmr_generate_tokens_ragged(ovmr_handle* h, const void* feats_f16, const int32_t* shots_host, const int32_t* offsets_dev,
                                int Cb, int R, float* tokens_f32, ovmr_stream stream);

/* PromptLearner.update_prompts (:156-157): out[c] = cat(base[row(c)][:2], half(tokens[c]),
 * base[row(c)][2:-n_ctx]); row(c) = labels[c] (int64) or 0 when labels == NULL (the "a ." template
 * broadcast, :173).  base: [*, context_length, width] fp16; out: [Cb, context_length, width] fp16. */
int ovmr_assemble_prompts(ovmr_handle* h, const void* base_f16, const int64_t* labels,
                          const float* tokens_f32, int Cb, void* out_f16, ovmr_stream stream);

/* Cross-validation counts (trainers/mm_classifier_one_prompt.py:261-270): for rows r of
 * feats [R, embed_dim] fp16 with int32 labels [R], logits = logit_scale * feats @ clf^T in fp16
 * (clf [C, embed_dim] fp16), pred = argmax (first index on ties); accumulates
 * n_pred[pred] += 1 and tp[label] += (pred == label) into int32 [C] arrays (caller zeroes). */
int ovmr_xval_counts(ovmr_handle* h, const void* feats_f16, const int32_t* labels, int R,
                     const void* clf_f16, int C, int32_t* tp, int32_t* n_pred, ovmr_stream stream);

/* F1 preference (:268-274): counts int32 [3][2][C] = {mm, vision, text} x {tp, n_pred},
 * n_label int32 [C]; out [C,3] fp32 = softmax(tau * f1) with f1 = 2pr/(p+r), NaN -> 0
 * (torcheval==0.0.7 multiclass_f1_score(average=None)). */
int ovmr_fusion_weights(ovmr_handle* h, const int32_t* counts, const int32_t* n_label, int C,
                        float tau, float* out_f32, ovmr_stream stream);

/* CustomCLIP.forward eval branch (:348-363).  feats [B, embed_dim] fp16 (L2-normalised);
 * mm / v / t classifiers [C, embed_dim] fp16 (unused ones may be NULL for single modes);
 * w [C,3] fp32 (fusion only); out [B,C] fp32 probabilities. */
int ovmr_fused_logits(ovmr_handle* h, const void* feats_f16, int B, const void* mm_f16,
                      const void* v_f16, const void* t_f16, const float* w_f32, int C, int mode,
                      float* out_f32, ovmr_stream stream);

/* All four eval modes of :348-363 from ONE pass over the head (EVAL_MODE all: the four columns of the reference's result tables without
 * four runs).  Operands as for ovmr_fused_logits, all three classifiers and w required.  out_f32: four planes [B, C] fp32 with dense rows,
 * plane p at out_f32 + p * plane_stride, plane_stride >= B * C elements (so a row slice of a [4, Btot, C] tensor can be handed in); the
 * plane index is the OVMR_MODE_* value: 0 fusion = sum_m w[c][m] p_m, 1 text = p_t, 2 vision = p_v, 3 multimodal = p_mm.  Contract: plane p
 * is bit-equal to what ovmr_fused_logits(..., mode = p, ...) writes on the same handle, options and operands.  It takes the implementation
 * ovmr_head_plan(h, B, C) names, under the same options ("fused_head", "head_max_grid", "gemm") and in the same workspace; asynchronous, no
 * allocation, no synchronisation; B == 0 returns 0.  OVMR_E_ARG with nothing written: a NULL classifier, w or output, plane_stride < B * C,
 * C < 1. */
int ovmr_fused_logits_all(ovmr_handle* h, const void* feats_f16, int B, const void* mm_f16, const void* v_f16, const void* t_f16,
                          const float* w_f32, int C, float* out_f32, long plane_stride, ovmr_stream stream);

/* Which implementation ovmr_fused_logits runs for B query rows and C classes on this handle: 1 = the one-launch head, 0 = scale + GEMMs +
 * softmax (-1: bad arguments / not finalized).  Both keep the reference's rounding points (:357-363) but sum K in different orders, so a
 * logit may land on the neighbouring fp16 value: a caller that splits one batch over several calls and promises the unsplit call's bits
 * (CustomCLIP.forward's two halves) splits only where the plan is the same. */
int ovmr_head_plan(const ovmr_handle* h, int B, int C);

/* ZeroshotCLIP.model_inference (trainers/zsclip.py:55-60): out [B,C] fp16 =
 * exp(logit_scale) * feats @ text_feats^T (raw logits). */
int ovmr_zeroshot_logits(ovmr_handle* h, const void* feats_f16, int B, const void* text_f16, int C,
                         void* out_f16, ovmr_stream stream);

/* Class-sharded generation (no counterpart in the reference, which has no distributed path: trainers/mm_classifier_one_prompt.py:414-419
 * wraps the model in nn.DataParallel): a rank's contribution to the job's ONE all-gather.  block [bound, K + 2] fp16 with
 * K = 3 D + n_ctx D: row i < n = mm[c] | v[c] | t[c] | tokens[c] for c = labels[i] (int64 class ids; mm / v / t are the class-indexed
 * [C, D] fp16 buffers of forward_prompt, :216-225, tokens [C, n_ctx, D] fp16) followed by c as an int32 bit pattern in two fp16 columns;
 * rows n <= i < bound are zero with label -1.  D even.  Needs no handle. */
int ovmr_pack_rows(const void* mm_f16, const void* v_f16, const void* t_f16, const void* tokens_f16, const int64_t* labels, int n,
                   int D, int n_ctx, int bound, void* block_f16, ovmr_stream stream);

/* The inverse, on the gathered blocks of all ranks ([rows, K + 2] fp16, rank-major): every row whose label lies in [0, C) is written to
 * row `label` of mm / v / t [C, D] and tokens [C, n_ctx, D]; seen (int32 [C + 1], zeroed by the caller) counts the rows per class -- the
 * job is complete iff seen[c] == 1 for every class (:259) -- and, in seen[C], labels outside [-1, C). */
int ovmr_unpack_rows(const void* gathered_f16, int rows, int C, int D, int n_ctx, void* mm_f16, void* v_f16, void* t_f16,
                     void* tokens_f16, int32_t* seen, ovmr_stream stream);

/* Classification.process of the test loop (Dassl.pytorch/dassl/evaluation/evaluator.py:50-67): outputs [B, C] (fp32 = what
 * CustomCLIP.forward returns, or fp16 = ZeroshotCLIP's raw logits; row stride ld elements), labels int64 [B] (the batch's LongTensor as
 * it is).  pred = outputs.max(1)[1] -- lowest column on ties, a NaN is the largest value -- then counts[0][pred] += (pred == label)
 * (true positives), counts[1][pred] += 1, counts[2][label] += 1; counts is int32 [3][C] followed by ONE more int32 that counts the rows
 * whose label lies outside [0, C) (such rows touch no histogram; the host raises when it is not zero).  The caller zeroes counts once
 * and accumulates over the batches of a test pass: no host round trip per batch (the reference does .item() / .cpu() per batch, :59-67);
 * accuracy, error rate, macro-F1 and the per-class tables of evaluate() (:69-138) are functions of these 3C integers.  Needs no handle. */
int ovmr_eval_counts(const void* outputs, int dtype, long ld, const int64_t* labels, int B, int C, int32_t* counts, ovmr_stream stream);

/* Classification.process(topk > 1) (Dassl.pytorch/dassl/evaluation/evaluator.py:56-58) and ranked prediction: per row of outputs [B, C] (fp16 or
 * fp32, row stride ld >= C elements) the k best columns, best first.  The order is total: larger value first, equal values in increasing
 * column order, every NaN above +inf (NaNs among themselves in increasing column order), -0.0 == +0.0 (ordered by column) -- what
 * torch.sort(descending=True, stable=True) gives on the host, so column 0 is the prediction ovmr_eval_counts counts for the same row.
 * values (may be NULL): the selected elements as fp32 (fp16 converts exactly, a NaN stays a NaN); indices: int32 [B, k].  labels int64 [B]
 * and hits int32 [1] come together or not at all: hits[0] += the number of rows whose label is among the row's k columns (:56-58; a label
 * outside [0, C) never hits; the caller zeroes hits once and accumulates over the batches of a test pass).  1 <= k <= min(C, 32),
 * otherwise OVMR_E_ARG; B == 0 returns 0.  One launch; needs no handle. */
int ovmr_topk_rows(const void* outputs, int dtype, long ld, int B, int C, int k, float* values, int32_t* indices,
                   const int64_t* labels, int32_t* hits, ovmr_stream stream);

/* The evaluator's detail mode: ALL the counting of Classification.process for one batch in one launch -- the per-class results
 * (Dassl.pytorch/dassl/evaluation/evaluator.py:38-40, 69-73, printed by :140-163) and the confusion matrix (:165-171) next to what
 * ovmr_eval_counts and ovmr_topk_rows count; it replaces both launches.  outputs [B, C] fp16 / fp32 with row stride ld >= C elements
 * (rows need no alignment), labels int64 [B], 1 <= k <= min(C, 32).  Per row the k best columns in the total order of ovmr_topk_rows;
 * pred = the best one = the argmax of ovmr_eval_counts.  counts: int32 [3][C] + [1], updated exactly as ovmr_eval_counts does; a row
 * whose label lies outside [0, C) touches nothing but its last slot.  For the other rows, each of the following may be NULL:
 *   hits       int32 [1]      += 1 when the label is among the row's k columns (the hits of ovmr_topk_rows)
 *   class_hits int32 [C]      class_hits[label] += 1 for the same rows: the `matches` of _per_class_res[label] (:69-73); at k == 1 it
 *                             equals counts[0]
 *   cmat       int32 [C][C]   cmat[label][pred] += 1, row-major, 64-bit index arithmetic: _y_true against _y_pred (:62-67)
 * The caller zeroes the buffers once and accumulates over a test pass; integer atomics only, so the result does not depend on the
 * order of execution.  OVMR_E_ARG (nothing is written) for a NULL outputs / labels / counts, ld < C, an unknown dtype or k out of
 * range; B == 0 returns 0.  One launch, no allocation, no host synchronisation; needs no handle. */
int ovmr_eval_detail(const void* outputs, int dtype, long ld, const int64_t* labels, int B, int C, int k, int32_t* counts, int32_t* hits,
                     int32_t* class_hits, int32_t* cmat, ovmr_stream stream);

/* exp(logit_scale) as held by the handle (set through ovmr_set_weight("logit_scale")). */
float ovmr_logit_scale(const ovmr_handle* h);

/* Device half of the test transform -- replaces ToTensor + Normalize of _build_transform_test
 * (Dassl.pytorch/dassl/data/transforms/transforms.py:495-526; mean / std of configs/trainers/MM_CLS_OP/*.yaml:14-15) and the
 * .type(fp16) of trainers/mm_classifier_one_prompt.py:243,306.  u8_hwc: DEVICE uint8 [B, R, R, 3], the decoded, bicubic-resized and
 * centre-cropped images (the host's share of the transform); out_f16: fp16 [B, 3, R, R] = h(((u / 255) - mean[c]) / std[c]), the
 * fp32 arithmetic of torchvision bit for bit.  mean3 / std3 are HOST pointers to three floats.  R % 8 == 0.  Needs no handle. */
int ovmr_preprocess_u8(const void* u8_hwc, int B, int R, const float* mean3, const float* std3, void* out_f16, ovmr_stream stream);

/* Device half of the test transform, first part -- replaces Resize(max(INPUT.SIZE), INPUT.INTERPOLATION) + CenterCrop(INPUT.SIZE) of
 * _build_transform_test (Dassl.pytorch/dassl/data/transforms/transforms.py:495-526; torchvision on PIL images, i.e. PIL.Image.resize +
 * crop) for bicubic and bilinear interpolation, BIT-EQUAL to PIL: PIL's own two integer passes (22-bit fixed-point weights, uint8
 * intermediate) over window / weight tables the host builds exactly as PIL does (ovmr_amd/resize.py).  One job per image:
 *   in_offset   byte offset of its decoded uint8 [h, w, 3] pixels in `pixels` (device)
 *   y0, ny      the input rows the R x R crop window needs;  tmp_offset: byte offset of its [ny, R, 3] intermediate in `tmp`
 *   table       offset (in int32) of its size's table in `tables` (device):
 *               [bounds_h R x 2 (xmin, n) | k_h R x ksize_h | bounds_v R x 2 (ymin - y0, n) | k_v R x ksize_v]
 *   passthrough 1: `pixels` already holds the R x R crop of this image (resized on the host: nearest, or an image too large for the
 *               upload ring) and is copied
 * jobs: DEVICE array of n jobs; max_ny: the largest ny among them; out_u8: DEVICE uint8 [n, R, R, 3], the input of
 * ovmr_preprocess_u8.  Needs no handle. */
typedef struct ovmr_resize_job {
    int64_t in_offset;
    int64_t tmp_offset;
    int32_t w, h;
    int32_t y0, ny;
    int32_t table;
    int32_t ksize_h, ksize_v;
    int32_t passthrough;
} ovmr_resize_job;
int ovmr_resize_crop_u8(const void* pixels, const ovmr_resize_job* jobs, int n, const int32_t* tables, void* tmp, int max_ny,
                        void* out_u8, int R, ovmr_stream stream);

/* Images per launch sequence of ovmr_encode_image after ovmr_finalize (<= max_images): a batch of MORE than max_images images is
 * encoded in chunks of this many (one that fits the workspace is a single launch sequence), chosen so that the 256-row-tile grids of the block GEMMs are whole rounds of the CUs and no launch has more than 600 row tiles (ViT-B/16 on 256 CUs: 775 of a
 * reserve of 775 or more, 665 of 768); ovmr_set_option(h, "enc_chunk", n) pins it (0 = automatic).  Chunks of at least 256
 * token rows give bit-identical features; smaller ones take the small-matrix kernels (other rounding points, same tolerance).
 * 0 before ovmr_finalize. */
int ovmr_encode_chunk(const ovmr_handle* h);

/* Closed-form FLOP counts.  ovmr_flops_per_image is the ALGORITHMIC count of the reference's
 * VisionTransformer.forward (every block over every token, clip/model.py:411-428: 35.127 GFLOP for ViT-B/16);
 * ovmr_flops_per_image_executed is what ovmr_encode_image launches for a batch that fills the reserve: its last block runs
 * attention / out_proj / MLP for the CLS query row only (identical result), ~6 % fewer, and -- in launch sequences of at least 256
 * images -- the Q projection too.  ovmr_flops_executed(h, B) is the count for ONE call of ovmr_encode_image on B images: the plan
 * actually run (ovmr_encode_plan), the 256-image rule applied per launch sequence (a query batch of 128 projects Q for every token). */
double ovmr_flops_per_image(const ovmr_handle* h);
double ovmr_flops_per_image_executed(const ovmr_handle* h);
double ovmr_flops_executed(const ovmr_handle* h, int B);
double ovmr_flops_per_prompt(const ovmr_handle* h, int seq_len);

/* Unit-test hooks: launch ONE kernel (no handle).  f32 selects the fp32 (aggregator) kernels;
 * `variant` selects the kernel implementation as ovmr_set_option does; `epi` is the epilogue id of
 * ovmr_amd/csrc/common.h.  A [M,K], W [N,K], C [M,ldc]; qkv [B*L, 3*H*64] -> out [B*L, H*64].  The *_strided / *_q
 * forms take the operand strides and query counts of the engine's sub-matrix launches.
 * For the LayerNorm-folding epilogues (epi 6/7) ovmr_debug_gemm reads `bias` as the folded bias fp32 [N], `pos` as the
 * column sums fp32 [N] and `res` as the row statistics fp32 [M][K/256][2]; with epi 8 (fused row argmax) C receives
 * fp32 [M][ceil(N/256)][2] = (tile maximum, bits of the lowest column holding it); with epi 3 a non-NULL `pos` receives the
 * statistics of the stored rows, fp32 [M][N/256][2]. */
int ovmr_debug_gemm(int f32, int variant, const void* A, const void* W, const void* bias, const void* res,
                    const void* pos, void* C, int M, int N, int K, int ldc, int epi, float scale,
                    int rows_in, int rows_out, ovmr_stream stream);
/* kernel-test hook for the LayerNorm-folding GEMM epilogues (ovmr_amd/csrc/common.h, EPI_LN_BIAS):
 * x1 = h(h(A1 W1^T + b1) + res) [M,D] (skipped when A1 is NULL: x1 is then an input), C2 = h(LN(x1) W2^T + b2) [M,N2],
 * QuickGELU on top when qgelu != 0.  Mirrors clip/model.py:191-194 (ln_1 + in_proj, ln_2 + c_fc). */
int ovmr_debug_lnfold(int variant, const void* A1, const void* W1, const void* b1, const void* res, int M, int D, int K1,
                      const void* W2, const float* gamma, const float* beta, const void* b2, int N2, int qgelu,
                      void* x1, void* C2, ovmr_stream stream);
int ovmr_debug_layernorm(int f32, const void* x, void* y, const float* g, const float* b, int rows, int D,
                         long in_stride, ovmr_stream stream);
int ovmr_debug_attention(int f32, int variant, const void* qkv, void* out, int B, int L, int H, int causal,
                         ovmr_stream stream);
/* The row kernels either side of the GEMMs, one launcher each (tests/rowops_exact.py states what each must give, bit for bit).
 * OVMR_E_ARG for a NULL pointer, a negative count or a width the kernel's 8-byte accesses do not take (D % 4 != 0).
 *   l2norm          x [rows, D] fp16, in place, x / h(||x||), applied `times` times (what normalize = 1 / 2 of the encoders runs)
 *   text_ensemble   feats [T, rows, E] fp16 -> out [rows, E] fp16 (csrc/text_ensemble.hip); the pointers go to the launcher as they
 *                   are: 16-byte aligned operands with E % 8 == 0 and E <= 1024 take the vector kernels, anything else (an `out`
 *                   that is only 2-byte aligned, for one) the element-wise kernel
 *   text_embed_ids  x[n * Lseq + l] = h(h(tok_emb[ids[n * ids_stride + l]]) + pos[l]) for l < Lseq, index[n] = the first maximum of
 *                   ids[n * ids_stride + 0 .. Lctx); tok_emb fp32 [vocab, D], pos fp16 [>= Lseq, D], Lseq <= Lctx <= ids_stride
 *   text_add_pos    x[n * Lseq + l] = h(prompts[n * Lctx + l] + pos[l]) for l < Lseq
 *   gather_rows     out[n] = x[n * Lseq + clamp(index[n], 0, Lseq - 1)] */
int ovmr_debug_l2norm(void* x_f16, int rows, int D, int times, ovmr_stream stream);
int ovmr_debug_text_ensemble(const void* feats_f16, int T, int rows, int E, void* out_f16, ovmr_stream stream);
int ovmr_debug_text_embed_ids(const int64_t* ids, int ids_stride, const float* tok_emb, const void* pos_f16, void* x_f16, int32_t* index,
                              int N, int Lctx, int Lseq, int D, ovmr_stream stream);
int ovmr_debug_text_add_pos(const void* prompts_f16, int Lctx, const void* pos_f16, void* x_f16, int N, int Lseq, int D, ovmr_stream stream);
int ovmr_debug_gather_rows(const void* x_f16, const int32_t* index, void* out_f16, int N, int Lseq, int D, ovmr_stream stream);
/* The front of the image tower (tests/front_exact.py states what each must give, bit for bit).  OVMR_E_ARG for a NULL pointer, a
 * negative count or a shape the kernel's accesses do not take.
 *   im2col        image [B, 3, R, R] (fp16 or fp32, any element alignment) -> out [B * (R/P)^2, Kpad] fp16: row (b, gy, gx), column
 *                 k = c * P * P + ky * P + kx, +0 from 3 * P * P on; Kpad % 8 == 0, R % P == 0, out 16-byte aligned
 *   fill_cls      x [B * L, W] fp16: row b * L = cls_pos [W], every other row untouched; W % 4 == 0
 *   gemm_patches  the patch-embedding GEMM gathering its rows from the fp16 images (16 x 16 patches, G = R / 16, K = 768):
 *                 C [B * (G*G + 1), N], row b * (G*G + 1) + 1 + p = h(h(patch p of image b . W [N, 768]) + pos [G*G + 1, N] row 1 + p),
 *                 the rows b * (G*G + 1) untouched.  Returns the launcher's rc: -2 for R % 16 != 0 or an image pointer that is not
 *                 16-byte aligned, -4 for B * G*G < 256, N < 128 or images of 2^31 bytes or more (the 256-row kernel alone gathers). */
int ovmr_debug_im2col(const void* image, int image_dtype, int B, int R, int P, int Kpad, void* out_f16, ovmr_stream stream);
int ovmr_debug_fill_cls(void* x_f16, const void* cls_pos_f16, int B, int L, int W, ovmr_stream stream);
int ovmr_debug_gemm_patches(int variant, const void* image_f16, int R, const void* W_f16, const void* pos_f16, void* C_f16, int B, int N,
                            ovmr_stream stream);
/* ovmr_debug_gemm (fp16 kernels) with explicit strides: A [M, lda], W [N, ldw], res [M, ldres], C [M, ldc] -- the sub-matrix
 * launches of the last vision block (CLS-row Q with A strided by a sequence, K/V written next to Q, out_proj reading the residual
 * of the CLS rows from the token rows).  For epi 6/7, W [N,K] and bias fp16 [N] are the RAW weight and bias: they are folded with
 * gamma / beta fp32 [K] in scratch allocated here, the row statistics are taken over the dense buffer A strides over
 * (lda = row_step * K, ldw = K, K % 256 == 0) and read every row_step rows, as the CLS-row Q launch does (row_step = L).
 * OVMR_E_ARG for EPI_PATCH / EPI_SCALE_ARGMAX; otherwise the launcher's rc. */
int ovmr_debug_gemm_strided(int variant, const void* A, int lda, const void* W, int ldw, const void* bias, const void* res,
                            int ldres, void* C, int ldc, int M, int N, int K, int epi, float scale, const float* gamma,
                            const float* beta, int row_step, ovmr_stream stream);
/* fp32 attention (hd = 64) over nseq sequences packed row after row: sequence b is the rows [offsets[b] + b * n_ctx,
 * offsets[b + 1] + (b + 1) * n_ctx) of qkv [M, 3 * H * 64], offsets_dev a DEVICE int32 [nseq + 1] exclusive prefix sum, every length
 * in [1, max_len]; out [M, H * 64].  The table mode of attn_f32_small, the kernel ovmr_debug_attention(f32 = 1) runs in its uniform
 * mode: row by row the same arithmetic.  -2 for max_len > 128. */
int ovmr_debug_attention_f32_varlen(const void* qkv, void* out, const int32_t* offsets_dev, int nseq, int n_ctx, int max_len, int H,
                                    ovmr_stream stream);

/* attn_f32_long, the kernel the generator runs for a chunk whose longest class has more than 128 rows, launched directly at ANY max_len
 * (short launches included): 128-row query tiles, the keys walked in order in 64-key LDS blocks.  offsets_dev as above, or NULL for the
 * uniform mode: nseq sequences of max_len rows each, n_ctx unused.  Per sequence bit-equal to attn_f32_small up to 128 rows and to
 * this launch on the sequence alone beyond; max_len only sizes the grid.  -2 for max_len > OVMR_AGG_MAX_LEN_CEILING, before any launch. */
int ovmr_debug_attention_f32_long(const void* qkv, void* out, const int32_t* offsets_dev, int nseq, int n_ctx, int max_len, int H,
                                  ovmr_stream stream);
/* fp16 attention for the first Lq <= L queries of every sequence (the last vision block runs Lq = 1, the CLS query):
 * out [B*Lq, H*64], row b*Lq + q.  Lq > L returns OVMR_E_SHAPE. */
int ovmr_debug_attention_q(int variant, const void* qkv, void* out, int B, int L, int Lq, int H, int causal,
                           ovmr_stream stream);
/* The kernel an fp16 attention launch under option "attn" = variant runs (no launch, no GPU): 0 plain flash-style, 1 flash-style
 * LDS-DMA, 2 short sequences, 3 single-pass, 5 32x32x16 flash. */
int ovmr_debug_attention_route(int variant, int L, int Lq, int causal);
/* The plan of an fp16 GEMM launch under option "gemm" = variant (no launch, no GPU), for 16-byte-aligned operands with lda = ldw = K
 * and every operand present that a feature of the 256-row kernel needs; stats: with the row statistics output; im2col: the image
 * side R of a patch-gathering launch (rows_in = (R / 16)^2), 0 = A is a matrix.  out[10]:
 *   [0] kernel: 0 none (the launch returns [1]), 1 the 128 x 128 kernel, 2 64 x 64 split-K, 3 256-row family tile kernel;
 *   [1] return code of a launch that runs no kernel (0: empty shape);
 *   [2] split-K: K-steps of 32 prefetched per wave, [3] groups of that many steps per wave;
 *   tile kernel: [4] tile rows (128 / 256), [5] K loop (0 double-buffered, 1 iteration boundary inside the MFMA stream, 2 ping-pong),
 *   [6] nontemporal A stream, [7] nontemporal C stores, [8] N tiles per group of the tile order (4, or all of them);
 *   [9] QuickGELU in the one-rounding form (epilogues 2 and 7).
 * The plan is that of option "gemm_persist" = 0; no field above depends on that option. */
int ovmr_debug_gemm_route(int variant, int M, int N, int K, int epi, int ldc, int ldres, int stats, int im2col, int* out);
/* The instantiations of the tile kernel the library holds, (epilogue, tile rows / 32, option bits) each: returns their number and
 * writes the first `cap` of them to out[3 * cap].  The route reaches every one of them and no other (tests/test_gemm_route_cpu.py). */
int ovmr_debug_gemm_tile_kernels(int* out, int cap);
/* Fills the whole workspace arena of a finalized handle with the 32-bit pattern on the stream (hipMemsetD32Async): it allocates
 * nothing and does not synchronise.  OVMR_E_ARG for a NULL handle, OVMR_E_STATE before ovmr_finalize.  It never touches the fused
 * head's device counters: those must stay zero between launches, and a poisoned counter makes the head's wait spin forever.
 * For tests/test_hip_poison.py: the result of a pass is a function of its inputs and weights, not of what the arena held. */
int ovmr_debug_fill_workspace(ovmr_handle* h, uint32_t pattern, ovmr_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* OVMR_HIP_H */
