// Launchers, one per .hip translation unit: host prototypes only.  common.h includes this file as its last line, so every unit sees them;
// they live here because common.h holds what kernels are compiled from (its hash stamps the counter summaries, build.source_sha16).
#pragma once

int launch_gemm_f16(const GemmArgs& a, int variant, hipStream_t s);   // gemm_route.h: which kernel it runs
int launch_gemm_f32(const GemmArgs& a, hipStream_t s);
int launch_layernorm(const void* x, void* y, const float* g, const float* b, int rows, int D,
                     long in_row_stride, int is_f32, hipStream_t s);
int launch_row_stats(const half_t* x, float* stats, int rows, int D, int slots, hipStream_t s);
int launch_fold_ln(const half_t* W, const float* gamma, const float* beta, const half_t* bias, half_t* Wf, float* g, float* b,
                   int N, int K, hipStream_t s);
int launch_attention_f16(const half_t* qkv, half_t* out, int B, int L, int H, int causal, int variant, hipStream_t s);
int launch_attention_f16_q(const half_t* qkv, half_t* out, int B, int L, int Lq, int H, int causal, int variant, hipStream_t s);
// up to 4 groups of sequences of at most 32 tokens in one launch (attention_short.hip); -100: not taken
int launch_attention_f16_short(const half_t* qkv, half_t* out, int n_groups, const int* nseq, const int* L, const long* row0, int H,
                               int causal, hipStream_t s);
// attention.hip: attn_f32_small for q.len <= 128, attn_f32_long up to max_len (route_f32 there), -2 above it before any launch
int launch_attention_f32(const float* qkv, float* out, const AggSeqs& q, int H, int max_len, hipStream_t s);
int launch_attention_f32_long(const float* qkv, float* out, const AggSeqs& q, int H, hipStream_t s);   // attn_f32_long at any q.len
int launch_im2col(const void* img, int img_is_f32, half_t* out, int B, int R, int P, int Kpad, hipStream_t s);
int launch_fill_cls(half_t* x, const half_t* cls_pos, int B, int L, int W, hipStream_t s);
int launch_l2norm_f16(half_t* x, int rows, int D, hipStream_t s);
int launch_cast(const void* src, int src_f32, void* dst, int dst_f32, long n, hipStream_t s);
int launch_transpose_to_f16(const void* src, int src_f32, half_t* dst, int rows, int cols, hipStream_t s);
int launch_pad_rows_f16(const half_t* src, half_t* dst, int rows, int cols, int cols_pad, hipStream_t s);
int launch_add_f16(const half_t* a, const half_t* b, half_t* out, long n, hipStream_t s);
int launch_text_embed_ids(const int64_t* ids, int ids_stride, const float* tok_emb, const half_t* pos16,
                          half_t* x, int* index, int N, int Lctx, int Lseq, int D, hipStream_t s);
int launch_embed_gather(const int64_t* ids, const float* tok_emb, half_t* out, long rows, int D, hipStream_t s);
int launch_text_add_pos(const half_t* prompts, int Lctx, const half_t* pos16, half_t* x, int N, int Lseq, int D, hipStream_t s);
int launch_gather_rows_f16(const half_t* x, const int* index, half_t* out, int N, int Lseq, int D, hipStream_t s);
int launch_pack_rows(const half_t* mm, const half_t* v, const half_t* t, const half_t* tokens, const int64_t* labels, int n, int D, int n_ctx,
                     int bound, half_t* block, hipStream_t s);
int launch_unpack_rows(const half_t* gathered, int rows, int C, int D, int n_ctx, half_t* mm, half_t* v, half_t* t, half_t* tokens, int* seen,
                       hipStream_t s);
// feats [R, D]: the exemplar rows of the whole call (q.first_shot indexes it)
int launch_agg_input(const float* cls_token, const half_t* feats, int R, float* x, const AggSeqs& q, int D, hipStream_t s);
int launch_agg_output(const float* x, float* tokens, const AggSeqs& q, int D, hipStream_t s);
int launch_assemble_prompts(const half_t* base, const int64_t* labels, const float* tokens, half_t* out,
                            int Cb, int Lctx, int n_ctx, int D, hipStream_t s);
int launch_argmax_counts(const half_t* logits, int ld, const int* labels, int R, int C, int* tp, int* n_pred, hipStream_t s);
int launch_argmax_reduce(const float* partial, int tiles, const int* labels, int R, int C, int* tp, int* n_pred, hipStream_t s);
int launch_fusion_weights(const int* counts, const int* n_label, int C, float tau, float* out, hipStream_t s);
int launch_eval_counts(const void* out, int out_is_f32, long ld, const int64_t* labels, int B, int C, int* counts, hipStream_t s);
int launch_scale_f16(const half_t* x, half_t* y, float scale, long n, hipStream_t s);
struct ovmr_resize_job;
int launch_resize_crop_u8(const uint8_t* pixels, const ovmr_resize_job* jobs, int n, const int32_t* tables, uint8_t* tmp, int max_ny,
                          uint8_t* out, int R, hipStream_t s);
int launch_preprocess_u8(const uint8_t* in, half_t* out, int B, int R, const float* mean3, const float* std3, hipStream_t s);
// one-launch classifier head (head_fused.hip); -100: shape not taken
size_t head_fused_ws_bytes(int B, int C);
int head_fused_sync_ints();
// plane_stride > 0: the all-modes form -- `out` is four planes [B, C], plane_stride floats apart (fusion, text, vision, multimodal)
int launch_head_fused(const half_t* feats, int B, int D, float scale, const half_t* const* clf, int n_mod, int C, const float* w,
                      float* out, long plane_stride, half_t* raw_out, void* ws, int* sync, int n_cu, int max_grid, hipStream_t s);
// the softmax of the GEMM path (fusion_head.hip); plane_stride > 0: the same four planes (three logit buffers and w required)
int launch_fused_softmax(const half_t* l0, const half_t* l1, const half_t* l2, const float* w, int n_mod,
                         float* out, long plane_stride, int B, int C, hipStream_t s);
int launch_text_ensemble(const half_t* feats, int T, int rows, int E, half_t* out, hipStream_t s);
int launch_topk_rows(const void* out, int out_is_f32, long ld, int B, int C, int k, float* values, int32_t* indices, const int64_t* labels,
                     int* hits, hipStream_t s);
// neighbours.hip: the one-wave-per-query launch of ovmr_neighbours_rows (max_range in [1, 4096]; operands already checked by the caller)
int launch_neighbours_short(const void* Q, int B, const void* X, long R, int D, int k, const int32_t* ranges, const int32_t* exclude,
                            int max_range, float* values, int32_t* indices, hipStream_t stream);
int launch_eval_detail(const void* out, int out_is_f32, long ld, const int64_t* labels, int B, int C, int k, int* counts, int* hits,
                       int* class_hits, int* cmat, hipStream_t s);
