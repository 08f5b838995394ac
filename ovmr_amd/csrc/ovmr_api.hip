// C ABI of libovmr_hip.so (see include/ovmr_hip.h): weight arena, workspace and the launch
// sequences of the OVMR hot path.  No call in the compute entry points allocates, copies to the
// host or synchronises, so every one of them can be captured into a hipGraph by the caller.
#include "../../include/ovmr_hip.h"
#include "carver.h"
#include "gemm_route.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

struct Buf {
    void* p = nullptr;
    size_t elems = 0;
    int f32 = 0;
    std::vector<int64_t> shape;
};

struct Block {   // one residual attention block; element type depends on the tower
    void *in_w, *in_b, *out_w, *out_b, *fc_w, *fc_b, *pj_w, *pj_b;
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    // LayerNorm folded into in_proj / c_fc (common.h EPI_LN_BIAS): h(gamma (.) W), column sums, folded bias; built by finalize
    half_t *in_wf = nullptr, *fc_wf = nullptr;
    float *in_g = nullptr, *in_bf = nullptr, *fc_g = nullptr, *fc_bf = nullptr;
};

}  // namespace

struct ovmr_handle {
    ovmr_model_desc d;
    std::map<std::string, Buf> w;
    std::vector<void*> owned;     // weight arena (lives until ovmr_destroy)
    std::vector<void*> derived;   // layouts rebuilt by every ovmr_finalize
    std::string err;
    bool finalized = false;
    int gelu_exact = 0;           // 0 (default): one-rounding fp32 QuickGELU in the c_fc epilogue (common.h quick_gelu_f32x2) -- DEVIATES from the
                                  // reference's fp16 rounding points by up to 8e-3 * max(1, |g|) per value, 6e-7 in 1 - cos end to end (INTEGRATION.md,
                                  // DESIGN.md section 3); 1: the reference's three fp16 rounding points
    int last_q_cls = 1;           // last vision block: Q projected for the CLS rows only (launch sequences of >= 256 images)
    int fuse_im2col = 1;          // patch rows gathered by the patch-embedding GEMM itself (fp16 images, 16 x 16 patches)
    int gemm_variant = 8, attn_variant = 3;   // defaults = fastest verified kernels (tools/gemm_bench.py, tools/attn_bench.py); attention 3 falls back to 1 / 0 by shape
    int ln_fold = 1;                          // fold ln_1 / ln_2 of the fp16 towers into the consuming GEMM where the shape allows
    int gemm_persist = 1;                     // in_proj / c_fc as a tile loop of one workgroup per CU (gemm_f16_v5.hip "Tile loop"; DESIGN.md section 4 for the default)
    int xval_fused = 1;                       // cross-validation logits: row argmax fused into the GEMM epilogue (never stored)
    int fused_head = 1;                       // ovmr_fused_logits / ovmr_zeroshot_logits as ONE launch (head_fused.hip); 0: scale + GEMMs + softmax
    int head_max_grid = 0;                    // > 0 caps the fused head's grid (tests: workgroups then take several tiles)
    int* head_sync = nullptr;                 // the fused head's device counters (zero between launches)
    float logit_scale_exp = 100.f;
    bool have_logit_scale = false;

    std::vector<Block> vis, txt, agg;
    half_t *conv_w = nullptr, *pos16_vis = nullptr, *cls_pos16 = nullptr, *proj_t = nullptr;
    half_t *pos16_txt = nullptr, *textproj_t = nullptr;
    void *conv1 = nullptr, *cls_emb = nullptr, *pos_vis = nullptr, *proj = nullptr, *pos_txt = nullptr, *textproj = nullptr;   // as set: the sources of those
    float *ln_pre_g = nullptr, *ln_pre_b = nullptr, *ln_post_g = nullptr, *ln_post_b = nullptr;
    float *ln_final_g = nullptr, *ln_final_b = nullptr, *tok_emb = nullptr, *cls_token = nullptr;
    int Kpad = 0, G = 0, L = 0;

    char* ws = nullptr;
    size_t ws_bytes = 0;
    int max_images = 0, max_prompts = 0, max_classes = 0;
    int enc_chunk_forced = 0;     // option "enc_chunk": > 0 pins the chunk, 0 = pick_encode_chunk
    int n_cu = 0;
    int enc_chunk = 0;            // images per launch sequence of ovmr_encode_image (<= max_images; pick_encode_chunk); option "enc_chunk" overrides
    int enc_fold = 0;             // a remainder of at most this many images (one round of the narrowest GEMM grid) joins the last full sequence
    int img_cap = 0;              // images the workspace holds: max_images + enc_fold
    long agg_rows_cap = 0, logit_elems_cap = 0;
    int agg_max_len = 128;             // option "agg_max_len": the most rows (n_ctx + shots) of one class
};

namespace {

int fail(ovmr_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

#define CK(expr)                                                                         \
    do {                                                                                 \
        int _rc = (expr);                                                                \
        if (_rc != 0) return fail(h, _rc, "%s failed with %d (%s:%d)", #expr, _rc, __FILE__, __LINE__); \
    } while (0)

bool ends_with(const std::string& s, const char* suf) {
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// Device allocation registered in `list`: h->owned (until ovmr_destroy) or h->derived (until the next ovmr_finalize)
void* dev_alloc(std::vector<void*>& list, size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
    list.push_back(p);
    return p;
}

int need_finalized(ovmr_handle* h) {
    return h->finalized ? 0 : fail(h, OVMR_E_STATE, "ovmr_finalize() has not been called");
}

// The weights, each stated ONCE: name (block weights: the suffix behind "<prefix><layer>."), elements, stored dtype and where ovmr_finalize
// binds it.  ovmr_set_weight reads the tables for "is this name known" and the dtype, ovmr_finalize for presence, size and binding, in
// table order.  dtype policy of convert_weights() (clip/model.py:852-873): LayerNorm parameters and embeddings stay fp32.
struct Weight { const char* name; size_t elems; bool f32; void** dst; };

std::array<Weight, 12> block_weights(size_t w, Block& k) {
    return {{{"attn.in_proj_weight", 3 * w * w, false, &k.in_w}, {"attn.in_proj_bias", 3 * w, false, &k.in_b},
             {"attn.out_proj.weight", w * w, false, &k.out_w},   {"attn.out_proj.bias", w, false, &k.out_b},
             {"mlp.c_fc.weight", 4 * w * w, false, &k.fc_w},     {"mlp.c_fc.bias", 4 * w, false, &k.fc_b},
             {"mlp.c_proj.weight", 4 * w * w, false, &k.pj_w},   {"mlp.c_proj.bias", w, false, &k.pj_b},
             {"ln_1.weight", w, true, (void**)&k.ln1_g},         {"ln_1.bias", w, true, (void**)&k.ln1_b},
             {"ln_2.weight", w, true, (void**)&k.ln2_g},         {"ln_2.bias", w, true, (void**)&k.ln2_b}}};
}

struct Tower { const char* prefix; int layers, width; std::vector<Block>* blocks; bool f32; };
std::array<Tower, 3> towers(ovmr_handle* h) {
    const ovmr_model_desc& d = h->d;
    return {{{"visual.transformer.resblocks.", d.vision_layers, d.vision_width, &h->vis, false},
             {"transformer.resblocks.", d.transformer_layers, d.transformer_width, &h->txt, false},
             {"prompt_learner.aggregator.resblocks.", d.agg_layers, d.embed_dim, &h->agg, true}}};   // the aggregator is never halved
}

std::array<Weight, 14> single_weights(ovmr_handle* h) {   // (logit_scale is none of them: read to the host, never stored)
    const ovmr_model_desc& d = h->d;
    const size_t W = d.vision_width, T = d.transformer_width, E = d.embed_dim, P = d.vision_patch_size;
    return {{{"visual.conv1.weight", W * 3 * P * P, false, &h->conv1},
             {"visual.class_embedding", W, true, &h->cls_emb},
             {"visual.positional_embedding", (size_t)h->L * W, true, &h->pos_vis},
             {"visual.proj", W * E, false, &h->proj},
             {"positional_embedding", (size_t)d.context_length * T, true, &h->pos_txt},
             {"text_projection", T * E, false, &h->textproj},
             {"visual.ln_pre.weight", W, true, (void**)&h->ln_pre_g},   {"visual.ln_pre.bias", W, true, (void**)&h->ln_pre_b},
             {"visual.ln_post.weight", W, true, (void**)&h->ln_post_g}, {"visual.ln_post.bias", W, true, (void**)&h->ln_post_b},
             {"ln_final.weight", T, true, (void**)&h->ln_final_g},      {"ln_final.bias", T, true, (void**)&h->ln_final_b},
             {"token_embedding.weight", (size_t)d.vocab_size * T, true, (void**)&h->tok_emb},
             {"prompt_learner.cls_token", (size_t)d.n_ctx * E, true, (void**)&h->cls_token}}};
}

int bind_weight(ovmr_handle* h, const std::string& name, const Weight& wt) {
    auto it = h->w.find(name);
    if (it == h->w.end()) return fail(h, OVMR_E_STATE, "weight '%s' was never set", name.c_str());
    if (it->second.elems != wt.elems)
        return fail(h, OVMR_E_STATE, "weight '%s' has %zu elements, expected %zu", name.c_str(), it->second.elems, wt.elems);
    *wt.dst = it->second.p;
    return 0;
}

GemmArgs gemm(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, int epi,
              const void* bias = nullptr, const void* res = nullptr, int ldres = 0) {
    GemmArgs a;
    memset(&a, 0, sizeof a);
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc;
    a.M = M; a.N = N; a.K = K; a.epi = epi; a.bias = bias; a.res = res; a.ldres = ldres; a.scale = 1.f;
    return a;
}

// One pass of an fp16 tower over M token rows of N sequences.  Image tower (image_ws): the patch rows `col` come first and `rows` are
// the CLS rows; text tower (text_ws): `rows` are the read-out rows and `index` their positions.  A buffer of 0 elements takes no room.
struct TowerWs : Carver {
    half_t *col, *x, *y, *qkv, *hid, *rows;
    int* index;
    float* stats;
    TowerWs(char* base, size_t W, size_t M, size_t N, size_t col_elems, size_t n_index) : Carver(base) {
        col = take<half_t>(col_elems);
        x = take<half_t>(M * W);
        y = take<half_t>(M * W);
        qkv = take<half_t>(M * 3 * W);
        hid = take<half_t>(M * 4 * W);                     // mlp hidden
        rows = take<half_t>(N * W);
        index = take<int>(n_index);
        stats = take<float>(M * ((W + 255) / 256) * 2);    // LayerNorm partial statistics
    }
};
TowerWs image_ws(const ovmr_handle* h, char* base, size_t B) { return TowerWs(base, h->d.vision_width, B * h->L, B, B * h->G * h->G * h->Kpad, 0); }
TowerWs text_ws(const ovmr_handle* h, char* base, size_t M, size_t N) { return TowerWs(base, h->d.transformer_width, M, N, 0, N); }

struct EnsembleWs : TowerWs {   // ovmr_encode_text_ensemble: a text pass, then the [T, c, E] raw rows of its N = T * c prompts behind it
    half_t* raw;
    EnsembleWs(const ovmr_handle* h, char* base, size_t M, size_t N) : TowerWs(text_ws(h, base, M, N)) { raw = take<half_t>(N * h->d.embed_dim); }
};

struct AggWs : Carver {         // the fp32 aggregator over `rows` token rows
    float *x, *y, *qkv, *hid;
    AggWs(const ovmr_handle* h, char* base, size_t rows) : Carver(base) {
        const size_t D = h->d.embed_dim;
        x = take<float>(rows * D);
        y = take<float>(rows * D);
        qkv = take<float>(rows * 3 * D);
        hid = take<float>(rows * 4 * D);
    }
};

// The classifier head's GEMM path: `n_logits` buffers of logit_elems_cap fp16 logits, then 65536 rows of scaled features.
// A probability call takes one per classifier (ovmr_finalize sizes for three), ovmr_xval_counts one, a raw call (zero-shot) none.
struct HeadWs : Carver {
    half_t *l[3] = {nullptr, nullptr, nullptr}, *sf;
    HeadWs(const ovmr_handle* h, char* base, int n_logits) : Carver(base) {
        for (int m = 0; m < n_logits; ++m) l[m] = take<half_t>((size_t)h->logit_elems_cap);
        sf = take<half_t>((size_t)65536 * h->d.embed_dim);
    }
};

// LayerNorm folding applies when the v5 GEMM takes the shape (it then also emits the statistics): see common.h.
// Not for latency-bound passes (the N = W launches -- out_proj, c_proj -- then take the 64 x 64 split-K kernel under the default
// variant, which emits no statistics; the separate LayerNorm kernel costs ~4 us there).
bool can_fold_ln(const ovmr_handle* h, const Block& k, int M, int W) {
    return h->ln_fold && k.in_wf && M >= 256 && (W % 256) == 0 && W / 256 <= 64 && !gemm_f16_latency_bound(h->gemm_variant, M, W);
}

GemmArgs gemm_ln(GemmArgs a, const float* stats, int slots, const float* g, const float* b) {
    a.ln_stats = stats; a.ln_slots = slots; a.ln_g = g; a.ln_b = b;
    return a;
}
GemmArgs gemm_stats(GemmArgs a, float* stats) {
    a.stats_out = stats;
    return a;
}
// The patch-embedding GEMM that gathers its rows from the fp16 images [B, 3, R, R] itself (gemm_f16_v5.hip, a.im2col_R): 16 x 16
// patches, K = 768, G * G = (R / 16)^2 patch rows per image written behind the image's CLS row.  x [B * (G * G + 1), W].
GemmArgs gemm_patches(const void* image, int R, const void* conv_w, const void* pos, void* x, int B, int W) {
    const int G2 = (R >> 4) * (R >> 4);
    GemmArgs a = gemm(image, 768, conv_w, 768, x, W, B * G2, W, 768, EPI_PATCH);
    a.im2col_R = R; a.pos = pos; a.rows_in = G2; a.rows_out = G2 + 1;
    return a;
}

// Scratch of the two LayerNorm-fold hooks, allocated per call: the statistics of `rows` rows and the folded form of a raw [N, K]
// weight (rc: allocation or fold failure).  Leaving the hook waits for the stream and frees it.
struct LnFoldScratch {
    float *stats = nullptr, *g = nullptr, *bf = nullptr;
    half_t* wf = nullptr;
    hipStream_t s;
    int rc = 0;
    LnFoldScratch(size_t rows, const void* W, const float* gamma, const float* beta, const void* bias, int N, int K, hipStream_t s_) : s(s_) {
        if (hipMalloc((void**)&stats, rows * (K / 256) * 8) != hipSuccess || hipMalloc((void**)&g, (size_t)N * 4) != hipSuccess ||
            hipMalloc((void**)&bf, (size_t)N * 4) != hipSuccess || hipMalloc((void**)&wf, (size_t)N * K * 2) != hipSuccess)
            rc = OVMR_E_NOMEM;
        if (!rc) rc = launch_fold_ln((const half_t*)W, gamma, beta, (const half_t*)bias, wf, g, bf, N, K, s);
    }
    ~LnFoldScratch() {
        (void)hipStreamSynchronize(s);
        (void)hipFree(stats); (void)hipFree(g); (void)hipFree(bf); (void)hipFree(wf);
    }
};

// A LayerNorm-fed linear layer of a block: in_proj behind ln_1, or c_fc (QuickGELU epilogue) behind ln_2; wf / g / bf = its folded form
struct LnLinear { const float *ln_g, *ln_b; const half_t *w, *b, *wf; const float *g, *bf; bool gelu; };
LnLinear in_proj(const Block& k) { return {k.ln1_g, k.ln1_b, (const half_t*)k.in_w, (const half_t*)k.in_b, k.in_wf, k.in_g, k.in_bf, false}; }
LnLinear c_fc(const Block& k) { return {k.ln2_g, k.ln2_b, (const half_t*)k.fc_w, (const half_t*)k.fc_b, k.fc_wf, k.fc_g, k.fc_bf, true}; }

// One GEMM of such a layer: weight rows [r0, r0 + n) applied to M input rows, every `step`-th row of the buffer, into C (row stride ldc)
struct LnPart { int r0, n, M, step; half_t* C; int ldc; };

// LayerNorm of the `rows` rows of x, then the GEMMs `parts`.  stats != nullptr (the partial row statistics of x): the LayerNorm is folded
// into the GEMMs (folded weights, EPI_LN_BIAS[_QGELU]); nullptr: launch_layernorm x -> y once, plain GEMMs on y.
int ln_linear(ovmr_handle* h, const LnLinear& l, const half_t* x, half_t* y, int rows, int W, const float* stats, int variant,
              std::initializer_list<LnPart> parts, hipStream_t s) {
    if (!stats) CK(launch_layernorm(x, y, l.ln_g, l.ln_b, rows, W, W, 0, s));
    const int slots = W / 256, epi = l.gelu ? (stats ? EPI_LN_BIAS_QGELU : EPI_BIAS_QGELU) : (stats ? EPI_LN_BIAS : EPI_BIAS);
    for (const LnPart& p : parts) {
        GemmArgs a = gemm(stats ? x : y, p.step * W, (stats ? l.wf : l.w) + (size_t)p.r0 * W, W, p.C, p.ldc, p.M, p.n, W, epi, stats ? nullptr : l.b + p.r0);
        if (stats) { a = gemm_ln(a, stats, slots, l.g + p.r0, l.bf + p.r0); a.ln_stride = p.step * slots; }
        a.gelu_mode = l.gelu && !h->gelu_exact;              // the one-rounding QuickGELU (common.h quick_gelu_f32x2)
        a.persist = h->gemm_persist;                         // the tile loop, where gemm_f16_route plans it
        CK(launch_gemm_f16(a, variant, s));
    }
    return 0;
}

// One pre-LN residual attention block (clip/model.py:191-194) on fp16 activations.
// stats != nullptr: ln_1 / ln_2 are folded into in_proj / c_fc.  On entry `stats` holds the partial row statistics of x
// (launch_row_stats, or the previous block's c_proj epilogue); on exit those of the new x.
// `groups` (text tower, ovmr_encode_text_groups): the token rows are several groups of sequences with their own length each --
// the GEMMs run over all rows at once, attention once per group; nullptr: nseq sequences of L tokens.
// `cls_rows` (last vision block): only the CLS row reaches ln_post (clip/model.py:423), so after the K/V projection of all tokens,
// attention / out_proj / MLP run for the CLS query row only and the new CLS rows land in cls_rows [nseq, W] -- identical result,
// ~6 % fewer FLOPs; x keeps the block's input.
struct SeqGroup { int nseq, L; long row0; };

int run_block_f16(ovmr_handle* h, const Block& k, half_t* x, half_t* y, half_t* qkv, half_t* hid,
                  int nseq, int L, int W, int causal, hipStream_t s, float* stats = nullptr,
                  const std::vector<SeqGroup>* groups = nullptr, half_t* cls_rows = nullptr) {
    int M = nseq * L;
    if (groups) { M = 0; for (auto& g : *groups) M += g.nseq * g.L; }
    const int H = W / 64;
    if (cls_rows && nseq >= 256 && h->last_q_cls) {
        // ... and of the in-projection itself only K and V are needed for every token: with at least 256 images (a full row tile of
        // CLS rows) the Q third runs as its own launch over the CLS rows (A and C strided by a sequence; bit-identical values),
        // a third of this block's largest GEMM less.  Both launches take the kernel the all-token launch of last_q_cls = 0 would
        // take (gemm_f16_pinned_variant: the split-K kernel if [M, 3W] is a latency-bound shape, else the tile kernels) so that the K summation
        // order, and with it every bit, is the same either way (folded launches run the 256-row kernel under either number).
        CK(ln_linear(h, in_proj(k), x, y, M, W, stats, gemm_f16_pinned_variant(h->gemm_variant, M, 3 * W),
                     {{W, 2 * W, M, 1, qkv + W, 3 * W}, {0, W, nseq, L, qkv, L * 3 * W}}, s));
    } else
        CK(ln_linear(h, in_proj(k), x, y, M, W, stats, h->gemm_variant, {{0, 3 * W, M, 1, qkv, 3 * W}}, s));
    if (cls_rows)
        CK(launch_attention_f16_q(qkv, y, nseq, L, 1, H, causal, h->attn_variant, s));
    else if (groups) {
        // short groups (every prompt family of a classifier head: <= ~20 tokens) share ONE launch; longer ones run group by group
        int rc = -100;
        if (h->attn_variant >= 1 && groups->size() <= 4) {
            int ns[4], Ls[4];
            long r0[4];
            for (size_t i = 0; i < groups->size(); ++i) { ns[i] = (*groups)[i].nseq; Ls[i] = (*groups)[i].L; r0[i] = (*groups)[i].row0; }
            rc = launch_attention_f16_short(qkv, y, (int)groups->size(), ns, Ls, r0, H, causal, s);
            if (rc != -100) CK(rc);
        }
        if (rc == -100)
            for (auto& g : *groups)
                CK(launch_attention_f16(qkv + g.row0 * 3 * W, y + g.row0 * W, g.nseq, g.L, H, causal, h->attn_variant, s));
    } else
        CK(launch_attention_f16(qkv, y, nseq, L, H, causal, h->attn_variant, s));
    // the rest of the block on xo: x itself, or (cls_rows) the CLS rows alone, their residual read from the token rows and no statistics kept
    half_t* xo = cls_rows ? cls_rows : x;
    const int Mo = cls_rows ? nseq : M;
    float* so = cls_rows ? nullptr : stats;
    CK(launch_gemm_f16(gemm_stats(gemm(y, W, k.out_w, W, xo, W, Mo, W, W, EPI_BIAS_RES, k.out_b, x, cls_rows ? L * W : W), so), h->gemm_variant, s));
    CK(ln_linear(h, c_fc(k), xo, y, Mo, W, so, h->gemm_variant, {{0, 4 * W, Mo, 1, hid, 4 * W}}, s));
    CK(launch_gemm_f16(gemm_stats(gemm(hid, 4 * W, k.pj_w, 4 * W, xo, W, Mo, W, 4 * W, EPI_BIAS_RES, k.pj_b, xo, W), so), h->gemm_variant, s));
    return 0;
}

// Same block in fp32 (ResidualAttentionBlockWithDropout in eval mode, clip/model.py:248-251) over the q.M packed rows of an aggregator
// pass: only the attention launch reads the sequences, every other step is per row.
int run_block_f32(ovmr_handle* h, const Block& k, float* x, float* y, float* qkv, float* hid, const AggSeqs& q, int W, hipStream_t s) {
    const int M = q.M, H = W / 64;
    CK(launch_layernorm(x, y, k.ln1_g, k.ln1_b, M, W, W, 1, s));
    CK(launch_gemm_f32(gemm(y, W, k.in_w, W, qkv, 3 * W, M, 3 * W, W, EPI_BIAS, k.in_b), s));
    CK(launch_attention_f32(qkv, y, q, H, h->agg_max_len, s));
    CK(launch_gemm_f32(gemm(y, W, k.out_w, W, x, W, M, W, W, EPI_BIAS_RES, k.out_b, x, W), s));
    CK(launch_layernorm(x, y, k.ln2_g, k.ln2_b, M, W, W, 1, s));
    CK(launch_gemm_f32(gemm(y, W, k.fc_w, W, hid, 4 * W, M, 4 * W, W, EPI_BIAS_QGELU, k.fc_b), s));
    CK(launch_gemm_f32(gemm(hid, 4 * W, k.pj_w, 4 * W, x, W, M, W, 4 * W, EPI_BIAS_RES, k.pj_b, x, W), s));
    return 0;
}

// The visual tokens of Cb classes, after the entry points' checks: class c has shots_host[c] exemplars (every class S where shots_host
// is null: the uniform call, which has no device table either) and its rows of feats [R, D] start at the prefix sum of the shots.
// Chunks are runs of whole classes whose packed rows fit agg_rows_cap, at least one class each -- on equal counts floor(agg_rows_cap / La)
// classes, the uniform call's chunks; planned from the host's counts, indexed on the device through the table.
int generate_tokens(ovmr_handle* h, const half_t* feats, const int32_t* shots_host, int S, const int32_t* offsets_dev, int Cb, int R,
                    float* tokens_f32, hipStream_t s) {
    const ovmr_model_desc& d = h->d;
    const int D = d.embed_dim;
    auto len = [&](int c) { return d.n_ctx + (int)(shots_host ? shots_host[c] : S); };
    // two walks over the same plan: the first only checks that every chunk fits (a class longer than finalize sized the workspace
    // for -- option "agg_max_len" raised afterwards -- is refused before anything of the call has launched), the second launches
    for (int launch = 0; launch < 2; ++launch)
        for (int c0 = 0, off0 = 0; c0 < Cb;) {
            int c1 = c0, max_len = 0;
            long rows = 0;
            while (c1 < Cb && (c1 == c0 || rows + len(c1) <= h->agg_rows_cap)) {
                rows += len(c1);
                max_len = std::max(max_len, len(c1));
                ++c1;
            }
            const AggWs ws(h, h->ws, (size_t)rows);
            if (ws.bytes() > h->ws_bytes)
                return fail(h, OVMR_E_SHAPE, "the %ld aggregator rows of class %d do not fit the workspace", rows, c0);
            const int Cc = c1 - c0;
            if (launch) {
                const AggSeqs q{offsets_dev ? offsets_dev + c0 : nullptr, off0, Cc, d.n_ctx, max_len, (int)rows};
                CK(launch_agg_input(h->cls_token, feats, R, ws.x, q, D, s));
                for (auto& k : h->agg) CK(run_block_f32(h, k, ws.x, ws.y, ws.qkv, ws.hid, q, D, s));
                CK(launch_agg_output(ws.x, tokens_f32 + (size_t)c0 * d.n_ctx * D, q, D, s));
            }
            c0 = c1;
            off0 += (int)(rows - (long)Cc * d.n_ctx);
        }
    return 0;
}

int normalize_rows(ovmr_handle* h, half_t* x, int rows, int D, int mode, hipStream_t s) {
    for (int i = 0; i < mode; ++i) CK(launch_l2norm_f16(x, rows, D, s));
    return 0;
}

// One group of prompts of a text-tower pass: N sequences truncated to Ls tokens, read-out row `index` per sequence.
struct TextGroup {
    const half_t* prompts = nullptr;   // [N, context_length, W] embedded prompts, or
    const int64_t* ids = nullptr;      // [N, context_length] token ids (read-out row = argmax, clip/model.py:831)
    const int* index = nullptr;        // embedded prompts: [N]
    int N = 0, Ls = 0, normalize = 0;
    half_t* out = nullptr;             // [N, embed_dim]
};

// Text tower (clip/model.py:824-831) over all groups in ONE pass: embedding per group, the blocks' GEMMs over all token rows,
// causal attention with each group's own length (truncation to the last needed row is exact under the causal mask; one launch for
// all groups of at most 32 tokens, attention_short.hip, else group by group),
// read-out row gather, ln_final and projection per group.  The caller has checked that the rows fit the workspace.
int run_text_groups(ovmr_handle* h, const std::vector<TextGroup>& gs, hipStream_t s) {
    const ovmr_model_desc& d = h->d;
    const int W = d.transformer_width, Lc = d.context_length, E = d.embed_dim;
    size_t M = 0, N = 0;
    std::vector<SeqGroup> seq;
    for (auto& g : gs) { seq.push_back({g.N, g.Ls, (long)M}); M += (size_t)g.N * g.Ls; N += g.N; }
    const TowerWs ws = text_ws(h, h->ws, M, N);
    size_t n0 = 0;
    for (size_t i = 0; i < gs.size(); ++i) {
        const TextGroup& g = gs[i];
        half_t* xg = ws.x + seq[i].row0 * W;
        if (g.ids) CK(launch_text_embed_ids(g.ids, Lc, h->tok_emb, h->pos16_txt, xg, ws.index + n0, g.N, Lc, g.Ls, W, s));
        else CK(launch_text_add_pos(g.prompts, Lc, h->pos16_txt, xg, g.N, g.Ls, W, s));
        n0 += g.N;
    }
    float* stats = !h->txt.empty() && can_fold_ln(h, h->txt[0], (int)M, W) ? ws.stats : nullptr;
    if (stats) CK(launch_row_stats(ws.x, stats, (int)M, W, W / 256, s));
    for (auto& k : h->txt) CK(run_block_f16(h, k, ws.x, ws.y, ws.qkv, ws.hid, 0, 0, W, 1, s, stats, &seq));
    n0 = 0;
    for (size_t i = 0; i < gs.size(); ++i) {
        const TextGroup& g = gs[i];
        CK(launch_gather_rows_f16(ws.x + seq[i].row0 * W, g.ids ? ws.index + n0 : g.index, ws.rows + n0 * W, g.N, g.Ls, W, s));
        n0 += g.N;
    }
    CK(launch_layernorm(ws.rows, ws.rows, h->ln_final_g, h->ln_final_b, (int)N, W, W, 0, s));
    n0 = 0;
    for (auto& g : gs) {
        CK(launch_gemm_f16(gemm(ws.rows + n0 * W, W, h->textproj_t, W, g.out, E, g.N, E, W, EPI_NONE), h->gemm_variant, s));
        CK(normalize_rows(h, g.out, g.N, E, g.normalize, s));
        n0 += g.N;
    }
    return 0;
}

// One group, any size: chunks of max_prompts sequences.
int run_text_group_chunked(ovmr_handle* h, const TextGroup& g, hipStream_t s) {
    const int Lc = h->d.context_length, W = h->d.transformer_width, E = h->d.embed_dim;
    for (int n0 = 0; n0 < g.N; n0 += h->max_prompts) {
        TextGroup c = g;
        c.N = std::min(h->max_prompts, g.N - n0);
        if (g.ids) c.ids = g.ids + (size_t)n0 * Lc;
        else { c.prompts = g.prompts + (size_t)n0 * Lc * W; c.index = g.index + n0; }
        c.out = g.out + (size_t)n0 * E;
        CK(run_text_groups(h, {c}, s));
    }
    return 0;
}

// ovmr_fused_logits: the one-launch head (head_fused.hip) or scale + GEMMs + softmax.  Up to 256 query rows at any class count, up to 512
// rows x 2048 classes: every 64-row tile re-reads the classifier matrices, so beyond that the GEMM path's 256-row tiles win
// (tools/head_bench.py); option fused_head = 2 takes the one-launch kernel at any size, 0 never.  The two sum K in different orders: a logit
// may land on the neighbouring fp16 value, so callers that promise bit-equal rows for differently batched calls ask ovmr_head_plan.
bool head_takes_one_launch(const ovmr_handle* h, int B, int C) {
    return h->fused_head && (B <= 256 || (B <= 512 && C <= 2048) || h->fused_head == 2) && head_fused_ws_bytes(B, C) <= h->ws_bytes;
}

// One call of the classifier head: the probabilities of n_mod classifiers [C, D] weighted by w [C, 3] (null: one classifier, weight 1)
// into fp32 `out` [B, C] (plane_stride > 0: the four planes of the all-modes form), or the fp16 logits of ONE classifier into raw_out.
struct HeadCall {
    const half_t* feats; int B;
    const half_t* clf[3]; int n_mod;
    const float* w;
    int C;
    float* out; long plane_stride;
    half_t* raw_out;
};

// The one-launch head (head_fused.hip) where the call takes it -- raw calls whenever fused_head is set, at any size (one pass, no workspace,
// no counters); the others under head_takes_one_launch -- and the launcher takes the shape; else scale + GEMMs + softmax over row chunks.
int run_head(ovmr_handle* h, const HeadCall& c, hipStream_t s) {
    const int D = h->d.embed_dim, C = c.C;
    const bool raw = c.raw_out != nullptr;
    if (raw ? h->fused_head != 0 : head_takes_one_launch(h, c.B, C)) {
        // one launch: scaled features staged once, the (up to) three products, both rounding points, softmax and weighted sum
        const int rc = launch_head_fused(c.feats, c.B, D, h->logit_scale_exp, c.clf, c.n_mod, C, c.w, c.out, c.plane_stride, c.raw_out,
                                         h->ws, h->head_sync, h->n_cu, h->head_max_grid, s);
        if (rc != -100) { CK(rc); return 0; }
    }
    const HeadWs ws(h, h->ws, raw ? 0 : c.n_mod);            // raw logits go straight to raw_out: no logits buffer bounds the chunk
    const int chunk = raw ? 65536 : (int)std::min<long>(std::max<long>(1, h->logit_elems_cap / C), 65536);
    for (int b0 = 0; b0 < c.B; b0 += chunk) {
        const int Bc = std::min(chunk, c.B - b0);
        // (logit_scale * image_features) is rounded to fp16 before the matmul (:358-360)
        CK(launch_scale_f16(c.feats + (size_t)b0 * D, ws.sf, h->logit_scale_exp, (long)Bc * D, s));
        for (int m = 0; m < c.n_mod; ++m)
            CK(launch_gemm_f16(gemm(ws.sf, D, c.clf[m], D, raw ? c.raw_out + (size_t)b0 * C : ws.l[m], C, Bc, C, D, EPI_NONE), h->gemm_variant, s));
        if (!raw) CK(launch_fused_softmax(ws.l[0], ws.l[1], ws.l[2], c.w, c.n_mod, c.out + (size_t)b0 * C, c.plane_stride, Bc, C, s));   // every plane advances by b0 * C
    }
    return 0;
}

int check_text_call(ovmr_handle* h, int seq_len, int normalize) {
    if (normalize < 0 || normalize > 2) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    if (seq_len < 1 || seq_len > h->d.context_length) return fail(h, OVMR_E_ARG, "seq_len %d outside [1,%d]", seq_len, h->d.context_length);
    return 0;
}

}  // namespace

extern "C" {

const char* ovmr_version(void) { return "ovmr_hip 0.1 (gfx950)"; }

int ovmr_create(const ovmr_model_desc* d, ovmr_handle** out) {
    if (!d || !out) return OVMR_E_ARG;
    if (d->vision_width % 64 || d->transformer_width % 64 || d->embed_dim % 64 || d->vision_patch_size <= 0 ||
        d->image_resolution % d->vision_patch_size || d->n_ctx < 1 || d->context_length < 4 + d->n_ctx)
        return OVMR_E_SHAPE;
    ovmr_handle* h = new ovmr_handle();
    h->d = *d;
    h->G = d->image_resolution / d->vision_patch_size;
    h->L = h->G * h->G + 1;
    h->Kpad = (3 * d->vision_patch_size * d->vision_patch_size + 63) / 64 * 64;
    const size_t sync_bytes = (size_t)head_fused_sync_ints() * sizeof(int);
    if (hipMalloc((void**)&h->head_sync, sync_bytes) != hipSuccess || hipMemset(h->head_sync, 0, sync_bytes) != hipSuccess) {
        delete h;
        return OVMR_E_NOMEM;
    }
    h->owned.push_back(h->head_sync);
    *out = h;
    return 0;
}

void ovmr_destroy(ovmr_handle* h) {
    if (!h) return;
    for (void* p : h->owned) (void)hipFree(p);
    for (void* p : h->derived) (void)hipFree(p);
    if (h->ws) (void)hipFree(h->ws);
    delete h;
}

const char* ovmr_last_error(const ovmr_handle* h) { return h ? h->err.c_str() : "null handle"; }

// Images per launch sequence of the image tower.  Every GEMM of a block runs 256-row tiles, one workgroup per CU at a time, so a launch
// costs WHOLE rounds of the CUs: with t = ceil(B * L / 256) row tiles the N = W launches (out_proj, K = W; c_proj, K = 4W) pay
// ceil(t * W/256 / CUs) rounds, in_proj ceil(3 t W/256 / CUs), c_fc ceil(4 t W/256 / CUs), a round's time being proportional to K.
// The chunk is the B <= max_images with the most images per unit of that cost (ViT-B/16, 256 CUs: 775 images = 597 tiles = 6.996 /
// 20.99 / 27.98 rounds where 768 pays 7 / 21 / 28 for 6.93 / 20.78 / 27.70; ViT-L/14@336px: 170 images = 384 tiles = 6.0 / 18.0 / 24.0)
// -- measured +1.5-2 % end to end.  Reserves of less than two rounds keep max_images.  No more than 600 row
// tiles per chunk: beyond that the A panels of a launch compete for the L2s (ViT-B/16: 998 and 1108 images per chunk ran 4-5 % slower
// than 775, c_fc at 0.384-0.388 of peak instead of 0.41; ViT-L/14@336px: 227 images = 512 tiles slower than 170 = 384).
static int pick_encode_chunk(int max_images, int L, int W, int n_cu) {
    const long nw = std::max(1, W / 256);
    auto tiles = [&](long b) { return (b * L + 255) / 256; };
    auto rounds = [&](long wg) { return (wg + n_cu - 1) / n_cu; };
    if (n_cu < 1 || tiles(max_images) * nw < 2L * n_cu) return max_images;
    auto cost = [&](long b) { const long t = tiles(b); return 5 * rounds(t * nw) + rounds(3 * t * nw) + rounds(4 * t * nw); };
    const int top = (int)std::min<long>(max_images, std::max<long>(1, 600L * 256 / L));
    int best = top;
    double best_rate = (double)top / (double)cost(top);
    for (int b = top - 1; b >= std::max(1, top * 3 / 4); --b) {
        const double r = (double)b / (double)cost(b);
        if (r > best_rate * 1.002) { best_rate = r; best = b; }      // (a smaller chunk has to buy more than launch overheads cost)
    }
    return best;
}

static void set_enc_chunk(ovmr_handle* h) {               // needs max_images and n_cu: ovmr_finalize, and the option once finalized
    h->enc_chunk = h->enc_chunk_forced > 0 ? std::min(h->enc_chunk_forced, h->max_images)
                                           : pick_encode_chunk(h->max_images, h->L, (int)h->d.vision_width, h->n_cu);
}

// Launch sequences of a batch of B images: one if it fits the reserve; else chunks of enc_chunk images, a remainder of at most
// enc_fold images (less than one round of tiles on the narrowest grid: as its own sequence it would pay a whole round on every launch
// PLUS ~70 launches of latency, 2.1 ms for 25 ViT-B/16 images where the extra round inside the previous sequence costs 1.8) folded
// into the last full chunk.
static std::vector<int> encode_plan(const ovmr_handle* h, int B) {
    std::vector<int> plan;
    const int chunk = h->enc_chunk_forced > 0 ? h->enc_chunk : (B > h->max_images && h->enc_chunk > 0 ? h->enc_chunk : h->max_images);
    for (int b0 = 0; b0 < B;) {
        int Bc = std::min(chunk, B - b0);
        const int left = B - b0 - Bc;
        if (left > 0 && left <= h->enc_fold && Bc + left <= h->img_cap) Bc += left;
        plan.push_back(Bc);
        b0 += Bc;
    }
    return plan;
}

int ovmr_set_option(ovmr_handle* h, const char* key, int value) {
    if (!h || !key) return OVMR_E_ARG;
    if (!strcmp(key, "gemm")) h->gemm_variant = value;
    else if (!strcmp(key, "attn")) h->attn_variant = value;
    else if (!strcmp(key, "fuse_im2col")) h->fuse_im2col = value != 0;
    else if (!strcmp(key, "last_q_cls")) h->last_q_cls = value != 0;
    else if (!strcmp(key, "enc_chunk")) {
        h->enc_chunk_forced = value > 0 ? value : 0;
        if (h->finalized) set_enc_chunk(h);
    }
    else if (!strcmp(key, "ln_fold")) h->ln_fold = value;
    else if (!strcmp(key, "xval_fused")) h->xval_fused = value;
    else if (!strcmp(key, "fused_head")) h->fused_head = value;
    else if (!strcmp(key, "head_max_grid")) h->head_max_grid = value;
    else if (!strcmp(key, "gelu_exact")) h->gelu_exact = value;
    else if (!strcmp(key, "gemm_persist")) h->gemm_persist = value != 0;
    else if (!strcmp(key, "agg_max_len")) {
        if (value < 128 || value > OVMR_AGG_MAX_LEN_CEILING)
            return fail(h, OVMR_E_ARG, "agg_max_len %d outside [128,%d]", value, OVMR_AGG_MAX_LEN_CEILING);
        h->agg_max_len = value;
    }
    else return fail(h, OVMR_E_NAME, "unknown option '%s'", key);
    return 0;
}

float ovmr_logit_scale(const ovmr_handle* h) { return h ? h->logit_scale_exp : 0.f; }

int ovmr_preprocess_u8(const void* u8_hwc, int B, int R, const float* mean3, const float* std3, void* out_f16, ovmr_stream stream) {
    if (B == 0) return 0;
    if (!u8_hwc || !out_f16 || !mean3 || !std3 || B < 0 || R <= 0) return OVMR_E_ARG;
    if (R % 8) return OVMR_E_SHAPE;
    return launch_preprocess_u8((const uint8_t*)u8_hwc, (half_t*)out_f16, B, R, mean3, std3, (hipStream_t)stream);
}

int ovmr_resize_crop_u8(const void* pixels, const ovmr_resize_job* jobs, int n, const int32_t* tables, void* tmp, int max_ny,
                        void* out_u8, int R, ovmr_stream stream) {
    if (n == 0) return 0;
    if (!pixels || !jobs || !tables || !out_u8 || n < 0 || R <= 0 || max_ny < 0 || (max_ny > 0 && !tmp)) return OVMR_E_ARG;
    return launch_resize_crop_u8((const uint8_t*)pixels, jobs, n, tables, (uint8_t*)tmp, max_ny, (uint8_t*)out_u8, R, (hipStream_t)stream);
}

int ovmr_set_weight(ovmr_handle* h, const char* name_c, const void* data, int dtype, int ndim,
                    const int64_t* shape, ovmr_stream stream) {
    if (!h || !name_c || !data || (dtype != OVMR_F16 && dtype != OVMR_F32) || ndim < 0 || ndim > 4) return OVMR_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const std::string name(name_c);
    size_t elems = 1;
    for (int i = 0; i < ndim; ++i) elems *= (size_t)shape[i];
    if (name == "logit_scale") {
        if (elems != 1) return fail(h, OVMR_E_SHAPE, "logit_scale must be a scalar");
        float v = 0.f;
        if (dtype == OVMR_F32) {
            HIP_CHECK_RET(hipMemcpyAsync(&v, data, 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK_RET(hipStreamSynchronize(s));
        } else {
            half_t hv;
            HIP_CHECK_RET(hipMemcpyAsync(&hv, data, 2, hipMemcpyDeviceToHost, s));
            HIP_CHECK_RET(hipStreamSynchronize(s));
            v = (float)hv;
        }
        h->logit_scale_exp = expf(v);     // logit_scale.exp(), trainers/mm_classifier_one_prompt.py:238,296
        h->have_logit_scale = true;
        return 0;
    }
    int f32 = -1;                         // the stored dtype, from the tables; -1: no table has the name
    Block none;
    for (const Tower& t : towers(h))
        if (name.rfind(t.prefix, 0) == 0)
            for (const Weight& wt : block_weights(0, none))
                if (ends_with(name, wt.name)) f32 = wt.f32 || t.f32;
    for (const Weight& wt : single_weights(h))
        if (name == wt.name) f32 = wt.f32;
    if (f32 < 0) return fail(h, OVMR_E_NAME, "unknown weight name '%s'", name_c);
    Buf& b = h->w[name];
    b.f32 = f32;
    if (!b.p || b.elems != elems) {
        b.p = dev_alloc(h->owned, elems * (b.f32 ? 4 : 2));
        if (!b.p) return fail(h, OVMR_E_NOMEM, "hipMalloc failed for '%s'", name_c);
    }
    b.elems = elems;
    b.shape.assign(shape, shape + ndim);
    h->finalized = false;
    return launch_cast(data, dtype == OVMR_F32, b.p, b.f32, (long)elems, s);
}

int ovmr_finalize(ovmr_handle* h, int max_images, int max_prompts, int max_classes, ovmr_stream stream) {
    if (!h || max_images < 1 || max_prompts < 1 || max_classes < 1) return OVMR_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const ovmr_model_desc& d = h->d;
    const size_t W = d.vision_width, T = d.transformer_width, E = d.embed_dim, P = d.vision_patch_size;
    if (!h->have_logit_scale) return fail(h, OVMR_E_STATE, "weight 'logit_scale' was never set");

    for (const Tower& t : towers(h)) {
        t.blocks->assign(t.layers, Block());
        for (int i = 0; i < t.layers; ++i)
            for (const Weight& wt : block_weights(t.width, (*t.blocks)[i]))
                if (int rc = bind_weight(h, t.prefix + std::to_string(i) + "." + wt.name, wt)) return rc;
    }
    for (const Weight& wt : single_weights(h))
        if (int rc = bind_weight(h, wt.name, wt)) return rc;

    // derived layouts of a previous finalize are dropped first (the stream is idle: every finalize ends with a sync)
    HIP_CHECK_RET(hipStreamSynchronize(s));
    for (void* p : h->derived) (void)hipFree(p);
    h->derived.clear();
    auto dalloc = [&](size_t bytes) { return dev_alloc(h->derived, bytes); };
    h->conv_w = (half_t*)dalloc(W * h->Kpad * 2);
    h->pos16_vis = (half_t*)dalloc((size_t)h->L * W * 2);
    h->cls_pos16 = (half_t*)dalloc(W * 2);
    h->proj_t = (half_t*)dalloc(E * W * 2);
    h->pos16_txt = (half_t*)dalloc((size_t)d.context_length * T * 2);
    h->textproj_t = (half_t*)dalloc(E * T * 2);
    half_t* cls16 = (half_t*)dalloc(W * 2);
    if (!h->conv_w || !h->pos16_vis || !h->cls_pos16 || !h->proj_t || !h->pos16_txt || !h->textproj_t || !cls16)
        return fail(h, OVMR_E_NOMEM, "hipMalloc failed for derived weights");
    CK(launch_pad_rows_f16((const half_t*)h->conv1, h->conv_w, (int)W, (int)(3 * P * P), h->Kpad, s));
    CK(launch_cast(h->pos_vis, 1, h->pos16_vis, 0, (long)h->L * W, s));        // positional_embedding.to(fp16), clip/model.py:416
    CK(launch_cast(h->cls_emb, 1, cls16, 0, (long)W, s));                      // class_embedding.to(fp16), :415
    CK(launch_add_f16(cls16, h->pos16_vis, h->cls_pos16, (long)W, s));
    CK(launch_transpose_to_f16(h->proj, 0, h->proj_t, (int)W, (int)E, s));     // x @ proj == x * proj^T^T
    CK(launch_cast(h->pos_txt, 1, h->pos16_txt, 0, (long)d.context_length * T, s));
    CK(launch_transpose_to_f16(h->textproj, 0, h->textproj_t, (int)T, (int)E, s));

    // LayerNorm folded into in_proj / c_fc of the two fp16 towers (common.h EPI_LN_BIAS)
    for (auto* tower : {&h->vis, &h->txt}) {
        const size_t Wd = tower == &h->vis ? W : T;
        if (Wd % 256) continue;                                                  // the statistics come in 256-column slots
        for (Block& k : *tower) {
            k.in_wf = (half_t*)dalloc(3 * Wd * Wd * 2); k.in_g = (float*)dalloc(3 * Wd * 4); k.in_bf = (float*)dalloc(3 * Wd * 4);
            k.fc_wf = (half_t*)dalloc(4 * Wd * Wd * 2); k.fc_g = (float*)dalloc(4 * Wd * 4); k.fc_bf = (float*)dalloc(4 * Wd * 4);
            if (!k.in_wf || !k.in_g || !k.in_bf || !k.fc_wf || !k.fc_g || !k.fc_bf)
                return fail(h, OVMR_E_NOMEM, "hipMalloc failed for LayerNorm-folded weights");
            CK(launch_fold_ln((const half_t*)k.in_w, k.ln1_g, k.ln1_b, (const half_t*)k.in_b, k.in_wf, k.in_g, k.in_bf, (int)(3 * Wd), (int)Wd, s));
            CK(launch_fold_ln((const half_t*)k.fc_w, k.ln2_g, k.ln2_b, (const half_t*)k.fc_b, k.fc_wf, k.fc_g, k.fc_bf, (int)(4 * Wd), (int)Wd, s));
        }
    }

    // workspace: one arena for the largest of the four passes (image_ws, text_ws, AggWs, HeadWs)
    h->max_images = max_images; h->max_prompts = max_prompts; h->max_classes = max_classes;
    {
        int dev = 0;
        HIP_CHECK_RET(hipGetDevice(&dev));
        HIP_CHECK_RET(hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        set_enc_chunk(h);
    }
    {
        // fold slack: one round of the narrowest grid (N = W: W/256 column tiles of 256 rows), for reserves of two rounds or more
        const long nw = std::max<long>(1, (long)W / 256), round_images = (long)h->n_cu * 256 / (nw * h->L);
        const bool big = ((long)max_images * h->L + 255) / 256 * nw >= 2L * h->n_cu;
        h->enc_fold = big ? (int)std::min<long>(round_images, max_images / 4) : 0;
        h->img_cap = max_images + h->enc_fold;
    }
    // (the longest class the option lets through fits a chunk of its own; at the option's default the capacity is what it always was)
    h->agg_rows_cap = std::max((long)max_classes * (d.n_ctx + 32), h->agg_max_len > 128 ? (long)h->agg_max_len : 0L);
    h->logit_elems_cap = 32L << 20;
    const size_t need = std::max({image_ws(h, nullptr, h->img_cap).bytes(), text_ws(h, nullptr, (size_t)max_prompts * d.context_length, max_prompts).bytes(),
                                  AggWs(h, nullptr, h->agg_rows_cap).bytes(), HeadWs(h, nullptr, 3).bytes()});
    if (need > h->ws_bytes) {
        if (h->ws) (void)hipFree(h->ws);
        h->ws = nullptr;
        if (hipMalloc((void**)&h->ws, need) != hipSuccess) return fail(h, OVMR_E_NOMEM, "workspace of %zu bytes", need);
        h->ws_bytes = need;
    }
    HIP_CHECK_RET(hipStreamSynchronize(s));
    h->finalized = true;
    return 0;
}

int ovmr_encode_image(ovmr_handle* h, const void* image, int image_dtype, int B, void* out_f16, int normalize,
                      ovmr_stream stream) {
    if (h && B == 0) return 0;   // empty batch: torch hands out a null data_ptr
    if (!h || !image || !out_f16 || B < 0 || (image_dtype != OVMR_F16 && image_dtype != OVMR_F32)) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const ovmr_model_desc& d = h->d;
    const int W = d.vision_width, R = d.image_resolution, L = h->L, G2 = h->G * h->G, E = d.embed_dim;
    const size_t px = (size_t)3 * R * R * (image_dtype == OVMR_F32 ? 4 : 2);
    // a batch that fits the workspace is ONE launch sequence; a larger one is split into chunks of enc_chunk images (pick_encode_chunk),
    // unless the option pins the chunk; a sub-round remainder joins the last chunk (encode_plan)
    int b0 = 0;
    for (const int Bc : encode_plan(h, B)) {
        const int M = Bc * L;
        const TowerWs ws = image_ws(h, h->ws, Bc);
        half_t *col = ws.col, *x = ws.x, *rows = ws.rows;
        half_t* out = (half_t*)out_f16 + (size_t)b0 * E;
        // K1/K2: conv1 as GEMM over patches, positional add in the epilogue, CLS row, ln_pre
        // fp16 images with 16 x 16 patches: the GEMM's K loop gathers the patch rows from the image itself (gemm_f16_v5.hip, a.im2col_R);
        // otherwise (fp32 images, other patch sizes, a handful of rows, the 128 x 128 kernel) an im2col pass writes them out first
        const bool fused_patches = h->fuse_im2col && image_dtype == OVMR_F16 && d.vision_patch_size == 16 && h->Kpad == 768 && (R & 15) == 0 &&
                                   Bc * G2 >= 256 && W >= 128 && h->gemm_variant >= 1 && ((uintptr_t)image & 15) == 0;
        GemmArgs pe;
        if (fused_patches) {
            pe = gemm_patches((const char*)image + (size_t)b0 * px, R, h->conv_w, h->pos16_vis, x, Bc, W);
        } else {
            CK(launch_im2col((const char*)image + (size_t)b0 * px, image_dtype == OVMR_F32, col, Bc, R, d.vision_patch_size, h->Kpad, s));
            pe = gemm(col, h->Kpad, h->conv_w, h->Kpad, x, W, Bc * G2, W, h->Kpad, EPI_PATCH);
            pe.pos = h->pos16_vis; pe.rows_in = G2; pe.rows_out = L;
        }
        CK(launch_gemm_f16(pe, h->gemm_variant, s));
        CK(launch_fill_cls(x, h->cls_pos16, Bc, L, W, s));
        CK(launch_layernorm(x, x, h->ln_pre_g, h->ln_pre_b, M, W, W, 0, s));
        float* stats = can_fold_ln(h, h->vis[0], M, W) ? ws.stats : nullptr;
        if (stats) CK(launch_row_stats(x, stats, M, W, W / 256, s));
        for (size_t li = 0; li < h->vis.size(); ++li)           // the last block leaves its CLS rows in `rows` (run_block_f16, cls_rows)
            CK(run_block_f16(h, h->vis[li], x, ws.y, ws.qkv, ws.hid, Bc, L, W, 0, s, stats, nullptr, li + 1 == h->vis.size() ? rows : nullptr));
        // K9: ln_post on the CLS rows, projection; K10: normalise
        CK(launch_layernorm(rows, rows, h->ln_post_g, h->ln_post_b, Bc, W, W, 0, s));
        CK(launch_gemm_f16(gemm(rows, W, h->proj_t, W, out, E, Bc, E, W, EPI_NONE), h->gemm_variant, s));
        CK(normalize_rows(h, out, Bc, E, normalize ? 1 : 0, s));
        b0 += Bc;
    }
    return 0;
}

int ovmr_encode_plan(const ovmr_handle* h, int B, int* sizes, int max_sizes) {
    if (!h || !h->finalized || B < 0) return -1;
    const std::vector<int> plan = encode_plan(h, B);
    for (size_t i = 0; i < plan.size() && (int)i < max_sizes; ++i) sizes[i] = plan[i];
    return (int)plan.size();
}

int ovmr_encode_text_embedded(ovmr_handle* h, const void* prompts_f16, const int32_t* index, int N, int seq_len,
                              void* out_f16, int normalize, ovmr_stream stream) {
    if (h && N == 0) return 0;
    if (!h || !prompts_f16 || !index || !out_f16 || N < 0) return OVMR_E_ARG;
    if (int rc = check_text_call(h, seq_len, normalize)) return rc;
    TextGroup g;
    g.prompts = (const half_t*)prompts_f16; g.index = index; g.N = N; g.Ls = seq_len; g.normalize = normalize; g.out = (half_t*)out_f16;
    return run_text_group_chunked(h, g, (hipStream_t)stream);
}

int ovmr_encode_text_ids(ovmr_handle* h, const int64_t* ids, int N, int seq_len, void* out_f16, int normalize,
                         ovmr_stream stream) {
    if (h && N == 0) return 0;
    if (!h || !ids || !out_f16 || N < 0) return OVMR_E_ARG;
    if (int rc = check_text_call(h, seq_len, normalize)) return rc;
    TextGroup g;
    g.ids = ids; g.N = N; g.Ls = seq_len; g.normalize = normalize; g.out = (half_t*)out_f16;
    return run_text_group_chunked(h, g, (hipStream_t)stream);
}

int ovmr_encode_text_groups(ovmr_handle* h, const ovmr_text_group* groups, int n_groups, ovmr_stream stream) {
    if (!h || (!groups && n_groups > 0) || n_groups < 0) return OVMR_E_ARG;
    std::vector<TextGroup> gs;
    size_t M = 0, N = 0;
    for (int i = 0; i < n_groups; ++i) {
        const ovmr_text_group& u = groups[i];
        if (u.n == 0) continue;
        if (u.n < 0 || !u.out_f16 || (!u.ids && (!u.prompts_f16 || !u.index)) || (u.ids && u.prompts_f16)) return OVMR_E_ARG;
        if (int rc = check_text_call(h, u.seq_len, u.normalize)) return rc;
        TextGroup g;
        g.prompts = (const half_t*)u.prompts_f16; g.ids = u.ids; g.index = u.index; g.N = u.n; g.Ls = u.seq_len;
        g.normalize = u.normalize; g.out = (half_t*)u.out_f16;
        gs.push_back(g);
        M += (size_t)u.n * u.seq_len; N += u.n;
    }
    if (gs.empty()) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (text_ws(h, nullptr, M, N).bytes() <= h->ws_bytes) return run_text_groups(h, gs, s);      // one pass over all groups
    for (auto& g : gs) CK(run_text_group_chunked(h, g, s));                                    // too many rows for the workspace
    return 0;
}

int ovmr_encode_text_ensemble(ovmr_handle* h, const int64_t* ids, int T, int C, const int32_t* seq_lens, void* out_f16,
                              ovmr_stream stream) {
    if (!h || T < 1 || C < 0) return OVMR_E_ARG;
    if (C == 0) return 0;
    if (!ids || !out_f16) return OVMR_E_ARG;
    const int Lc = h->d.context_length, E = h->d.embed_dim;
    size_t sumL = 0;
    for (int t = 0; t < T; ++t) {
        if (int rc = check_text_call(h, seq_lens ? seq_lens[t] : Lc, 0)) return rc;
        sumL += seq_lens ? seq_lens[t] : Lc;
    }
    // chunk of classes: the tower's rows for all T templates of c classes, then the [T, c, E] scratch of raw rows behind them
    auto need = [&](size_t c) { return EnsembleWs(h, nullptr, c * sumL, c * T).bytes(); };
    if (need(1) > h->ws_bytes)
        return fail(h, OVMR_E_SHAPE, "the %d prompts of one class (%zu token rows) do not fit the workspace of %zu bytes: finalize with a "
                    "larger reserve", T, sumL, h->ws_bytes);
    size_t lo = 1, hi = (size_t)C;                       // largest c with need(c) <= ws_bytes (need grows with c)
    while (lo < hi) {
        const size_t mid = (lo + hi + 1) / 2;
        if (need(mid) <= h->ws_bytes) lo = mid; else hi = mid - 1;
    }
    const int n_chunks = (int)((C + lo - 1) / lo);       // balanced chunks of at most `lo` classes
    hipStream_t s = (hipStream_t)stream;
    std::vector<TextGroup> gs(T);
    for (int i = 0, c0 = 0; i < n_chunks; ++i) {
        const int cc = C / n_chunks + (i < C % n_chunks ? 1 : 0);
        half_t* raw = EnsembleWs(h, h->ws, (size_t)cc * sumL, (size_t)cc * T).raw;
        for (int t = 0; t < T; ++t) {                    // ids are template-major: [T, C, context_length]
            TextGroup& g = gs[t];
            g.ids = ids + ((size_t)t * C + c0) * Lc; g.N = cc; g.Ls = seq_lens ? seq_lens[t] : Lc; g.normalize = 0;
            g.out = raw + (size_t)t * cc * E;
        }
        CK(run_text_groups(h, gs, s));
        CK(launch_text_ensemble(raw, T, cc, E, (half_t*)out_f16 + (size_t)c0 * E, s));
        c0 += cc;
    }
    return 0;
}

int ovmr_embed_tokens(ovmr_handle* h, const int64_t* ids, int N, int L, void* out_f16, ovmr_stream stream) {
    if (h && N == 0) return 0;
    if (!h || !ids || !out_f16 || N < 0 || L < 1) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    return launch_embed_gather(ids, h->tok_emb, (half_t*)out_f16, (long)N * L, h->d.transformer_width, (hipStream_t)stream);
}

int ovmr_generate_tokens(ovmr_handle* h, const void* feats_f16, int Cb, int S, float* tokens_f32, ovmr_stream stream) {
    if (h && Cb == 0) return 0;
    if (!h || !feats_f16 || !tokens_f32 || Cb < 0 || S < 1) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    const ovmr_model_desc& d = h->d;
    const int D = d.embed_dim, La = d.n_ctx + S;
    if (La > h->agg_max_len) return fail(h, OVMR_E_SHAPE, "n_ctx + shots = %d exceeds %d", La, h->agg_max_len);
    return generate_tokens(h, (const half_t*)feats_f16, nullptr, S, nullptr, Cb, Cb * S, tokens_f32, (hipStream_t)stream);
}

int ovmr_generate_tokens_ragged(ovmr_handle* h, const void* feats_f16, const int32_t* shots_host, const int32_t* offsets_dev,
                                int Cb, int R, float* tokens_f32, ovmr_stream stream) {
    if (h && Cb == 0) return 0;
    if (!h || !feats_f16 || !shots_host || !offsets_dev || !tokens_f32 || Cb < 0 || R < 0) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    const ovmr_model_desc& d = h->d;
    const int D = d.embed_dim;
    long sum = 0;
    for (int c = 0; c < Cb; ++c) {
        if (shots_host[c] < 1) return fail(h, OVMR_E_SHAPE, "class %d of the call has %d exemplars, at least 1 is needed", c, (int)shots_host[c]);
        if (d.n_ctx + (long)shots_host[c] > h->agg_max_len)
            return fail(h, OVMR_E_SHAPE, "class %d of the call: n_ctx + shots = %ld exceeds %d", c, d.n_ctx + (long)shots_host[c], h->agg_max_len);
        sum += shots_host[c];
    }
    if (sum != R) return fail(h, OVMR_E_SHAPE, "the shots add up to %ld rows, feats has %d", sum, R);
    return generate_tokens(h, (const half_t*)feats_f16, shots_host, 0, offsets_dev, Cb, R, tokens_f32, (hipStream_t)stream);
}

int ovmr_assemble_prompts(ovmr_handle* h, const void* base_f16, const int64_t* labels, const float* tokens_f32, int Cb,
                          void* out_f16, ovmr_stream stream) {
    if (h && Cb == 0) return 0;
    if (!h || !base_f16 || !tokens_f32 || !out_f16 || Cb < 0) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    if (h->d.embed_dim != h->d.transformer_width)
        return fail(h, OVMR_E_SHAPE, "visual tokens (embed_dim %d) do not fit the text width %d", h->d.embed_dim, h->d.transformer_width);
    CK(launch_assemble_prompts((const half_t*)base_f16, labels, tokens_f32, (half_t*)out_f16, Cb, h->d.context_length,
                               h->d.n_ctx, h->d.transformer_width, (hipStream_t)stream));
    return 0;
}

int ovmr_xval_counts(ovmr_handle* h, const void* feats_f16, const int32_t* labels, int R, const void* clf_f16, int C,
                     int32_t* tp, int32_t* n_pred, ovmr_stream stream) {
    if (h && R == 0) return 0;
    if (!h || !feats_f16 || !labels || !clf_f16 || !tp || !n_pred || R < 0 || C < 1) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int D = h->d.embed_dim;
    half_t* logits = HeadWs(h, h->ws, 1).l[0];
    if (h->xval_fused && R >= 256 && C >= 128) {
        // K18 + K19 fused: the [R, C] logits never reach HBM.  The GEMM epilogue leaves one
        // (maximum, lowest column) pair per row and 256-column tile; a row kernel finishes the argmax and counts.
        const int tiles = (C + 255) / 256;
        float* partial = (float*)logits;                                  // 2 floats per (row, tile) in the logits workspace
        const long cap_rows = std::min<long>(std::max<long>(512, h->logit_elems_cap / (4L * tiles)), 1L << 22);
        if (cap_rows * tiles * 8 > h->logit_elems_cap * 2) return fail(h, OVMR_E_SHAPE, "class count %d too large for the logits workspace", C);
        const long n_chunks = (R + cap_rows - 1) / cap_rows;              // balanced chunks: each has > cap_rows / 2 >= 256 rows
        for (long i = 0, r0 = 0; i < n_chunks; ++i) {
            const int Rc = (int)(R / n_chunks + (i < R % n_chunks ? 1 : 0));
            GemmArgs g = gemm((const half_t*)feats_f16 + (size_t)r0 * D, D, clf_f16, D, nullptr, C, Rc, C, D, EPI_SCALE_ARGMAX);
            g.scale = h->logit_scale_exp;
            g.argmax_out = partial;
            CK(launch_gemm_f16(g, h->gemm_variant, s));
            CK(launch_argmax_reduce(partial, tiles, labels + r0, Rc, C, tp, n_pred, s));
            r0 += Rc;
        }
        return 0;
    }
    const int chunk = (int)std::min<long>(std::max<long>(64, h->logit_elems_cap / C), 1L << 20);
    for (int r0 = 0; r0 < R; r0 += chunk) {
        const int Rc = std::min(chunk, R - r0);
        if ((long)Rc * C > h->logit_elems_cap) return fail(h, OVMR_E_SHAPE, "class count %d too large for the logits workspace", C);
        GemmArgs g = gemm((const half_t*)feats_f16 + (size_t)r0 * D, D, clf_f16, D, logits, C, Rc, C, D, EPI_SCALE);
        g.scale = h->logit_scale_exp;
        CK(launch_gemm_f16(g, h->gemm_variant, s));
        CK(launch_argmax_counts(logits, C, labels + r0, Rc, C, tp, n_pred, s));
    }
    return 0;
}

int ovmr_fusion_weights(ovmr_handle* h, const int32_t* counts, const int32_t* n_label, int C, float tau, float* out_f32,
                        ovmr_stream stream) {
    if (!h || !counts || !n_label || !out_f32 || C < 1) return OVMR_E_ARG;
    CK(launch_fusion_weights(counts, n_label, C, tau, out_f32, (hipStream_t)stream));
    return 0;
}

int ovmr_head_plan(const ovmr_handle* h, int B, int C) {
    if (!h || !h->finalized || B < 0 || C < 1) return -1;
    return head_takes_one_launch(h, B, C) && h->d.embed_dim % 64 == 0 ? 1 : 0;
}

int ovmr_pack_rows(const void* mm, const void* v, const void* t, const void* tokens, const int64_t* labels, int n, int D, int n_ctx, int bound,
                   void* block, ovmr_stream stream) {
    if (bound == 0) return 0;
    if (!mm || !v || !t || !tokens || !block || (n > 0 && !labels) || n < 0 || bound < n || D < 2 || (D & 1) || n_ctx < 1) return OVMR_E_ARG;
    return launch_pack_rows((const half_t*)mm, (const half_t*)v, (const half_t*)t, (const half_t*)tokens, labels, n, D, n_ctx, bound,
                            (half_t*)block, (hipStream_t)stream);
}

int ovmr_unpack_rows(const void* gathered, int rows, int C, int D, int n_ctx, void* mm, void* v, void* t, void* tokens, int32_t* seen,
                     ovmr_stream stream) {
    if (rows == 0) return 0;
    if (!gathered || !mm || !v || !t || !tokens || !seen || rows < 0 || C < 1 || D < 2 || (D & 1) || n_ctx < 1) return OVMR_E_ARG;
    return launch_unpack_rows((const half_t*)gathered, rows, C, D, n_ctx, (half_t*)mm, (half_t*)v, (half_t*)t, (half_t*)tokens, seen,
                              (hipStream_t)stream);
}

int ovmr_eval_counts(const void* outputs, int dtype, long ld, const int64_t* labels, int B, int C, int32_t* counts, ovmr_stream stream) {
    if (B == 0) return 0;
    if (!outputs || !labels || !counts || B < 0 || C < 1 || ld < C || (dtype != OVMR_F16 && dtype != OVMR_F32)) return OVMR_E_ARG;
    return launch_eval_counts(outputs, dtype == OVMR_F32, ld, labels, B, C, counts, (hipStream_t)stream);
}

int ovmr_topk_rows(const void* outputs, int dtype, long ld, int B, int C, int k, float* values, int32_t* indices, const int64_t* labels,
                   int32_t* hits, ovmr_stream stream) {
    if (B == 0) return 0;
    if (!outputs || !indices || B < 0 || k < 1 || k > C || k > 32 || ld < C || (dtype != OVMR_F16 && dtype != OVMR_F32) || !labels != !hits)
        return OVMR_E_ARG;
    return launch_topk_rows(outputs, dtype == OVMR_F32, ld, B, C, k, values, indices, labels, hits, (hipStream_t)stream);
}

int ovmr_eval_detail(const void* outputs, int dtype, long ld, const int64_t* labels, int B, int C, int k, int32_t* counts, int32_t* hits,
                     int32_t* class_hits, int32_t* cmat, ovmr_stream stream) {
    if (B == 0) return 0;
    if (!outputs || !labels || !counts || B < 0 || C < 1 || k < 1 || k > C || k > 32 || ld < C || (dtype != OVMR_F16 && dtype != OVMR_F32))
        return OVMR_E_ARG;
    return launch_eval_detail(outputs, dtype == OVMR_F32, ld, labels, B, C, k, counts, hits, class_hits, cmat, (hipStream_t)stream);
}

int ovmr_fused_logits(ovmr_handle* h, const void* feats_f16, int B, const void* mm, const void* v, const void* t,
                      const float* w, int C, int mode, float* out_f32, ovmr_stream stream) {
    if (h && B == 0) return 0;
    if (!h || !feats_f16 || !out_f32 || B < 0 || C < 1) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    const half_t *cm = (const half_t*)mm, *cv = (const half_t*)v, *ct = (const half_t*)t;
    HeadCall c = {(const half_t*)feats_f16, B, {nullptr, nullptr, nullptr}, 1, nullptr, C, out_f32, 0, nullptr};
    switch (mode) {
        case OVMR_MODE_FUSION: c.clf[0] = cm; c.clf[1] = cv; c.clf[2] = ct; c.n_mod = 3; c.w = w; if (!w) return OVMR_E_ARG; break;   // column order mm, v, t (:361)
        case OVMR_MODE_TEXT: c.clf[0] = ct; break;
        case OVMR_MODE_VISION: c.clf[0] = cv; break;
        case OVMR_MODE_MULTIMODAL: c.clf[0] = cm; break;
        default: return fail(h, OVMR_E_ARG, "unknown eval mode %d", mode);
    }
    for (int m = 0; m < c.n_mod; ++m) if (!c.clf[m]) return fail(h, OVMR_E_ARG, "classifier %d is NULL for mode %d", m, mode);
    return run_head(h, c, (hipStream_t)stream);
}

// The four eval modes of one batch from one pass over the head (EVAL_MODE all): the route, the options and the workspace of
// ovmr_fused_logits(mode = fusion); the launch that writes the weighted sum also stores the three softmaxes it is made of.
int ovmr_fused_logits_all(ovmr_handle* h, const void* feats_f16, int B, const void* mm, const void* v, const void* t,
                          const float* w, int C, float* out_f32, long plane_stride, ovmr_stream stream) {
    if (h && B == 0) return 0;
    if (!h || !feats_f16 || !mm || !v || !t || !w || !out_f32 || B < 0 || C < 1 || plane_stride < (long)B * C) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    const HeadCall c = {(const half_t*)feats_f16, B, {(const half_t*)mm, (const half_t*)v, (const half_t*)t}, 3, w, C, out_f32, plane_stride, nullptr};   // column order mm, v, t (:361)
    return run_head(h, c, (hipStream_t)stream);
}

int ovmr_zeroshot_logits(ovmr_handle* h, const void* feats_f16, int B, const void* text_f16, int C, void* out_f16,
                         ovmr_stream stream) {
    if (h && B == 0) return 0;
    if (!h || !feats_f16 || !text_f16 || !out_f16 || B < 0 || C < 1) return OVMR_E_ARG;
    if (int rc = need_finalized(h)) return rc;
    const HeadCall c = {(const half_t*)feats_f16, B, {(const half_t*)text_f16, nullptr, nullptr}, 1, nullptr, C, nullptr, 0, (half_t*)out_f16};
    return run_head(h, c, (hipStream_t)stream);
}

// Closed-form FLOPs (2*MAC), SURVEY.md section 2.3: per layer 24*L*W^2 (QKV 6, out 2, MLP 16) + 4*L^2*W
static double tower_flops(double L, double W, double layers) { return layers * (24.0 * L * W * W + 4.0 * L * L * W); }

int ovmr_encode_chunk(const ovmr_handle* h) { return h && h->finalized ? (h->enc_chunk > 0 ? h->enc_chunk : h->max_images) : 0; }

double ovmr_flops_per_image(const ovmr_handle* h) {
    if (!h) return 0;
    const ovmr_model_desc& d = h->d;
    const double G2 = (double)h->G * h->G, W = d.vision_width, K = 3.0 * d.vision_patch_size * d.vision_patch_size;
    return 2.0 * G2 * K * W + tower_flops(h->L, W, d.vision_layers) + 2.0 * W * d.embed_dim;
}
// FLOPs of one image with the last block as launched: K/V projection of all tokens (4 L W^2), then one query row: scores + PV (4 L W),
// out_proj (2 W^2), MLP (16 W^2).  Q: for the CLS row alone (2 W^2) where the launch sequence holds >= 256 images and last_q_cls is
// set (q_cls), else for every token (2 L W^2)
static double image_flops_executed(const ovmr_handle* h, bool q_cls) {
    const double L = h->L, W = h->d.vision_width;
    const double last_full = 24.0 * L * W * W + 4.0 * L * L * W;
    const double last_run = 4.0 * L * W * W + 4.0 * L * W + 18.0 * W * W + (q_cls ? 2.0 * W * W : 2.0 * L * W * W);
    return ovmr_flops_per_image(h) - last_full + last_run;
}
double ovmr_flops_per_image_executed(const ovmr_handle* h) {
    if (!h) return 0;
    // (what ovmr_encode_image does for a reserve of that size)
    return image_flops_executed(h, h->last_q_cls && (!h->finalized || std::min(h->max_images, h->enc_chunk > 0 ? h->enc_chunk : h->max_images) >= 256));
}
double ovmr_flops_executed(const ovmr_handle* h, int B) {
    if (!h || !h->finalized || B <= 0) return 0;
    double total = 0;
    for (const int Bc : encode_plan(h, B))                 // the launch sequences ovmr_encode_image runs for this batch
        total += Bc * image_flops_executed(h, h->last_q_cls && Bc >= 256);
    return total;
}
double ovmr_flops_per_prompt(const ovmr_handle* h, int seq_len) {
    if (!h) return 0;
    const ovmr_model_desc& d = h->d;
    return tower_flops(seq_len, d.transformer_width, d.transformer_layers) + 2.0 * d.transformer_width * d.embed_dim;
}

}  // extern "C"

// ---- unit-test hooks (tests/test_hip_kernels.py): one kernel per call, no handle state -----------
extern "C" {

int ovmr_debug_gemm(int f32, int variant, const void* A, const void* W, const void* bias, const void* res,
                    const void* pos, void* C, int M, int N, int K, int ldc, int epi, float scale,
                    int rows_in, int rows_out, ovmr_stream stream) {
    GemmArgs a = gemm(A, K, W, K, C, ldc, M, N, K, epi, bias, res, ldc);
    a.pos = pos; a.scale = scale; a.rows_in = rows_in; a.rows_out = rows_out;
    if (epi == EPI_LN_BIAS || epi == EPI_LN_BIAS_QGELU) {   // LN-folding epilogues: bias = ln_b fp32 [N], pos = ln_g fp32 [N], res = statistics fp32 [M][K/256][2]
        a.ln_b = (const float*)bias; a.ln_g = (const float*)pos; a.ln_stats = (const float*)res; a.ln_slots = K / 256;
        a.bias = nullptr; a.pos = nullptr; a.res = nullptr;
    }
    if (epi == EPI_SCALE_ARGMAX) {                          // fused row argmax: C receives fp32 [M][ceil(N/256)][2] = (max, column bits)
        a.argmax_out = (float*)C;
        a.C = nullptr;
    }
    if (epi == EPI_BIAS_RES && pos) {                       // statistics epilogue: pos = fp32 [M][N/256][2] output
        a.stats_out = (float*)pos;
        a.pos = nullptr;
    }
    return f32 ? launch_gemm_f32(a, (hipStream_t)stream) : launch_gemm_f16(a, variant, (hipStream_t)stream);
}

// x1 = h(h(A1 W1^T + b1) + res) with the statistics epilogue, then C2 = h(LN(x1; gamma, beta) W2^T + b2) [QuickGELU] with
// the LayerNorm folded into the second GEMM.  Scratch is allocated here (debug / kernel-test hook only).
int ovmr_debug_lnfold(int variant, const void* A1, const void* W1, const void* b1, const void* res, int M, int D, int K1,
                      const void* W2, const float* gamma, const float* beta, const void* b2, int N2, int qgelu,
                      void* x1, void* C2, ovmr_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    if (D % 256 || N2 % 64) return OVMR_E_ARG;
    const int slots = D / 256;
    const LnFoldScratch f((size_t)M, W2, gamma, beta, b2, N2, D, s);
    int rc = f.rc;
    if (!rc && A1)
        rc = launch_gemm_f16(gemm_stats(gemm(A1, K1, W1, K1, x1, D, M, D, K1, EPI_BIAS_RES, b1, res, D), f.stats), variant, s);
    else if (!rc)
        rc = launch_row_stats((const half_t*)x1, f.stats, M, D, slots, s);     // A1 == NULL: x1 is an input
    if (!rc) rc = launch_gemm_f16(gemm_ln(gemm(x1, D, f.wf, D, C2, N2, M, N2, D, qgelu ? EPI_LN_BIAS_QGELU : EPI_LN_BIAS), f.stats, slots, f.g, f.bf), variant, s);
    return rc;
}

// ovmr_debug_gemm (fp16) with the operand strides of the engine's sub-matrix launches (the last vision block: CLS-row Q, K/V next
// to Q, out_proj of the CLS rows).  epi 6/7: W / bias are the RAW weight and bias, folded with gamma / beta here, and the statistics
// are those of the dense [(M-1)*row_step+1, K] buffer A strides over (lda = row_step * K), read with ln_stride = row_step * K/256.
int ovmr_debug_gemm_strided(int variant, const void* A, int lda, const void* W, int ldw, const void* bias, const void* res,
                            int ldres, void* C, int ldc, int M, int N, int K, int epi, float scale, const float* gamma,
                            const float* beta, int row_step, ovmr_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    if (epi == EPI_PATCH || epi == EPI_SCALE_ARGMAX || epi < 0 || epi > EPI_LN_BIAS_QGELU) return OVMR_E_ARG;
    GemmArgs a = gemm(A, lda, W, ldw, C, ldc, M, N, K, epi, bias, res, ldres);
    a.scale = scale;
    if (epi != EPI_LN_BIAS && epi != EPI_LN_BIAS_QGELU) return launch_gemm_f16(a, variant, s);
    if (K % 256 || K / 256 > 64 || row_step < 1 || (long)lda != (long)row_step * K || ldw != K || !gamma || !beta || !bias)
        return OVMR_E_ARG;
    if (M <= 0 || N <= 0) return 0;
    const int slots = K / 256;
    const long rows = (long)(M - 1) * row_step + 1;
    const LnFoldScratch f((size_t)rows, W, gamma, beta, bias, N, K, s);
    int rc = f.rc;
    if (!rc) rc = rows > 0x7fffffffL ? OVMR_E_ARG : launch_row_stats((const half_t*)A, f.stats, (int)rows, K, slots, s);
    if (!rc) {
        a = gemm_ln(gemm(A, lda, f.wf, K, C, ldc, M, N, K, epi), f.stats, slots, f.g, f.bf);
        a.ln_stride = row_step * slots;
        rc = launch_gemm_f16(a, variant, s);
    }
    return rc;
}

int ovmr_debug_layernorm(int f32, const void* x, void* y, const float* g, const float* b, int rows, int D,
                         long in_stride, ovmr_stream stream) {
    return launch_layernorm(x, y, g, b, rows, D, in_stride, f32, (hipStream_t)stream);
}

// The row kernels either side of the GEMMs (tests/test_hip_rowops_exact.py): argument checks and the launch, nothing else.
int ovmr_debug_l2norm(void* x_f16, int rows, int D, int times, ovmr_stream stream) {
    if (!x_f16 || rows < 0 || D < 4 || (D & 3) || times < 0) return OVMR_E_ARG;
    int rc = 0;
    for (int i = 0; i < times && !rc; ++i) rc = launch_l2norm_f16((half_t*)x_f16, rows, D, (hipStream_t)stream);
    return rc;
}

int ovmr_debug_text_ensemble(const void* feats_f16, int T, int rows, int E, void* out_f16, ovmr_stream stream) {
    if (!feats_f16 || !out_f16 || T < 1 || rows < 0 || E < 1 || ((uintptr_t)feats_f16 & 1) || ((uintptr_t)out_f16 & 1)) return OVMR_E_ARG;
    return launch_text_ensemble((const half_t*)feats_f16, T, rows, E, (half_t*)out_f16, (hipStream_t)stream);
}

int ovmr_debug_text_embed_ids(const int64_t* ids, int ids_stride, const float* tok_emb, const void* pos_f16, void* x_f16, int32_t* index,
                              int N, int Lctx, int Lseq, int D, ovmr_stream stream) {
    if (!ids || !tok_emb || !pos_f16 || !x_f16 || !index || N < 0 || Lseq < 1 || Lseq > Lctx || ids_stride < Lctx || D < 4 || (D & 3))
        return OVMR_E_ARG;
    return launch_text_embed_ids(ids, ids_stride, tok_emb, (const half_t*)pos_f16, (half_t*)x_f16, index, N, Lctx, Lseq, D, (hipStream_t)stream);
}

int ovmr_debug_text_add_pos(const void* prompts_f16, int Lctx, const void* pos_f16, void* x_f16, int N, int Lseq, int D, ovmr_stream stream) {
    if (!prompts_f16 || !pos_f16 || !x_f16 || N < 0 || Lseq < 1 || Lseq > Lctx || D < 4 || (D & 3)) return OVMR_E_ARG;
    return launch_text_add_pos((const half_t*)prompts_f16, Lctx, (const half_t*)pos_f16, (half_t*)x_f16, N, Lseq, D, (hipStream_t)stream);
}

int ovmr_debug_gather_rows(const void* x_f16, const int32_t* index, void* out_f16, int N, int Lseq, int D, ovmr_stream stream) {
    if (!x_f16 || !index || !out_f16 || N < 0 || Lseq < 1 || D < 4 || (D & 3)) return OVMR_E_ARG;
    return launch_gather_rows_f16((const half_t*)x_f16, index, (half_t*)out_f16, N, Lseq, D, (hipStream_t)stream);
}

// The front of the image tower (tests/test_hip_front_exact.py): argument checks and the launch, nothing else.
int ovmr_debug_im2col(const void* image, int image_dtype, int B, int R, int P, int Kpad, void* out_f16, ovmr_stream stream) {
    if (!image || !out_f16 || (image_dtype != OVMR_F16 && image_dtype != OVMR_F32) || B < 0 || R < 1 || P < 1 || R % P || Kpad < 3 * P * P ||
        (Kpad & 7) || ((uintptr_t)out_f16 & 15))
        return OVMR_E_ARG;
    return launch_im2col(image, image_dtype == OVMR_F32, (half_t*)out_f16, B, R, P, Kpad, (hipStream_t)stream);
}

int ovmr_debug_fill_cls(void* x_f16, const void* cls_pos_f16, int B, int L, int W, ovmr_stream stream) {
    if (!x_f16 || !cls_pos_f16 || B < 0 || L < 1 || W < 4 || (W & 3) || ((uintptr_t)x_f16 & 7) || ((uintptr_t)cls_pos_f16 & 7)) return OVMR_E_ARG;
    if (B == 0) return 0;
    return launch_fill_cls((half_t*)x_f16, (const half_t*)cls_pos_f16, B, L, W, (hipStream_t)stream);
}

// The fused launch of ovmr_encode_image: the same GemmArgs (gemm_patches) into the same launcher, whose rc comes back.  What the
// launcher refuses (gemm_f16_route): -2 for R % 16 != 0 or an image pointer that is not 16-byte aligned -- the LDS-DMA reads 16-byte
// chunks, so such a launch never starts; -4 for fewer than 256 patch rows, N < 128 or images of 2^31 bytes or more.
int ovmr_debug_gemm_patches(int variant, const void* image_f16, int R, const void* W_f16, const void* pos_f16, void* C_f16, int B, int N,
                            ovmr_stream stream) {
    if (!image_f16 || !W_f16 || !pos_f16 || !C_f16 || B < 0 || N < 0 || R < 0) return OVMR_E_ARG;
    return launch_gemm_f16(gemm_patches(image_f16, R, W_f16, pos_f16, C_f16, B, N), variant, (hipStream_t)stream);
}

int ovmr_debug_attention(int f32, int variant, const void* qkv, void* out, int B, int L, int H, int causal,
                         ovmr_stream stream) {
    // fp32: B equal sequences are the arithmetic mode of the aggregator's sequence table
    return f32 ? launch_attention_f32((const float*)qkv, (float*)out, AggSeqs{nullptr, 0, B, 0, L, B * L}, H, 128, (hipStream_t)stream)
               : launch_attention_f16((const half_t*)qkv, (half_t*)out, B, L, H, causal, variant, (hipStream_t)stream);
}

int ovmr_debug_attention_f32_varlen(const void* qkv, void* out, const int32_t* offsets_dev, int nseq, int n_ctx, int max_len, int H,
                                    ovmr_stream stream) {
    if (nseq < 0 || n_ctx < 0 || H < 1 || max_len < 1) return OVMR_E_ARG;
    // (no row count in this signature: the clamp bound is the most rows nseq sequences of max_len can be)
    return launch_attention_f32((const float*)qkv, (float*)out, AggSeqs{offsets_dev, 0, nseq, n_ctx, max_len, nseq * max_len}, H,
                                128, (hipStream_t)stream);
}

int ovmr_debug_attention_f32_long(const void* qkv, void* out, const int32_t* offsets_dev, int nseq, int n_ctx, int max_len, int H,
                                  ovmr_stream stream) {
    if (nseq < 0 || n_ctx < 0 || H < 1 || max_len < 1) return OVMR_E_ARG;
    if (max_len > OVMR_AGG_MAX_LEN_CEILING || (long)nseq * max_len > 0x7fffffffL) return -2;
    // uniform (offsets_dev == NULL): nseq sequences of max_len rows, n_ctx unused; table: the clamp bound as in the hook above
    return launch_attention_f32_long((const float*)qkv, (float*)out, AggSeqs{offsets_dev, 0, nseq, n_ctx, max_len, nseq * max_len}, H,
                                     (hipStream_t)stream);
}

int ovmr_debug_attention_q(int variant, const void* qkv, void* out, int B, int L, int Lq, int H, int causal,
                           ovmr_stream stream) {
    return launch_attention_f16_q((const half_t*)qkv, (half_t*)out, B, L, Lq, H, causal, variant, (hipStream_t)stream);
}

// The whole workspace arena set to one 32-bit pattern (tests/test_hip_poison.py): what a pass computes must not depend on what the
// arena held before it.  h->head_sync is NOT part of the arena and stays zero: a poisoned counter makes hf_wait spin forever.
int ovmr_debug_fill_workspace(ovmr_handle* h, uint32_t pattern, ovmr_stream stream) {
    if (!h) return OVMR_E_ARG;
    if (!h->finalized) return need_finalized(h);
    if (!h->ws || h->ws_bytes < 4) return 0;
    HIP_CHECK_RET(hipMemsetD32Async((hipDeviceptr_t)h->ws, (int)pattern, h->ws_bytes / 4, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
