// fp16 MFMA GEMM for gfx950: C[M,N] = epi(A[M,K] * W[N,K]^T), fp32 accumulate.
//
// This one kernel family carries ~96 % of the hot path's FLOPs: patch embed (K1), QKV (K4),
// out-proj (K6), c_fc+QuickGELU (K7), c_proj (K8), the CLS/EOS projections (K9,K15) and the
// classifier logits (K18,K21) of SURVEY.md section 2.3.
//
// Which kernel of the family a launch runs is decided in ONE place, gemm_f16_route at the end of this file (gemm_route.h: the plan).
//
// This file's kernel ("t128", all of variant 0): 128x128x64 tile, 4 waves (2x2), each wave 64x64 = 4x4 MFMA 16x16x32 f16
// tiles; operands staged global -> registers -> LDS (double buffered, XOR-swizzled 128-byte
// rows so every ds_read_b128 lane group hits 16 distinct 16-byte slots).
// The MFMA is issued with W as the A operand and A as the B operand, so the accumulator holds
// C^T: lane l owns row m = l&15 and four CONSECUTIVE columns n = 4*(l>>4)..+3, which turns the
// epilogue (bias / residual / QuickGELU / positional add) into 8-byte vector loads and stores.
#include <string.h>

#include "gemm_epi.h"
#include "gemm_route.h"

namespace {

constexpr int BK = 64;

// ------------------------------------------------------------------------------------------
// 128x128x64, register-staged double buffer.
template <int EPI>
__global__ __launch_bounds__(256) void gemm_f16_t128(GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* sA = (half_t*)smem;               // [2][128*64]
    half_t* sB = sA + 2 * 128 * BK;           // [2][128*64]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_n = (a.N + 127) >> 7;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm << 7, n0 = tn << 7;

    const half_t* A = (const half_t*)a.A;
    const half_t* W = (const half_t*)a.W;

    // staging map: 16-byte chunk id = tid + 256*i -> row = id>>3 (0..127), chunk = id&7
    const int lc = tid & 7, lr = tid >> 3;
    const int sw = ((lc ^ (lr & 7)) << 3);
    const half_t* ga[4];
    const half_t* gb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int r = lr + 32 * i;
        int ma = min(m0 + r, a.M - 1), nb = min(n0 + r, a.N - 1);
        ga[i] = A + (long)ma * a.lda + lc * 8;
        gb[i] = W + (long)nb * a.ldw + lc * 8;
    }
    uint4 ra[4], rb[4];
    const int nk = a.K / BK;

#pragma unroll
    for (int i = 0; i < 4; ++i) { ra[i] = *(const uint4*)ga[i]; rb[i] = *(const uint4*)gb[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        *(uint4*)(sA + (lr + 32 * i) * BK + sw) = ra[i];
        *(uint4*)(sB + (lr + 32 * i) * BK + sw) = rb[i];
    }
    __syncthreads();

    float4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fg = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = (kt + 1 < nk);
        if (more) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ra[i] = *(const uint4*)(ga[i] + (long)(kt + 1) * BK);
                rb[i] = *(const uint4*)(gb[i] + (long)(kt + 1) * BK);
            }
        }
        const half_t* cA = sA + cur * 128 * BK;
        const half_t* cB = sB + cur * 128 * BK;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            half8_t fa[4], fb[4];
            const int ch = (((ks << 2) + fg) ^ (fr & 7)) << 3;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                fa[t] = *(const half8_t*)(cA + (wm * 64 + t * 16 + fr) * BK + ch);
                fb[t] = *(const half8_t*)(cB + (wn * 64 + t * 16 + fr) * BK + ch);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
        if (more) {
            half_t* nA = sA + (cur ^ 1) * 128 * BK;
            half_t* nB = sB + (cur ^ 1) * 128 * BK;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *(uint4*)(nA + (lr + 32 * i) * BK + sw) = ra[i];
                *(uint4*)(nB + (lr + 32 * i) * BK + sw) = rb[i];
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            epilogue_store<EPI>(a, m0 + wm * 64 + i * 16 + fr, n0 + wn * 64 + j * 16 + fg * 4, acc[i][j]);
}

template <int EPI>
int launch_t128(const GemmArgs& a, hipStream_t s) {
    const int tiles = ((a.M + 127) / 128) * ((a.N + 127) / 128);
    const size_t lds = 2 * 2 * 128 * BK * sizeof(half_t);
    static bool attr_set[OVMR_MAX_DEVICES] = {};      // the attribute is per device (one process may drive several)
    int dev = 0;
    HIP_CHECK_RET(hipGetDevice(&dev));
    if (dev >= 0 && dev < OVMR_MAX_DEVICES && !attr_set[dev]) {
        HIP_CHECK_RET(hipFuncSetAttribute((const void*)gemm_f16_t128<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[dev] = true;
    }
    hipLaunchKernelGGL(gemm_f16_t128<EPI>, dim3(tiles), dim3(256), lds, s, a);
    return (int)hipGetLastError();
}

// Shapes that are at most ONE round of 64 x 64 tiles on the 256 CUs: there the K loop of a tile kernel runs at one memory latency
// per K-tile on a mostly idle machine and the split-K kernel (gemm_f16_small.hip) wins -- 8-9 us against 10-14 us at K = 512,
// 20 against 28 at K = 2048, 27 against 43 at K = 3072, 3-5x at a few dozen rows; beyond one round its missing operand reuse costs
// more than the latency it hides (profiles/r04d_small_gemm_bench.log: the rule matches the faster kernel on all 81 measured shapes
// but the two within 5 %).
bool one_round_of_s64(int M, int N) { return (long)((M + 63) / 64) * ((N + 63) / 64) <= 256; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// GEMM_TILE: tile height, K loop, cache hints and tile order.  ping_pong: the variant asks for the ping-pong loop and K is a whole
// number of its two-K-tile iterations.
void plan_tile(const GemmArgs& a, bool ping_pong, GemmPlan& p) {
    const int tiles_n = (a.N + 255) / 256;
    const double t256 = (double)((a.M + 255) / 256) * tiles_n, t128 = (double)((a.M + 127) / 128) * tiles_n;
    auto rounds = [](double t) { return ceil(t / 256.0); };                   // of the 256 CUs
    auto eff = [&](double t) { return t / (rounds(t) * 256.0); };
    // Ping-pong K loop on 256-row tiles against the double-buffered loop on 128-row tiles: a round of 128-row tiles takes ~0.74 of a
    // round of 256-row tiles (r02d, batch 256: out_proj 19.8 vs 26.6 us, c_proj 59 vs 78 us per round), so the big tile wins unless the
    // small one saves a whole round -- e.g. 591 tiles (batch 256, N = 768): 3 rounds against 5 x 0.74; the CLS-only tail (6 tiles)
    // stays on 128-row tiles.  Without the ping-pong loop: grids far below one round of CUs (the CLS-only tail of the last vision
    // block: 512 rows): the smaller tile doubles the workgroups and shortens each K-tile (out_proj 22.5 -> 14.0 us, c_proj 67.7 -> 42.6
    // us at 512 rows).
    const bool big = ping_pong ? rounds(t256) <= 0.74 * rounds(t128) : t256 >= 64 && eff(t256) + 0.08 >= eff(t128);
    // (r02q, measured and removed: running the rows beyond the last whole round of 256-row tiles as a second launch of 128-row
    // tiles -- batch-256 inference, N = 768: 2.31 rounds -> 2 + 0.78 -- took 6 % off out_proj (81 -> 76 us) but added 2 % to
    // c_proj (K = 3072: the small-tile round is no shorter there); 0.1 % of a step.)
    p.tile_rows = big ? 256 : 128;
    const int tiles = (int)(big ? t256 : t128);
    const bool res = a.epi == EPI_BIAS_RES, lnf = a.epi == EPI_LN_BIAS || a.epi == EPI_LN_BIAS_QGELU;
    // The ping-pong loop exists for 256-row tiles only.  Where it does not run: the loop with the iteration boundary inside the MFMA
    // stream for the LayerNorm-folding launches (qkv_ln 354 -> 343 us, c_fc_ln 525 -> 518 us; the plain bias / QuickGELU launches of
    // the same shapes do not gain) and for the residual projections with K >= 2048 (c_proj 467 -> 449 us; at K = 768, 12 K-tiles, it
    // is neutral to 2 % slower); the double-buffered loop otherwise.
    p.loop = ping_pong && big ? LOOP_PINGPONG : (lnf || (res && a.K >= 2048)) ? LOOP_BOUNDARY : LOOP_DOUBLE;
    // Residual projections with N <= 1024 (at most four N tiles share an A panel): the A stream is loaded with the nontemporal policy
    // so that it does not push the W panels every tile re-reads out of the L2 (out_proj 146 -> 141 us, c_proj 477 -> 459 us).  With
    // 9-12 N tiles per A panel the same hint costs 6-11 %, and on the W operand it always costs.
    p.a_nt = res && tiles_n <= 4 && tiles >= 512;
    // C written with the nontemporal hint does not evict the A / W panels the other tiles of the XCD are streaming from its 4 MiB L2
    // (profiles/r01g_gemm_epilogue.md).  Not for the in-place residual updates (out_proj / c_proj: +4 % slower) nor for small outputs
    // the next kernel reads straight back (logits for the argmax); the fused argmax stores no C at all.
    p.nt_store = !res && a.epi != EPI_SCALE_ARGMAX && (size_t)a.M * a.N * 2 >= ((size_t)48 << 20);
    // Tile order.  Measured (profiles/r01e_gemm_experiments.md): groups of 4-6 N tiles raise the L2 hit rate of qkv / c_fc from
    // 65-68 % to 72-73 % but move the run time by < 2 %, and hurt c_proj: the order stays row-major (all N tiles in one group) --
    // but with the ping-pong K loop (r02c, same-process A/B at batch 512) groups of 4 from 8 N tiles on take 1.5-2.5 % off qkv / c_fc
    // (c_fc_ln 496 -> 484 us, qkv_ln 329 -> 325 us), nothing off the N = 768 shapes
    p.n_group = p.loop == LOOP_PINGPONG && tiles_n >= 8 ? 4 : tiles_n;
    // The tile loop (gemm_f16_v5.hip, "Tile loop": one workgroup per CU walks the tiles, the next tile's operands in flight under a
    // tile's epilogue) exists for the LayerNorm-folding ping-pong kernels; it is planned where the caller's option asks for it and
    // the launch has more tiles than the 256 CUs.  Measurements: DESIGN.md section 4.
    p.persist = a.persist && lnf && p.loop == LOOP_PINGPONG && tiles > 256;
}

}  // namespace

bool gemm_f16_latency_bound(int variant, int M, int N) { return variant == 8 && one_round_of_s64(M, N); }
int gemm_f16_pinned_variant(int variant, int M, int N) { return variant != 8 ? variant : one_round_of_s64(M, N) ? 9 : 7; }

// Which kernel runs a GEMM, by variant (+ 100: the one-rounding QuickGELU, common.h quick_gelu_f32x2; the engine sets
// GemmArgs::gelu_mode itself):
//   0            the 128 x 128 register-staged kernel above for every shape;
//   6            256-row tiles (gemm_f16_v5.hip) with the double-buffered K loop;
//   8 (default)  256-row tiles with the ping-pong K loop, and the 64 x 64 split-K kernel (gemm_f16_small.hip) for latency-bound
//                shapes (one_round_of_s64);
//   7            8 without the split-K kernel; 9: the split-K kernel wherever it takes the shape (both: tests, and the engine's
//                K/V + Q launches, gemm_f16_pinned_variant).
// The first kernel that takes the shape runs: split-K (K a multiple of 128, no positional add) -> 256-row (M >= 256, N >= 128,
// 16-byte rows, 31-bit operand offsets) -> 128 x 128.  What only the 256-row kernel does -- patch rows gathered from the image, the
// fused row argmax, the LayerNorm fold and its statistics -- runs there under every variant (0 / 7 / 9: with the loop of 8), and
// is -4 on a shape it does not take.  -2: K, a stride or a tile-only feature's operands; -5: a variant without a K loop; -3: epilogue.
GemmPlan gemm_f16_route(const GemmArgs& a, int variant) {
    GemmPlan p = {};
    auto run = [&p](int kernel, int rc = 0) { p.kernel = kernel; p.rc = rc; return p; };
    auto none = [&run](int rc) { return run(GEMM_NONE, rc); };
    const bool lnf = a.epi == EPI_LN_BIAS || a.epi == EPI_LN_BIAS_QGELU, res = a.epi == EPI_BIAS_RES, argmax = a.epi == EPI_SCALE_ARGMAX;
    if (a.epi == EPI_BIAS_QGELU || a.epi == EPI_LN_BIAS_QGELU) p.gelu_mode = variant >= 100 ? variant / 100 : a.gelu_mode;
    if (variant >= 100) variant %= 100;
    if (a.M <= 0 || a.N <= 0) return none(0);
    if (a.K <= 0 || (a.K % BK) != 0 || (a.lda & 7) || (a.ldw & 7)) return none(-2);  // caller pads K to 64
    const bool tile_only = a.im2col_R || argmax || lnf || a.stats_out;
    if (!tile_only && (variant == 9 || gemm_f16_latency_bound(variant, a.M, a.N)) && (a.K % 128) == 0 && aligned16(a.A) && aligned16(a.W) && a.epi != EPI_PATCH &&
        a.epi >= EPI_NONE && a.epi <= EPI_SCALE) {
        const int steps = a.K >> 7, tiles = ((a.M + 63) >> 6) * ((a.N + 63) >> 6);      // K-steps of 32 per wave; workgroups
        // D = 4 (32 loads in flight per lane, 284 registers: one wave per SIMD) while the grid leaves at most one workgroup per CU
        // anyway (the shapes variant 8 sends here); larger grids (variant 9 in the tests) keep two workgroups per CU resident (D <= 3)
        p.depth = steps % 4 == 0 && tiles <= 256 ? 4 : steps % 3 == 0 ? 3 : steps % 2 == 0 ? 2 : 1;
        p.groups = steps / p.depth;
        return run(GEMM_S64);
    }
    const bool takes = a.M >= 256 && a.N >= 128 && (long)a.M * a.lda * 2 < 0x7fffffffL && (long)a.N * a.ldw * 2 < 0x7fffffffL &&
                       (argmax ? a.argmax_out != nullptr
                               : !(a.N & 7) && !(a.ldc & 7) && aligned16(a.C) && (!res || (!(a.ldres & 7) && aligned16(a.res))));
    if ((tile_only || variant >= 1) && takes) {
        // A = fp16 images [B, 3, R, R], 16 x 16 patches: K = 768.  The images' bytes stay below 2^31 like every other operand's: an
        // image is rows_in * 768 * 2 bytes, so for whole images `takes` (M * lda * 2 with lda = 768) holds that already and a higher
        // bound here never admitted anything; this one counts a last, partly used image whole.
        if (a.im2col_R) {
            const int G = a.im2col_R >> 4;
            if (a.epi != EPI_PATCH || a.K != 768 || (a.im2col_R & 15) || a.rows_in != G * G || !aligned16(a.A) ||
                (long)((a.M + a.rows_in - 1) / a.rows_in) * 3 * a.im2col_R * a.im2col_R * 2 >= 0x7fffffffL)
                return none(-2);
        }
        if (lnf && ((a.N & 63) || !a.ln_stats || a.ln_slots < 1 || !a.ln_g || !a.ln_b)) return none(-2);
        if (a.stats_out && (!res || (a.N & 255))) return none(-2);
        const int loop = (variant == 0 || variant == 7 || variant == 9) ? 8 : variant;   // K loop of the 256-row kernel
        if (loop != 6 && loop != 8) return none(-5);
        if (a.epi < EPI_NONE || a.epi > EPI_SCALE_ARGMAX) return none(-3);
        plan_tile(a, loop == 8 && (a.K % 128) == 0, p);   // ping-pong K loop: two K-tiles per iteration
        return run(GEMM_TILE);
    }
    if (tile_only) return none(-4);
    if (a.epi < EPI_NONE || a.epi > EPI_SCALE) return none(-3);
    return run(GEMM_T128);
}

// The route for a launch with 16-byte-aligned operands, lda = ldw = K and every operand a tile-only feature needs present (no GPU).
// im2col: the image side R, 0 = none; persist: the caller's "gemm_persist" option.  out[11]: the GemmPlan, field by field.
extern "C" int ovmr_debug_gemm_plan(int variant, int M, int N, int K, int epi, int ldc, int ldres, int stats, int im2col, int persist, int* out) {
    static float operand[4];
    alignas(16) static char base[16];
    GemmArgs a = {};
    a.M = M; a.N = N; a.K = a.lda = a.ldw = K; a.epi = epi; a.ldc = ldc; a.ldres = ldres;
    a.A = a.W = a.res = base; a.C = base;
    a.ln_stats = a.ln_g = a.ln_b = operand; a.ln_slots = 1; a.argmax_out = operand; a.stats_out = stats ? operand : nullptr;
    a.im2col_R = im2col; a.rows_in = (im2col >> 4) * (im2col >> 4); a.rows_out = a.rows_in + 1;
    a.persist = persist;
    static_assert(sizeof(GemmPlan) == 11 * sizeof(int), "");
    *(GemmPlan*)out = gemm_f16_route(a, variant);
    return 0;
}

// ... with the option off; out[10]: the plan's first ten fields (include/ovmr_hip.h)
extern "C" int ovmr_debug_gemm_route(int variant, int M, int N, int K, int epi, int ldc, int ldres, int stats, int im2col, int* out) {
    int plan[11];
    const int rc = ovmr_debug_gemm_plan(variant, M, N, K, epi, ldc, ldres, stats, im2col, 0, plan);
    memcpy(out, plan, 10 * sizeof(int));
    return rc;
}

// A LayerNorm-folding GEMM (epi 6 / 7) with the tile loop chosen by the caller: persist = the "gemm_persist" option of the launch.
// max_wgs > 0 (tests/test_hip_gemm_persist.py): the launch runs the 256-row ping-pong tile kernel whatever the route says of the
// shape, as a tile loop of at most max_wgs workgroups -- so that a shape of a few tiles drives the loop; max_wgs >= the number of
// tiles is the one-tile-per-workgroup form.  A [M, lda], W [N, K], C [M, ldc]; ln_stats [.., ln_slots, 2] with ln_stride slots between
// the statistics of consecutive A rows (0: dense).
extern "C" int ovmr_debug_gemm_persist(int variant, const void* A, int lda, const void* W, const float* ln_b, const float* ln_stats, int ln_slots,
                                       int ln_stride, const float* ln_g, void* C, int ldc, int M, int N, int K, int epi, int persist, int max_wgs,
                                       void* stream) {
    if (epi != EPI_LN_BIAS && epi != EPI_LN_BIAS_QGELU) return -1;
    if (!A || !W || !ln_b || !ln_stats || !ln_g || !C || max_wgs < 0) return -1;
    GemmArgs a = {};
    a.A = A; a.lda = lda; a.W = W; a.ldw = K; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.epi = epi; a.scale = 1.f;
    a.ln_stats = ln_stats; a.ln_slots = ln_slots; a.ln_stride = ln_stride; a.ln_g = ln_g; a.ln_b = ln_b;
    a.persist = persist;
    if (!max_wgs) return launch_gemm_f16(a, variant, (hipStream_t)stream);
    GemmPlan p = gemm_f16_route(a, variant);
    if (p.kernel != GEMM_TILE) return p.kernel == GEMM_NONE ? p.rc : -4;
    if (K % 128) return -2;                                      // the ping-pong loop: two K-tiles per iteration
    const int tiles_n = (N + 255) / 256;
    p.tile_rows = 256; p.loop = LOOP_PINGPONG; p.a_nt = 0; p.n_group = tiles_n >= 8 ? 4 : tiles_n; p.persist = 1;
    a.n_group = p.n_group;
    a.gelu_mode = p.gelu_mode;
    return launch_gemm_f16_v5(a, p, (hipStream_t)stream, max_wgs);
}

int launch_gemm_f16(const GemmArgs& a_in, int variant, hipStream_t s) {
    const GemmPlan p = gemm_f16_route(a_in, variant);
    GemmArgs a = a_in;
    a.n_group = p.n_group;
    a.gelu_mode = p.gelu_mode;
    switch (p.kernel) {
        case GEMM_T128:
#define X(E) if (a.epi == E) return launch_t128<E>(a, s);
            X(EPI_NONE) X(EPI_BIAS) X(EPI_BIAS_QGELU) X(EPI_BIAS_RES) X(EPI_PATCH) X(EPI_SCALE)
#undef X
            return -3;
        case GEMM_S64: return launch_gemm_f16_small(a, p, s);
        case GEMM_TILE: return launch_gemm_f16_v5(a, p, s);
    }
    return p.rc;
}
