// Shared device/host helpers for the OVMR gfx950 kernels (wave64, MFMA 16x16x32 f16).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef _Float16 half_t;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef float float2_t __attribute__((ext_vector_type(2)));

#define OVMR_WAVE 64
#define OVMR_MAX_DEVICES 64

// GEMM epilogues (C = epi(A * W^T)), rounding points follow the reference's fp16 CPU path:
// every nn.Linear output is rounded to fp16 before the next elementwise op.
enum {
    EPI_NONE = 0,        // C = h(acc)
    EPI_BIAS = 1,        // C = h(acc + bias)                        nn.Linear            (clip/model.py:171,173-177)
    EPI_BIAS_QGELU = 2,  // u = h(acc+bias); C = u * sigmoid(1.702u) c_fc + QuickGELU     (clip/model.py:162-164)
    EPI_BIAS_RES = 3,    // C = h(h(acc+bias) + res)                 x + attn / x + mlp   (clip/model.py:192-193)
    EPI_PATCH = 4,       // C[b*Lout+1+p] = h(h(acc) + pos[1+p])     conv1 + pos add      (clip/model.py:412-416)
    EPI_SCALE = 5,       // C = h(h(acc) * scale)                    logit_scale * einsum (trainers/mm_classifier_one_prompt.py:263)
    // LayerNorm folded into the consuming nn.Linear (gemm_f16_v5 only).  A holds the RAW residual stream x, W holds
    // h(gamma (.) W), and the epilogue applies the row statistics:  LN(x) W^T + bias
    //   = rstd[m] * (acc[m,n] - mean[m] * ln_g[n]) + ln_b[n],  ln_g[n] = sum_k W'[n,k],  ln_b[n] = bias[n] + sum_k beta[k] W[n,k].
    // The reference rounds LN(x) to fp16 before the GEMM (clip/model.py:153-159); here the rounding sits on gamma (.) W
    // instead -- same magnitude of error, one full read + write of the activations less per LayerNorm.
    EPI_LN_BIAS = 6,        // C = h(LN-folded acc)                  ln_1 + in_proj       (clip/model.py:192)
    EPI_LN_BIAS_QGELU = 7,  // u = h(LN-folded acc); C = u * sigmoid(1.702u)   ln_2 + c_fc + QuickGELU (clip/model.py:193)
    // Cross-validation logits that are never written (gemm_f16_v5 only): u = h(h(acc) * scale) as EPI_SCALE, then per row
    // the (maximum, lowest column holding it) of the tile's 256 columns -> argmax_out[m][tn] = {max as float, column};
    // launch_argmax_reduce finishes the row argmax over the N tiles and counts.      (trainers/mm_classifier_one_prompt.py:263-270)
    EPI_SCALE_ARGMAX = 8,
};

struct GemmArgs {
    const void* A; int lda;     // [M,K] row-major
    const void* W; int ldw;     // [N,K] row-major (nn.Linear weight layout)
    void* C; int ldc;           // [M,N] row-major
    const void* bias;           // [N] or nullptr
    const void* res; int ldres; // [M,N] residual (may alias C) or nullptr
    const void* pos;            // EPI_PATCH: fp16 [Lout, N]
    int M, N, K;
    int epi;
    int rows_in, rows_out;      // EPI_PATCH: patches per image (G*G) and tokens per image (G*G+1)
    float scale;                // EPI_SCALE
    int n_group;                // N tiles per L2 group (tile order; launch_gemm_f16 fills it from the route's plan)
    // LayerNorm folding (see EPI_LN_BIAS).  Row statistics travel as per-row PARTIAL sums [M][slots][2] fp32
    // (sum, sum of squares), one slot per 256-column tile of the producing GEMM, summed in slot order by the consumer
    // (deterministic: no atomics).
    const float* ln_stats; int ln_slots;   // EPI_LN_*: statistics of the A rows over K
    int ln_stride;                         // ... slots between the statistics of consecutive A rows (0 = ln_slots: dense; the CLS-row launch strides over tokens)
    const float* ln_g; const float* ln_b;  // EPI_LN_*: [N] fp32 each
    float* stats_out;                      // EPI_BIAS_RES, optional: partial statistics of the stored C rows, [M][N/256][2]
    int persist;                           // the caller's "gemm_persist" option: gemm_f16_route may plan the tile loop (GemmPlan::persist); no kernel reads it
    float* argmax_out;                     // EPI_SCALE_ARGMAX: [M][ceil(N/256)][2] (value, column index bits)
    int gelu_mode;                         // QuickGELU epilogues: 0 = the reference's three fp16 rounding points, 1 = quick_gelu_f32x2
    // EPI_PATCH, gemm_f16_v5 only: A is the fp16 IMAGE tensor [B, 3, R, R] itself and the K loop gathers the patch rows
    // (k = c * 256 + ky * 16 + kx, 16 x 16 patches) straight into LDS -- no im2col pass.  0 = A is the [M, K] matrix.
    int im2col_R;
};

__device__ __forceinline__ float quick_gelu_h(float u) {
    // fp16 rounding points of `x * torch.sigmoid(1.702 * x)` on an fp16 tensor
    // (v_exp_f32 / v_rcp_f32 are 1-ulp fp32 approximations; their result is rounded to fp16 right away)
    half_t t = (half_t)(1.702f * u);
    half_t s = (half_t)__builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * (float)t));
    return (float)(half_t)(u * (float)s);
}

// The same rounding points on four fp16 values at a time (the epilogue's vector instructions are exposed time: nothing overlaps
// a tile's epilogue, profiles/r01g_gemm_epilogue.md).  The four denominators a b c d share ONE reciprocal, R = 1 / (abcd);
// 1/(ab) = cd R, 1/(cd) = ab R, 1/a = b / (ab) ...: 1.25 transcendental + 1.25 packed-fp32 multiplies per element instead of
// 1.5 + 1.5 (the transcendental unit is what bounds QuickGELU: quarter rate).  Exponent arguments are clamped at 30 (a sigmoid
// below 2^-25 rounds to fp16 zero either way), which keeps abcd below 2^124.
__device__ __forceinline__ half4_t quick_gelu_h4(half4_t u) {
    half4_t t;
    float4_t e;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t[k] = (half_t)(1.702f * (float)u[k]);
        e[k] = __builtin_amdgcn_exp2f(fminf(__builtin_fmaf((float)t[k], -1.4426950408889634f, 0.0f), 30.0f));
    }
    const float2_t p = (float2_t){e[0], e[2]} + 1.0f, q = (float2_t){e[1], e[3]} + 1.0f;
    const float2_t pq = p * q;                                     // (ab, cd)
    const float R = __builtin_amdgcn_rcpf(pq[0] * pq[1]);
    const float2_t rr = (float2_t){pq[1], pq[0]} * R;              // (1/(ab), 1/(cd))
    const float2_t sp = q * rr, sq = p * rr;                       // (1/a, 1/c), (1/b, 1/d)
    const half4_t s = __builtin_convertvector((float4_t){sp[0], sq[0], sp[1], sq[1]}, half4_t);
    return u * s;
}

// QuickGELU with ONE rounding point instead of the reference's three (ovmr_set_option "gelu_exact" = 0): the GEMM epilogue calls
// this on the fp32 value x = acc + bias BEFORE it is rounded to fp16 and rounds the product once, g = h(x / (1 + 2^(-1.702 log2(e) x)))
// -- v_mul_f32, v_exp_f32, v_add_f32, v_rcp_f32, v_mul_f32 at the full fp32 rate plus half a v_cvt_pk_f16_f32 per element, where
// quick_gelu_h4 takes a quarter-rate v_fma_mixlo_f16, 1.25 transcendentals and 5 more instructions (profiles/r03a_valu_rate.log: per SIMD
// with two waves, v_fma/mul/add_f32 2.6 cycles, other VOP3 4.4, transcendentals / v_fma_mixlo_f16 / v_permlane16_swap 8.3).  It is
// CLOSER to the real function than the reference's fp16 form (no h(u), h(1.702 u), h(sigmoid) in between); against the reference's
// result it differs by at most a few fp16 steps of the result (bound stated in tests/test_hip_kernels.py).  x < -52: e = +inf, s = 0, g = -0.
__device__ __forceinline__ float2_t quick_gelu_f32x2(float2_t x) {
    float2_t g;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float e = __builtin_amdgcn_exp2f(x[k] * -2.4554669595930157f);
        g[k] = x[k] * __builtin_amdgcn_rcpf(1.0f + e);
    }
    return g;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// The sequences of one fp32 aggregator pass (ovmr_generate_tokens, ovmr_generate_tokens_ragged): class c of the pass owns the rows
// [start(c), start(c + 1)) of the pass's M packed rows -- n_ctx cls_token rows, then its shots, the rows first_shot(c) ... of feats.
// The three kernels that read it (attn_f32_small, agg_input_kernel, agg_output_kernel) take the mode as a template parameter:
//   TABLE    `offsets` is a DEVICE exclusive prefix sum of the classes' shots, `base` its value at the pass's first class, `len` the
//            longest sequence.  A device array sets addresses, so every start is clamped to [0, M] (and the kernels clamp what they
//            build from it to `len` rows of LDS and the R rows of feats): offsets that disagree with the host's plan give wrong values,
//            never an access outside the buffers.
//   uniform  (offsets == nullptr) every class has len - n_ctx shots and `base` shots of the call lie before the pass: the arithmetic
//            mode of the same table, computed and never loaded -- the uniform call has no device array and may not make one.
struct AggSeqs {
    const int* offsets;
    int base, nseq, n_ctx, len, M;
    template <bool TABLE> __device__ __forceinline__ long start(int c) const {
        if (!TABLE) return (long)c * len;
        return min(max((long)offsets[c] - base + (long)c * n_ctx, 0L), (long)M);
    }
    template <bool TABLE> __device__ __forceinline__ long first_shot(int c) const {
        return TABLE ? (long)offsets[c] : base + (long)c * (len - n_ctx);
    }
};

#define HIP_CHECK_RET(expr)                                   \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) return (int)_e;                 \
    } while (0)

#include "launchers.h"   // last: the prototypes use the types above
