// The linear probe's inner evaluation (include/ovmr_hip_probe.h; DESIGN.md sections 4 and 6): scores, and the loss terms and gradient of
// the softmax objective scikit-learn minimises behind lpclip/linear_probe.py of the reference.  Three launches per evaluation:
//
// 1. launch_gemm_f32 with EPI_BIAS (gemm_f32.hip): z = X W^T + b into the workspace, rows PR_LD(C) = ceil4(C) floats apart.
//
// 2. probe_residual_rows: one wave per row, four rows per workgroup.  Three sweeps of the row, lane l at columns l, l + 64, ...:
//    the maximum (and z[y], picked by COMPARING the column with the label); e = expf(z - max) stored in place and summed; then
//    r = (e * (1 / sum) - [c == y]) * inv_n in place, zeros in the pad columns [C, ceil4(C)).  row_loss = logf(sum) - (z[y] - max).
//    Lane sums run in column order and meet in wave_sum's butterfly: a fixed order.  A foreign label: zeros, loss 0.
//
// 3. probe_grad_tn<TM>: gW[c, d] (+)= sum_n r[n, c] x[n, d] on v_mfma_f32_16x16x4_f32, the contraction over the ROWS of both operands.
//    A workgroup owns TM classes x 64 features of gW and walks ALL rows in tiles of PR_ROWS = 32; four waves, 2 (classes) x 2 (features),
//    each TM / 2 x 32 = TM / 32 x 2 MFMA tiles.  Both operands are contiguous along their OUTPUT dimension, so the row tiles go to LDS as
//    they lie in memory, K-major [row][column] (16-byte loads and stores), and lane (r = l & 15, g = l >> 4) reads its operand of MFMA
//    step s at [4 s + g][m0 + r]: consecutive lanes, consecutive words, no transpose anywhere.  A pitch of 16 words mod 32 puts the rows
//    g and g + 1 of a 32-lane half on disjoint banks.  x is the MFMA's first operand, so a lane holds four consecutive FEATURES of one
//    class: 16-byte accesses to gW.  gb rides along in the workgroups of the first feature tile: one more MFMA per class fragment and
//    step whose first operand is 1.0f, fma(1, r, acc) being the plain sum.
//    The accumulator STARTS as l2 * W (accumulate == 0) or as what gW / gb hold (accumulate == 1), and the f32 MFMA is bit for bit an
//    fmaf chain in k order: every output element is ONE chain over the rows in their order, whichever tile shape computes it.  Hence no
//    split over rows, no atomics, and the call over [0, N) equals the call over [0, n1) continued over [n1, N) when n1 is a multiple of
//    PR_ROWS (a partial last tile is padded with zero operands, which a chain passes through unchanged only at its end).
//    Rows past N and columns past C or D are loaded as zeros (masked, not clamped) and never stored.
//    TM: 64, or 32 where 64 would leave fewer than PR_SMALL_GRID workgroups (1000 classes x 512 features: 128 against 256).
#include "../../include/ovmr_hip_probe.h"
#include "common.h"

#include <limits.h>
#include <string.h>

namespace {

constexpr int PR_ROWS = 32;                 // rows per K tile of probe_grad_tn: the row quantum
constexpr int PR_TD = 64;                   // features per workgroup
constexpr int PR_XP = PR_TD + 16;           // floats between two rows of the x tile in LDS
constexpr int PR_SMALL_GRID = 256;          // fewer 64-class tiles than this: 32-class tiles

__host__ __device__ inline long PR_LD(int C) { return ((long)C + 3) & ~3L; }

__global__ __launch_bounds__(256) void probe_residual_rows(float* __restrict__ Z, long ld, const int64_t* __restrict__ labels, int N, int C,
                                                           float inv_n, float* __restrict__ row_loss) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= N) return;                                            // (wave-uniform)
    float* z = Z + row * ld;
    const long label = (long)labels[row];
    if (label < 0 || label >= C) {                                   // (wave-uniform) a foreign label: the row counts for nothing
        for (long c = lane; c < ld; c += 64) z[c] = 0.f;
        if (lane == 0) row_loss[row] = 0.f;
        return;
    }
    float m = -INFINITY, zy = 0.f;
    for (long c = lane; c < C; c += 64) {
        const float v = z[c];
        m = fmaxf(m, v);
        if (c == label) zy = v;
    }
    m = wave_max(m);
    zy = wave_sum(zy);                                               // (one lane holds it, the others 0)
    float s = 0.f;
    for (long c = lane; c < C; c += 64) {
        const float e = expf(z[c] - m);
        z[c] = e;
        s += e;
    }
    s = wave_sum(s);
    const float inv = 1.0f / s;
    for (long c = lane; c < ld; c += 64) {
        float r = 0.f;
        if (c < C) {
            const float p = z[c] * inv;
            r = (c == label ? p - 1.0f : p) * inv_n;
        }
        z[c] = r;
    }
    if (lane == 0) row_loss[row] = logf(s) - (zy - m);
}

template <int TM>
__global__ __launch_bounds__(256) void probe_grad_tn(const float* __restrict__ R, long ldr, const float* __restrict__ X, long ldx, int N, int C,
                                                     int D, const float* __restrict__ W, float l2, int accumulate, float* __restrict__ gW,
                                                     float* __restrict__ gb) {
    constexpr int CF = TM / 32;                                      // class fragments of a wave
    constexpr int RP = TM + 16;                                      // floats between two rows of the residual tile in LDS
    constexpr int RC = TM / 4;                                       // 16-byte chunks of a residual tile row
    constexpr int RL = TM / 32;                                      // residual chunks a thread moves
    __shared__ __attribute__((aligned(16))) float sX[2][PR_ROWS * PR_XP];
    __shared__ __attribute__((aligned(16))) float sR[2][PR_ROWS * RP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wc = wave >> 1, wd = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;
    const int tiles_d = (D + PR_TD - 1) / PR_TD;
    const int tc = blockIdx.x / tiles_d, td = blockIdx.x - tc * tiles_d;
    const long c0 = (long)tc * TM;
    const int d0 = td * PR_TD;
    const bool with_bias = td == 0 && wd == 0;                       // (wave-uniform) these waves sum gb of their classes as well

    const float4_t zero = (float4_t){0.f, 0.f, 0.f, 0.f};
    float4_t rx[2], rr[RL];
    auto fetch = [&](int kt) {                                       // the row tile kt into registers: zeros outside [0, N) x [0, D) / [0, ldr)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i;
            const long n = (long)kt * PR_ROWS + (idx >> 4);
            const int d = d0 + ((idx & 15) << 2);
            rx[i] = (n < N && d < D) ? *(const float4_t*)(X + n * ldx + d) : zero;
        }
#pragma unroll
        for (int i = 0; i < RL; ++i) {
            const int idx = tid + 256 * i;
            const long n = (long)kt * PR_ROWS + idx / RC;
            const long c = c0 + ((idx % RC) << 2);
            rr[i] = (n < N && c < ldr) ? *(const float4_t*)(R + n * ldr + c) : zero;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i;
            *(float4_t*)(&sX[buf][(idx >> 4) * PR_XP + ((idx & 15) << 2)]) = rx[i];
        }
#pragma unroll
        for (int i = 0; i < RL; ++i) {
            const int idx = tid + 256 * i;
            *(float4_t*)(&sR[buf][(idx / RC) * RP + ((idx % RC) << 2)]) = rr[i];
        }
    };

    const int nk = (int)(((long)N + PR_ROWS - 1) / PR_ROWS);
    fetch(0);

    // the accumulators start as the value every chain continues from
    float4_t acc[CF][2], accb[CF];
#pragma unroll
    for (int i = 0; i < CF; ++i) {
        const long c = c0 + wc * (TM / 2) + i * 16 + fr;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int d = d0 + wd * 32 + j * 16 + fg * 4;
            acc[i][j] = zero;
            if (c < C && d < D) {
                if (accumulate) acc[i][j] = *(const float4_t*)(gW + c * D + d);
                else acc[i][j] = *(const float4_t*)(W + c * D + d) * l2;
            }
        }
        const float b0 = (with_bias && accumulate && c < C) ? gb[c] : 0.f;
        accb[i] = (float4_t){b0, b0, b0, b0};
    }
    stash(0);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) fetch(kt + 1);
#pragma unroll
        for (int s = 0; s < PR_ROWS / 4; ++s) {
            const int k = 4 * s + fg;
            float xa[2], ra[CF];
#pragma unroll
            for (int j = 0; j < 2; ++j) xa[j] = sX[cur][k * PR_XP + wd * 32 + j * 16 + fr];
#pragma unroll
            for (int i = 0; i < CF; ++i) ra[i] = sR[cur][k * RP + wc * (TM / 2) + i * 16 + fr];
#pragma unroll
            for (int i = 0; i < CF; ++i) {
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[j], ra[i], acc[i][j], 0, 0, 0);
                if (with_bias) accb[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, ra[i], accb[i], 0, 0, 0);
            }
        }
        if (more) stash(cur ^ 1);
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < CF; ++i) {
        const long c = c0 + wc * (TM / 2) + i * 16 + fr;
        if (c >= C) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int d = d0 + wd * 32 + j * 16 + fg * 4;
            if (d < D) *(float4_t*)(gW + c * D + d) = acc[i][j];
        }
        if (with_bias && fg == 0) gb[c] = accb[i][0];
    }
}

bool bad_probe_shape(int rows, int C, int D, long ldx) {
    return rows < 0 || C < 1 || D < 32 || (D % 32) != 0 || ldx < D || (ldx & 3) || ldx > INT_MAX;
}

int probe_gemm(const float* x, long ldx, int rows, const float* W, const float* b, int C, int D, float* out, long ldo, hipStream_t s) {
    GemmArgs a;
    memset(&a, 0, sizeof a);
    a.A = x; a.lda = (int)ldx; a.W = W; a.ldw = D; a.C = out; a.ldc = (int)ldo;
    a.M = rows; a.N = C; a.K = D; a.epi = EPI_BIAS; a.bias = b; a.scale = 1.f;
    return launch_gemm_f32(a, s);
}

}  // namespace

extern "C" {

int ovmr_probe_row_quantum(void) { return PR_ROWS; }

long ovmr_probe_workspace_bytes(int N, int C, int D) {
    if (N < 0 || C < 1 || D < 32 || (D % 32) != 0) return -1;
    return 4 * (long)N * PR_LD(C);
}

int ovmr_probe_logits(const float* x, long ldx, int B, const float* W, const float* b, int C, int D, float* out, long ldo,
                      ovmr_stream stream) {
    if (bad_probe_shape(B, C, D, ldx) || ldo < C || ldo > INT_MAX || !x || !W || !b || !out) return OVMR_E_ARG;
    if ((uintptr_t)x & 15 || (uintptr_t)W & 15 || (uintptr_t)b & 3 || (uintptr_t)out & 3) return OVMR_E_ARG;
    if (B == 0) return 0;
    return probe_gemm(x, ldx, B, W, b, C, D, out, ldo, (hipStream_t)stream);
}

int ovmr_probe_loss_grad(const float* x, long ldx, const int64_t* labels, int N, int C, int D, const float* W, const float* b, float inv_n,
                         float l2, int accumulate, float* workspace, float* row_loss, float* gW, float* gb, ovmr_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    if (bad_probe_shape(N, C, D, ldx) || (accumulate != 0 && accumulate != 1) || !W || !b || !gW || !gb) return OVMR_E_ARG;
    if (N > 0 && (!x || !labels || !workspace || !row_loss)) return OVMR_E_ARG;
    if ((uintptr_t)x & 15 || (uintptr_t)W & 15 || (uintptr_t)gW & 15 || (uintptr_t)workspace & 15) return OVMR_E_ARG;
    if ((uintptr_t)b & 3 || (uintptr_t)gb & 3 || (uintptr_t)row_loss & 3 || (uintptr_t)labels & 7) return OVMR_E_ARG;
    if (N == 0 && accumulate) return 0;
    const long ldr = PR_LD(C);
    if (ldr > INT_MAX) return OVMR_E_ARG;
    if (N > 0) {
        const int rc = probe_gemm(x, ldx, N, W, b, C, D, workspace, ldr, s);
        if (rc != 0) return rc;
        hipLaunchKernelGGL(probe_residual_rows, dim3((unsigned)(((long)N + 3) / 4)), dim3(256), 0, s, workspace, ldr, labels, N, C, inv_n,
                           row_loss);
        HIP_CHECK_RET(hipGetLastError());
    }
    const long tiles_d = (D + PR_TD - 1) / PR_TD;
    const long tiles64 = (((long)C + 63) / 64) * tiles_d;
    if (tiles64 < PR_SMALL_GRID)
        hipLaunchKernelGGL(probe_grad_tn<32>, dim3((unsigned)((((long)C + 31) / 32) * tiles_d)), dim3(256), 0, s, workspace, ldr, x, ldx, N, C, D,
                           W, l2, accumulate, gW, gb);
    else
        hipLaunchKernelGGL(probe_grad_tn<64>, dim3((unsigned)tiles64), dim3(256), 0, s, workspace, ldr, x, ldx, N, C, D, W, l2, accumulate, gW,
                           gb);
    return (int)hipGetLastError();
}

}  // extern "C"
