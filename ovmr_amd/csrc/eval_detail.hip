// The evaluator's detail mode: everything Classification.process counts for one test batch, in ONE launch
// (Dassl.pytorch/dassl/evaluation/evaluator.py:50-73 -- pred / top-k matches, _y_true / _y_pred, _per_class_res -- and what :140-171
// make of them: the per-class block and the confusion matrix).  Per row: the selection rounds of topk.hip (eval_common.h) in the
// library's total order; round 0 is the prediction -- the argmax eval_counts_kernel takes -- and the rounds stop at the label's
// column, so a row whose label is its prediction costs one pass like eval_counts_kernel.  Then, per row with a label in [0, C):
//     counts (tp, n_pred, n_label, as eval_counts_kernel)      hits += label among the k columns      class_hits[label] += the same
//     cmat[label][pred] += 1 (64-bit cell index)
//
// One wave per row, SIXTEEN rows per 1024-thread workgroup: a test pass lists the split class folder by class folder, so the rows of a
// batch mostly share one label and one (label, pred) cell, and same-address atomics serialise (eval_common.h).  One wave per output
// buffer counts all sixteen rows with wave_histogram_add: at most one atomic per distinct address, buffer and workgroup -- 16 workgroups
// for a batch of 256 rows, a quarter of what four rows per block would send to the one hot address -- while a row still has a wave to
// itself, so the latency of a row is that of eval_counts_kernel / topk_rows_kernel.
#include "common.h"
#include "eval_common.h"

namespace {

constexpr int ROWS = 16;   // rows (= waves) per workgroup

template <typename T>
__global__ __launch_bounds__(64 * ROWS) void eval_detail_kernel(const T* __restrict__ out, long ld, const int64_t* __restrict__ labels,
                                                                 int rows, int C, int k, int* __restrict__ counts,
                                                                 int* __restrict__ hits, int* __restrict__ class_hits,
                                                                 int* __restrict__ cmat) {
    __shared__ int pred_s[ROWS], gt_s[ROWS], hit_s[ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * ROWS + wave;
    int pred = -1, g = -1;                                           // g: the label, -2 outside [0, C), -1 no row
    bool hit = false;
    if (row < rows) {                                                // (wave-uniform)
        const int64_t lab = labels[row];
        g = (lab >= 0 && lab < C) ? (int)lab : -2;
        if (g >= 0) {                                                // a row with a label outside [0, C) touches slot 3C only
            const T* r = out + (long)row * ld;
            const int rounds = (hits || class_hits) ? k : 1;
            unsigned long long limit = ~0ull;
            for (int j = 0; j < rounds && !hit; ++j) {
                const unsigned long long win = topk_round(r, C, lane, limit);   // never 0: k <= C and the keys of a row are distinct
                const int c = (int)(0xFFFFFFFFu - (unsigned)win);
                if (j == 0) pred = c;
                hit = c == g;
                limit = win - 1;
            }
        }
    }
    if (lane == 0) { pred_s[wave] = pred; gt_s[wave] = g; hit_s[wave] = hit ? 1 : 0; }
    __syncthreads();
    // the seven histograms go out from seven waves, one each: a wave sends its atomics one distinct address after the other
    // (wave_histogram_add), and with random labels sixteen rows are up to sixteen addresses per buffer
    if (wave < 7) {                                                  // (wave-uniform; the workgroup has ROWS = 16 waves)
        const int p = lane < ROWS ? pred_s[lane] : -1;
        g = lane < ROWS ? gt_s[lane] : -1;
        const bool live = g >= 0, h = live && hit_s[lane < ROWS ? lane : 0] != 0;
        switch (wave) {
            case 0: wave_histogram_add(counts + 2 * C, g, live); break;              // n_label
            case 1: wave_histogram_add(counts + C, p, live); break;                  // n_pred
            case 2: wave_histogram_add(counts, p, live && p == g); break;            // tp
            case 3: wave_histogram_add(counts + 3 * C, 0, g == -2); break;           // labels outside [0, C)
            case 4: if (hits) wave_histogram_add(hits, 0, h); break;
            case 5: if (class_hits) wave_histogram_add(class_hits, g, h); break;
            default: if (cmat) wave_histogram_add(cmat, (long)g * C + p, live); break;
        }
    }
}

}  // namespace

int launch_eval_detail(const void* out, int out_is_f32, long ld, const int64_t* labels, int B, int C, int k, int* counts, int* hits,
                       int* class_hits, int* cmat, hipStream_t s) {
    if (B <= 0) return 0;
    const dim3 grid((B + ROWS - 1) / ROWS), block(64 * ROWS);
    if (out_is_f32)
        hipLaunchKernelGGL(eval_detail_kernel<float>, grid, block, 0, s, (const float*)out, ld, labels, B, C, k, counts, hits, class_hits, cmat);
    else
        hipLaunchKernelGGL(eval_detail_kernel<half_t>, grid, block, 0, s, (const half_t*)out, ld, labels, B, C, k, counts, hits, class_hits, cmat);
    return (int)hipGetLastError();
}
