// Ranked prediction: the k best columns of every row of a [B, C] output matrix, best first -- Classification.process(topk > 1)
// (Dassl.pytorch/dassl/evaluation/evaluator.py:56-58: output.topk(max(topk), 1, True, True)) and the predict_topk methods of ovmr_amd/modules.py.
// The order is TOTAL (torch.sort(descending=True, stable=True) on the host): larger value first, equal values in increasing column order,
// every NaN above +inf (NaNs among themselves by column), -0 == +0.  Column 0 of the result is the row argmax of eval_counts_kernel
// (fusion_head.hip).
//
// One wave per row, four rows per 256-thread block, k selection rounds (topk_key / topk_round, eval_common.h: shared with
// eval_detail.hip).  An element maps to a 64-bit key
//     (order-preserving bits of the value: NaN -> 0xFFFFFFFF, -0 -> +0) << 32 | (0xFFFFFFFF - column)
// so that "better" is "larger key" and no two elements of a row share a key.  Round j takes the largest key at or below `limit` = the
// previous winner's key - 1: every lane scans its columns (16-byte loads where the row is aligned), the wave reduces by shuffles.  A row
// is at most 87 KB (21 841 fp32 classes): rounds 1 .. k-1 re-read it from L2.  The kernel is latency-bound.
#include "common.h"
#include "eval_common.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void topk_rows_kernel(const T* __restrict__ out, long ld, int rows, int C, int k,
                                                        float* __restrict__ values, int32_t* __restrict__ indices,
                                                        const int64_t* __restrict__ labels, int* __restrict__ hits) {
    __shared__ int hit_s[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    bool hit = false;
    if (row < rows) {                                                // (wave-uniform)
        const T* r = out + (long)row * ld;
        unsigned long long limit = ~0ull;
        int mine = -1;                                               // lane j keeps the column of rank j (k <= 32)
        for (int j = 0; j < k; ++j) {
            const unsigned long long win = topk_round(r, C, lane, limit);   // never 0: k <= C and the keys of a row are distinct
            if (lane == j) mine = (int)(0xFFFFFFFFu - (unsigned)win);
            limit = win - 1;
        }
        if (lane < k) {
            indices[(long)row * k + lane] = mine;
            if (values) values[(long)row * k + lane] = (float)r[mine];      // the element itself: a NaN stays a NaN, -0 keeps its sign
        }
        if (labels) hit = __builtin_amdgcn_ballot_w64(lane < k && (int64_t)mine == labels[row]) != 0;   // a label outside [0, C) equals no column
    }
    if (!hits) return;                                               // (uniform over the block)
    if (lane == 0) hit_s[wave] = hit ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) {                                          // the block's rows with ONE atomic
        const int n = hit_s[0] + hit_s[1] + hit_s[2] + hit_s[3];
        if (n) atomicAdd(hits, n);
    }
}

}  // namespace

int launch_topk_rows(const void* out, int out_is_f32, long ld, int B, int C, int k, float* values, int32_t* indices,
                     const int64_t* labels, int* hits, hipStream_t s) {
    if (B <= 0) return 0;
    if (out_is_f32)
        hipLaunchKernelGGL(topk_rows_kernel<float>, dim3((B + 3) / 4), dim3(256), 0, s, (const float*)out, ld, B, C, k, values, indices, labels, hits);
    else
        hipLaunchKernelGGL(topk_rows_kernel<half_t>, dim3((B + 3) / 4), dim3(256), 0, s, (const half_t*)out, ld, B, C, k, values, indices, labels, hits);
    return (int)hipGetLastError();
}
