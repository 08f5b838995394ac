// What the evaluator's kernels share (fusion_head.hip: xval_argmax_reduce, eval_counts_kernel; topk.hip: topk_rows_kernel;
// eval_detail.hip: eval_detail_kernel): the selection key and round of the library's total order, and the wave-aggregated histogram update.
#pragma once
#include "common.h"

namespace {

// v of lane `lane`, for all lanes
__device__ __forceinline__ int wave_read(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ long wave_read(long v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)v, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), lane);
    return (long)(((unsigned long long)hi << 32) | lo);
}
// counts[key] += 1 for every lane with valid set, ONE atomic per distinct key and wave: the argmax of exemplar rows concentrates on few
// classes (always with untrained weights, per class with trained ones: S consecutive rows share their label), and same-address atomics
// serialise -- 16 000 rows on a handful of classes took 155 us (r04o trace), most of the cross-validation step.
template <typename K>   // int, or long where the histogram has more than 2^31 cells (the confusion matrix)
__device__ __forceinline__ void wave_histogram_add(int* counts, K key, bool valid) {
    unsigned long long todo = __builtin_amdgcn_ballot_w64(valid);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const K k = wave_read(key, leader);
        const unsigned long long same = __builtin_amdgcn_ballot_w64(valid && key == k);
        if (lane == leader) atomicAdd(counts + k, (int)__builtin_popcountll(same));
        todo &= ~same;
    }
}

__device__ __forceinline__ unsigned long long topk_key(float v, int c) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0;                                     // -0 == +0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                  // negative values reversed below the positive ones: -inf -> 0x007FFFFF, +inf -> 0xFF800000
    if (v != v) u = 0xFFFFFFFFu;                                     // every NaN, of either sign: above +inf
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c);
}

// the largest key <= limit of the row (0: none left; a real key is at least 0x007FFFFF << 32)
template <typename T>
__device__ __forceinline__ unsigned long long topk_round(const T* __restrict__ row, int C, int lane, unsigned long long limit) {
    unsigned long long best = 0;
    auto take = [&](float v, int c) {
        const unsigned long long key = topk_key(v, c);
        if (key <= limit && key > best) best = key;
    };
    constexpr int V = 16 / (int)sizeof(T);
    if ((((uintptr_t)row) & 15) == 0) {
        const int Cv = C / V * V;
        for (int c = lane * V; c < Cv; c += 64 * V) {
            if constexpr (sizeof(T) == 4) {
                const float4 q = *(const float4*)(row + c);
                take(q.x, c); take(q.y, c + 1); take(q.z, c + 2); take(q.w, c + 3);
            } else {
                const uint4 q = *(const uint4*)(row + c);
                const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    half2_t h2 = *(const half2_t*)&u[i];
                    take((float)h2[0], c + 2 * i); take((float)h2[1], c + 2 * i + 1);
                }
            }
        }
        for (int c = Cv + lane; c < C; c += 64) take((float)row[c], c);
    } else
        for (int c = lane; c < C; c += 64) take((float)row[c], c);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(best >> 32), o, 64), lo = __shfl_xor((unsigned)best, o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        if (other > best) best = other;
    }
    return best;
}

}  // namespace
