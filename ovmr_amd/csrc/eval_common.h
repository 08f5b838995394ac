// What the evaluator's kernels share (fusion_head.hip: xval_argmax_reduce, eval_counts_kernel; topk.hip: topk_rows_kernel;
// eval_detail.hip: eval_detail_kernel): the selection key and round of the library's total order, and the wave-aggregated histogram update;
// and what the kernels that work along the COLUMNS of a [B, C] output share (retrieve.hip, eval_curves.hip): the launchers' test of that
// matrix and the transposed tile load.
#pragma once
#include "common.h"

namespace {

// out [B, C], rows ld elements apart, as ovmr_retrieve_update and ovmr_eval_curves take it: there, rows at least C apart, element-aligned
inline bool bad_out_matrix(const void* out, int out_is_f32, long ld, int C) {
    return !out || ld < C || (uintptr_t)out & (out_is_f32 ? 3 : 1);
}

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

// The [ROWS rows][TILE classes] corner at (r0, c0) of out [B, C] (TILE at least a 16-byte vector wide), loaded along the rows -- 16-byte
// loads where the address is aligned and the vector lies within the C classes, element loads otherwise (C odd: every second fp16 row)
// -- and written TRANSPOSED to LDS as fp32, tile[class][row], rows past B and classes past C as zeros; the caller's barrier follows.
// PITCH = 66 floats between two classes for ROWS = 64: ds_write_b32 and ds_read_b32 bank by (address / 4) mod 32 over groups of 32
// lanes; the 32 lanes of a store group hold 16 rows x 2 vectors (fp16) or 8 rows x 4 vectors (fp32) and element e of every vector goes
// out in one store: bank = (2 class + row) mod 32 is distinct over the group; a reader with lane = row walks consecutive addresses.
template <typename T, int TILE, int ROWS, int PITCH>
__device__ __forceinline__ void load_tile_transposed(float* tile, const T* out, long ld, long r0, int B, long c0, int C, int tid) {
    constexpr int V = 16 / (int)sizeof(T);                           // elements per 16-byte vector
    constexpr int SEGS = TILE / V;                                   // vectors per row of the tile
    if (tid < ROWS * SEGS) {
        const int lrow = tid / SEGS, seg = tid % SEGS;               // the loader's row and vector
        float v[V];
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = 0.f;
        const long c = c0 + seg * V;
        if (r0 + lrow < B && c < C) {
            const T* p = out + (r0 + lrow) * ld + c;
            if (c + V <= C && (((uintptr_t)p) & 15) == 0) {
                if constexpr (sizeof(T) == 4) {
                    const float4 q = *(const float4*)p;
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                } else {
                    const half8_t q = *(const half8_t*)p;
#pragma unroll
                    for (int e = 0; e < V; ++e) v[e] = (float)q[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (c + e < C) v[e] = (float)p[e];
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) tile[(seg * V + e) * PITCH + lrow] = v[e];
    }
}

}  // namespace
