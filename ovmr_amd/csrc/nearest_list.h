// The sorted key list of one query, shared by the nearest-exemplar kernels (nearest.hip: nearest_tiles_kernel, nearest_merge_kernel;
// neighbours.hip: neighbours_short_kernel) and, one list per class, by retrieve.hip.  A key is topk_key((float)score, bank row)
// (eval_common.h): 64 bits, larger = better, 0 = no row; the keys of one query are distinct, so "the k largest" is one set in one order.
// Beside the list: what a key decodes to, and the clamp of a row range read from device memory.
#pragma once
#include "eval_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace ovmr_list {

typedef unsigned long long nkey_t;

__device__ __forceinline__ nkey_t wave_read_key(nkey_t v, int lane) { return (nkey_t)wave_read((long)v, lane); }

// The sorted list of one query: lane j < k holds the key of rank j (descending; 0 = empty), lanes >= k hold 0.  Inserts the (wave-uniform)
// key c > 0, which differs from every key in the list; the last key falls off a full list.
__device__ __forceinline__ void list_insert(nkey_t& mine, nkey_t c, int lane, int k) {
    const int pos = (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mine > c));
    const unsigned lo = __shfl_up((unsigned)mine, 1, 64), hi = __shfl_up((unsigned)(mine >> 32), 1, 64);
    const nkey_t up = ((nkey_t)hi << 32) | lo;
    if (lane == pos) mine = c;
    else if (lane > pos) mine = up;
    if (lane >= k) mine = 0;
}

// Every candidate (one per lane, 0 = none) that belongs among the k best enters the list.  Returns whether the list changed.
__device__ __forceinline__ bool list_offer(nkey_t& mine, nkey_t cand, int lane, int k) {
    nkey_t thr = wave_read_key(mine, k - 1);                       // the k-th best (0 while the list is not full)
    unsigned long long todo = __builtin_amdgcn_ballot_w64(cand > thr);
    const bool any = todo != 0;
    while (todo) {
        const int src = __builtin_ctzll(todo);
        list_insert(mine, wave_read_key(cand, src), lane, k);
        thr = wave_read_key(mine, k - 1);
        todo &= todo - 1;
        todo &= __builtin_amdgcn_ballot_w64(cand > thr);           // the threshold rose: fewer survive
    }
    return any;
}

// the value a key was built from (topk_key inverted): NaN for every NaN, +0 for either zero
__device__ __forceinline__ float key_value(nkey_t key) {
    const unsigned u = (unsigned)(key >> 32);
    if (u == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// what a list entry says: (row, value), or (-1, -inf) for an empty one (retrieve_finish_kernel states the same with an int64 row)
__device__ __forceinline__ void key_decode(nkey_t key, int32_t& index, float& value) {
    index = key ? (int32_t)(0xFFFFFFFFu - (unsigned)key) : -1;
    value = key ? key_value(key) : -INFINITY;
}

// pair b of pairs [*, 2] (a range or an exclusion, read from device memory) clamped to the R rows: 0 <= lo <= hi <= R whatever it holds
template <typename I>   // unsigned or long
__device__ __forceinline__ void clamp_pair(const int32_t* pairs, long b, long R, I& lo, I& hi) {
    const long l = pairs[2 * b], u = pairs[2 * b + 1];
    const long cl = std::min<long>(std::max<long>(l, 0), R);
    lo = (I)cl;
    hi = (I)std::min<long>(std::max<long>(u, cl), R);
}

}  // namespace ovmr_list
