// Neighbours inside a short range: the k best rows of bank[lo, hi) for every query, minus an excluded row range, one WAVE per query
// (include/ovmr_hip_audit.h; DESIGN.md sections 4 and 6).  The tiled launch pair of nearest.hip multiplies a 64-query tile by every
// 256-row bank tile any of its queries touches; with one class of 16 .. 64 rows per query that is hundreds of times the products the
// answer needs.  Here a wave reads exactly its query's rows.  No counterpart in the reference.
//
// neighbours_short_kernel<PU>: four queries per 256-thread workgroup, one launch, no scratch, no atomics, no counters.
//   * the query is staged in LDS once (2 D bytes per wave); the one barrier of the kernel follows, and spare waves (B % 4) leave after it;
//   * eight lanes share a bank row: lane part p = lane & 7 takes the 16-byte chunk p of every 64-column group, so the eight lanes read
//     one whole 128-byte segment of the row per load; row slot g = lane >> 3.  A pass covers eight rows, a trip PU passes; a trip step
//     loads 8 / PU column groups of each of its PU rows: eight 16-byte loads per lane, the next step's in flight under this step's products.
//     PU is a launch-time choice by max_range and D (short classes do not pay for 64-row trips); it changes which rows travel together
//     and nothing about a row's sum;
//   * fp32 accumulation; rows behind the range's end read its last row again and never become candidates;
//   * ONE rounding to fp16, key = topk_key((float)s, r); rows that are excluded or behind hi' = min(hi, lo + max_range) get key 0;
//     lane (g, p < PU) offers row base + 8 p + g to list_offer (nearest_list.h), lane = rank;
//   * lanes 0 .. k-1 store index and value (key_decode, nearest_list.h) coalesced.
//
// The score of a (query, row) pair does not depend on the row's position in its range, on the pass, on PU or on what shares the workgroup:
// a lane sums the products of its columns in ONE fixed order (column groups ascending, the eight columns of a chunk ascending), each
// product exact in fp32 (two fp16 factors) and each addition one fp32 rounding, and the eight partial sums of a row are combined by ONE
// fixed butterfly (lane xor 1, 2, 4): every lane of the row evaluates the same tree ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)),
// fp32 addition being commutative.  The order differs from the matrix pipe's, so on general operands a score may differ from the tiled
// kernel's by one fp16 step; on operands whose partial sums are exact it is the same fp16 number.
//
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): see DESIGN.md section 4.
#include "../../include/ovmr_hip_audit.h"
#include "common.h"
#include "eval_common.h"
#include "nearest_list.h"

#include <algorithm>

namespace {

using ovmr_list::nkey_t;

constexpr int NS_QLD = 1024;                // halves of LDS per wave: the widest query

template <int PU>
__global__ __launch_bounds__(256) void neighbours_short_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ X,
                                                               const int32_t* __restrict__ ranges, const int32_t* __restrict__ exclude,
                                                               int B, unsigned R, int D, int k, int max_range,
                                                               float* __restrict__ values, int32_t* __restrict__ indices) {
    constexpr int CU = 8 / PU;                                      // column groups per trip step (D / 64 is a multiple: launch_neighbours_short)
    __shared__ __attribute__((aligned(16))) half_t sq[4 * NS_QLD];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = lane & 7, g = lane >> 3;
    const long b = (long)blockIdx.x * 4 + wave;
    half_t* myq = sq + wave * NS_QLD;
    if (b < B)
        for (int i = lane; i < D / 8; i += 64) *(half8_t*)(myq + i * 8) = *(const half8_t*)(Q + b * D + i * 8);
    __syncthreads();                                                // the only barrier: spare waves leave behind it
    if (b >= B) return;

    // the range and the exclusion, clamped to the bank; hi' honours the host's promise whatever the device values say
    long lo, hi, xlo = 0, xhi = 0;
    ovmr_list::clamp_pair(ranges, b, (long)R, lo, hi);
    hi = std::min<long>(hi, lo + max_range);
    if (exclude) ovmr_list::clamp_pair(exclude, b, (long)R, xlo, xhi);

    nkey_t mine = 0;
    for (long base = lo; base < hi; base += 8 * PU) {               // (an empty range: no trip, nothing is read)
        const half_t* xrow[PU];
#pragma unroll
        for (int pu = 0; pu < PU; ++pu) {
            const long r = std::min<long>(base + 8 * pu + g, hi - 1);                 // lo <= r < hi <= R
            xrow[pu] = X + (unsigned long long)r * (unsigned long long)D + p * 8;    // 64-bit: a bank may exceed 2^31 bytes
        }
        float acc[PU];
#pragma unroll
        for (int pu = 0; pu < PU; ++pu) acc[pu] = 0.f;
        half8_t xn[PU][CU];
#pragma unroll
        for (int pu = 0; pu < PU; ++pu)
#pragma unroll
            for (int cu = 0; cu < CU; ++cu) xn[pu][cu] = *(const half8_t*)(xrow[pu] + cu * 64);
        for (int c0 = 0; c0 < D; c0 += 64 * CU) {
            half8_t xf[PU][CU];
#pragma unroll
            for (int pu = 0; pu < PU; ++pu)
#pragma unroll
                for (int cu = 0; cu < CU; ++cu) xf[pu][cu] = xn[pu][cu];
            if (c0 + 64 * CU < D) {
#pragma unroll
                for (int pu = 0; pu < PU; ++pu)
#pragma unroll
                    for (int cu = 0; cu < CU; ++cu) xn[pu][cu] = *(const half8_t*)(xrow[pu] + c0 + 64 * CU + cu * 64);
            }
#pragma unroll
            for (int cu = 0; cu < CU; ++cu) {
                const half8_t qf = *(const half8_t*)(myq + c0 + cu * 64 + p * 8);
#pragma unroll
                for (int pu = 0; pu < PU; ++pu)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[pu] = __builtin_fmaf((float)xf[pu][cu][e], (float)qf[e], acc[pu]);   // the product is exact: one rounding
            }
        }
        // the eight partial sums of a row: one butterfly, the same tree in every lane
        float mys = 0.f;
#pragma unroll
        for (int pu = 0; pu < PU; ++pu) {
            float s = acc[pu];
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
            if (p == pu) mys = s;
        }
        const long r = base + 8 * p + g;
        const bool in = p < PU && r < hi && !(r >= xlo && r < xhi);
        const nkey_t cand = in ? topk_key((float)(half_t)mys, (int)(unsigned)r) : 0;   // the one rounding, to fp16
        ovmr_list::list_offer(mine, cand, lane, k);
    }
    if (lane < k) {
        ovmr_list::key_decode(mine, indices[b * k + lane], values[b * k + lane]);
    }
}

}  // namespace

int launch_neighbours_short(const void* Q, int B, const void* X, long R, int D, int k, const int32_t* ranges, const int32_t* exclude,
                            int max_range, float* values, int32_t* indices, hipStream_t stream) {
    const dim3 grid((unsigned)((B + 3) / 4)), block(256);
    const int NC = D / 64;
    // passes per trip: 64-row trips for long classes, shorter ones where a class would leave most of a trip's loads behind its end
    const int PU = (max_range > 32 || NC % 2) ? 8 : (max_range > 16 || NC % 4) ? 4 : 2;
#define OVMR_NS_LAUNCH(P)                                                                                                                  \
    hipLaunchKernelGGL(neighbours_short_kernel<P>, grid, block, 0, stream, (const half_t*)Q, (const half_t*)X, ranges, exclude, B, (unsigned)R, \
                       D, k, max_range, values, indices)
    if (PU == 8) OVMR_NS_LAUNCH(8);
    else if (PU == 4) OVMR_NS_LAUNCH(4);
    else OVMR_NS_LAUNCH(2);
#undef OVMR_NS_LAUNCH
    return (int)hipGetLastError();
}
