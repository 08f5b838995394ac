// Nearest exemplars: the k best bank rows of every query, s[b, r] = h(Q[b] . X[r]), without the [B, R] score matrix ever being written
// (include/ovmr_hip_nearest.h).  No counterpart in the reference: it answers "which reference images made the model
// say that" from the exemplar features the model already carries (modules.CustomCLIP.nearest_exemplars).
//
// Order: the library's total order (eval_common.h) on topk_key((float)s, r) -- larger score first, equal scores to the lower bank row,
// NaN above +inf, -0 == +0.  The k keys of a query are distinct, so "the k largest" is one set in one order, whatever the grid.
//
// Launch 1, nearest_tiles_kernel<QB>: a workgroup owns one tile of BM = 32 QB queries and one SLICE of the bank, and walks the slice's
// 256-row tiles in increasing row order.
//   * the query tile is staged in LDS once (rows past B: zeros, with an empty range);
//   * a bank tile is multiplied on v_mfma_f32_32x32x16_f16 in the layout of head_fused.hip: the bank rows are the A operand, straight
//     from global memory (each row is read once per workgroup), the queries the B operand from LDS; wave w owns rows 64 w .. 64 w + 63
//     of the tile, a lane ends up with ONE query (per 32-query block) and 16 rows per 32 x 32 block;
//   * the scores are rounded to fp16 -- the one rounding -- and written to an LDS score tile [BM][256];
//   * selection: wave w owns the queries w BM/4 ..; per query, lanes 0 .. k-1 hold the current k best keys (rank = lane; kept in LDS between
//     tiles), lane l looks at the four scores of rows 4 l .. 4 l + 3.  A score must beat the query's k-th best key to matter: one ballot
//     per four rows says whether any does, and after the first tiles almost none do.  Survivors are inserted one at a time
//     (position = number of keys above it: a ballot and a population count; the tail shifts by one lane), the threshold rising as they
//     enter.  Rows outside the query's range or past R never become candidates (key 0).
//   * a workgroup whose slice meets none of its queries' ranges writes its empty lists and leaves before its first barrier (every wave
//     evaluates the condition on all BM ranges: it is uniform); otherwise it walks the tiles between the lowest lo and highest hi
//     and skips, by the same uniform test, every tile none of its ranges reaches.
//   * per-slice lists -> scratch [B][S][k] keys (0 = no row).
// Launch 2, nearest_merge_kernel: one wave per query takes the k largest of its S k keys with the same insertion, lane j keeps rank j and
// stores index and value (key_decode) coalesced.  No atomics on global memory, no counters, nothing to re-arm: the scratch is
// written completely before it is read.
//
// include/ovmr_hip_audit.h adds an excluded row range per query: nearest_tiles_kernel<QB, EXCL = true> keeps the clamped exclusions beside the
// ranges in LDS and turns excluded candidates into key 0 (the instantiations without EXCL are the code they were), and ovmr_neighbours_rows
// takes the one-wave-per-query launch of neighbours.hip where the host promises short ranges.  The list helpers, key_decode and the
// range clamp (clamp_pair) live in nearest_list.h.
//
// Registers (hipcc -O3, gfx950, --save-temps): see DESIGN.md section 4.
#include "../../include/ovmr_hip_nearest.h"
#include "../../include/ovmr_hip_audit.h"
#include "common.h"
#include "eval_common.h"
#include "nearest_list.h"

#include <algorithm>

namespace {

typedef float float16_t __attribute__((ext_vector_type(16)));
typedef unsigned long long key_t;

constexpr int NR_BN = 256;                  // bank rows per tile: 4 waves x 64
constexpr int NR_SLD = NR_BN + 4;           // score tile row stride in halves (8-byte aligned rows)
constexpr int NR_KMAX = 32;
constexpr int NB_MAX_RANGE = 4096;          // ovmr_neighbours_rows: the ceiling of max_range, the project's ceiling for a class (agg_max_len)
constexpr int NR_CUS = 256;                 // the launcher's S is a pure function of B and R (ovmr_nearest_scratch_bytes): no device query

using ovmr_list::wave_read_key; using ovmr_list::list_insert; using ovmr_list::list_offer;   // nearest_list.h
using ovmr_list::key_decode; using ovmr_list::clamp_pair;

struct NearestArgs {
    const half_t* Q; const half_t* X; const int32_t* ranges; key_t* scratch;
    int B, D, k, S;
    unsigned R, Tq;
    int tiles_per_slice;
    const int32_t* exclude;                     // EXCL instantiations only (last: the other fields keep their places)
};

size_t nearest_lds_bytes(int BM, int D, bool excl = false) {
    return (size_t)BM * NR_KMAX * 8 + (size_t)BM * (D + 8) * 2 + (size_t)BM * NR_SLD * 2 + (size_t)BM * (excl ? 4 : 2) * 4;
}

// EXCL: query b also leaves out the rows xlo <= r < xhi of a.exclude (ovmr_neighbours_rows).  Exclusion only turns candidates into key 0:
// the "meets" and tile-skip tests below look at the ranges alone and stay correct, because they over-approximate.
template <int QB, bool EXCL = false>
__global__ __launch_bounds__(256) void nearest_tiles_kernel(const NearestArgs a) {
    constexpr int BM = 32 * QB;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int D = a.D, k = a.k, ldq = D + 8;                        // + 16 B per row: the 16 lanes of a ds_read_b128 pass hit 64 distinct banks
    key_t* list = (key_t*)smem_raw;                                 // [BM][32]
    half_t* sq = (half_t*)(smem_raw + (size_t)BM * NR_KMAX * 8);    // [BM][ldq] queries
    half_t* sc = sq + (size_t)BM * ldq;                             // [BM][NR_SLD] fp16 scores of the current tile
    unsigned* qlo = (unsigned*)(sc + (size_t)BM * NR_SLD);          // [BM], then qhi [BM]
    unsigned* qhi = qlo + BM;
    unsigned* qxlo = qhi + BM;                                      // [BM], then qxhi [BM]: EXCL only
    unsigned* qxhi = qxlo + BM;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    // Workgroups go to the 8 XCDs round robin by their index: the Tq query tiles of one slice take indices 8 apart, so that they run
    // on ONE XCD at about the same time and the slice's bank rows come from HBM once and from that XCD's L2 for the other tiles
    // (whole bank, 256 queries x 640 000 rows: every query tile reading the bank from HBM bounded the launch).
    const unsigned within = blockIdx.x % (8u * a.Tq);
    const int s = (int)(blockIdx.x / (8u * a.Tq) * 8u + within % 8u), q0 = (int)(within / 8u) * BM;
    if (s >= a.S) return;                                           // (the last group of eight slices may be short; uniform, nothing to write)
    const unsigned R = a.R;
    // the slice [s0, s1): whole tiles; slices past the last tile are empty
    const unsigned long long t_first = (unsigned long long)s * a.tiles_per_slice * NR_BN;
    const unsigned s0 = (unsigned)std::min<unsigned long long>(t_first, R);
    const unsigned s1 = (unsigned)std::min<unsigned long long>(t_first + (unsigned long long)a.tiles_per_slice * NR_BN, R);

    // every wave: the ranges of all BM queries (lane = query), clamped to [0, R]; does any of them meet the slice?
    unsigned lo = 0, hi = 0;
    if (lane < BM && q0 + lane < a.B) {
        if (a.ranges) clamp_pair(a.ranges, q0 + lane, (long)R, lo, hi);
        else hi = R;
    }
    const bool meets = std::max(lo, s0) < std::min(hi, s1);
    unsigned wlo = meets ? lo : 0xFFFFFFFFu, whi = meets ? hi : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        wlo = std::min(wlo, (unsigned)__shfl_xor(wlo, o, 64));
        whi = std::max(whi, (unsigned)__shfl_xor(whi, o, 64));
    }
    if (whi == 0) {                                                 // nothing to do (uniform over the workgroup): empty lists, no barrier
        for (int i = tid; i < BM * k; i += 256) {
            const int q = i / k, r = i % k;
            if (q0 + q < a.B) a.scratch[((long)(q0 + q) * a.S + s) * k + r] = 0;
        }
        return;
    }
    const unsigned t_beg = std::max(s0, wlo) / NR_BN * NR_BN, t_end = std::min(s1, whi);   // s0 is a multiple of the tile: so is t_beg >= s0

    if (wave == 0 && lane < BM) { qlo[lane] = lo; qhi[lane] = hi; }
    if constexpr (EXCL) {
        if (wave == 1 && lane < BM) {                               // clamped like the range; rows past B: empty
            unsigned xlo = 0, xhi = 0;
            if (q0 + lane < a.B) clamp_pair(a.exclude, q0 + lane, (long)R, xlo, xhi);
            qxlo[lane] = xlo; qxhi[lane] = xhi;
        }
    }
    for (int i = tid; i < BM * NR_KMAX; i += 256) list[i] = 0;
    for (int i = tid; i < BM * (D / 8); i += 256) {
        const int row = i / (D / 8), ch = i % (D / 8);
        half8_t v;
        if (q0 + row < a.B) v = *(const half8_t*)(a.Q + (long)(q0 + row) * D + ch * 8);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (half_t)0.f;
        }
        *(half8_t*)(sq + row * ldq + ch * 8) = v;
    }
    __syncthreads();

    for (unsigned long long t0l = t_beg; t0l < t_end; t0l += NR_BN) {
        const unsigned t0 = (unsigned)t0l;
        // a tile no query's range reaches is skipped (every wave holds all BM ranges, lane = query: uniform over the workgroup) -- queries
        // restricted to one class each leave most of a slice untouched
        if (!__builtin_amdgcn_ballot_w64(std::max<unsigned long long>(lo, t0) < std::min<unsigned long long>(hi, t0l + NR_BN))) continue;
        // ---- scores of bank rows t0 + 64 wave + 32 rb + (e & 3) + 8 (e >> 2) + 4 h against query 32 qb + j -> acc[rb][qb][e]
        float16_t acc[2][QB];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[rb][qb][e] = 0.f;
        const half_t* arow[2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {                            // rows past the bank repeat its last row; they never become candidates
            const unsigned long long r = std::min<unsigned long long>((unsigned long long)t0 + wave * 64 + rb * 32 + j, (unsigned long long)R - 1);
            arow[rb] = a.X + r * (unsigned long long)D + h * 8;     // 64-bit: a bank may exceed 2^31 bytes
        }
        constexpr int KU = 4;                                      // k-steps per trip: 64 columns (D is a multiple of 64), eight 16-byte loads per lane in flight
        half8_t an[2][KU];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int u = 0; u < KU; ++u) an[rb][u] = *(const half8_t*)(arow[rb] + u * 16);
        for (int k0 = 0; k0 < D; k0 += 16 * KU) {                   // the next trip's fragments are in flight while this trip's products run:
            half8_t af[2][KU];                                      // the bank comes straight from global memory, its latency bounds a tile
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int u = 0; u < KU; ++u) af[rb][u] = an[rb][u];
            if (k0 + 16 * KU < D) {
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int u = 0; u < KU; ++u) an[rb][u] = *(const half8_t*)(arow[rb] + k0 + 16 * KU + u * 16);
            }
#pragma unroll
            for (int u = 0; u < KU; ++u)
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) {
                    const half8_t b = *(const half8_t*)(sq + (qb * 32 + j) * ldq + k0 + u * 16 + h * 8);
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) acc[rb][qb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[rb][u], b, acc[rb][qb], 0, 0, 0);
                }
        }
        // ---- the one rounding, to fp16; four consecutive rows per store
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                for (int kq = 0; kq < 4; ++kq)
                    *(half4_t*)(sc + (qb * 32 + j) * NR_SLD + wave * 64 + rb * 32 + kq * 8 + 4 * h) =
                        (half4_t){(half_t)acc[rb][qb][4 * kq], (half_t)acc[rb][qb][4 * kq + 1], (half_t)acc[rb][qb][4 * kq + 2],
                                  (half_t)acc[rb][qb][4 * kq + 3]};
        __syncthreads();
        // ---- selection: wave w, queries w BM/4 ..; lane l, rows t0 + 4 l .. + 3
        for (int qi = 0; qi < BM / 4; ++qi) {
            const int q = wave * (BM / 4) + qi;
            const unsigned long long ql = qlo[q], qh = qhi[q];
            if (std::max<unsigned long long>(ql, t0) >= std::min<unsigned long long>(qh, (unsigned long long)t0 + NR_BN)) continue;   // (wave-uniform)
            unsigned long long xl = 0, xh = 0;
            if constexpr (EXCL) { xl = qxlo[q]; xh = qxhi[q]; }
            key_t mine = lane < NR_KMAX ? list[q * NR_KMAX + lane] : 0;
            const half4_t sv = *(const half4_t*)(sc + q * NR_SLD + lane * 4);
            bool changed = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned long long r = (unsigned long long)t0 + lane * 4 + e;
                bool in = r >= ql && r < qh;
                if constexpr (EXCL) in = in && !(r >= xl && r < xh);
                const key_t cand = in ? topk_key((float)sv[e], (int)(unsigned)r) : 0;
                changed |= list_offer(mine, cand, lane, k);
            }
            if (changed && lane < NR_KMAX) list[q * NR_KMAX + lane] = mine;
        }
        __syncthreads();                                            // the score tile is free again
    }
    for (int i = tid; i < BM * k; i += 256) {
        const int q = i / k, r = i % k;
        if (q0 + q < a.B) a.scratch[((long)(q0 + q) * a.S + s) * k + r] = list[q * NR_KMAX + r];
    }
}

__global__ __launch_bounds__(256) void nearest_merge_kernel(const key_t* __restrict__ scratch, int B, int S, int k,
                                                            float* __restrict__ values, int32_t* __restrict__ indices) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * 4 + wave;
    if (b >= B) return;                                             // (wave-uniform; no barrier below)
    const key_t* keys = scratch + b * S * k;
    const long n = (long)S * k;
    key_t mine = 0;
    for (long i = 0; i < n; i += 64) {
        const key_t cand = i + lane < n ? keys[i + lane] : 0;
        list_offer(mine, cand, lane, k);
    }
    if (lane < k) {
        key_decode(mine, indices[b * k + lane], values[b * k + lane]);
    }
}

template <int QB, bool EXCL = false>
int launch_tiles(const NearestArgs& a, int grid, size_t lds, hipStream_t s) {
    auto kern = nearest_tiles_kernel<QB, EXCL>;
    static size_t lds_set[OVMR_MAX_DEVICES] = {};                    // per QB and device: the largest dynamic LDS size granted so far
    if (lds > 64 * 1024) {
        int dev = 0;
        HIP_CHECK_RET(hipGetDevice(&dev));
        if (dev < 0 || dev >= OVMR_MAX_DEVICES) return OVMR_E_ARG;
        if (lds > lds_set[dev]) {
            HIP_CHECK_RET(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            lds_set[dev] = lds;
        }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, s, a);
    return (int)hipGetLastError();
}

long bank_tiles(long R) { return (R + NR_BN - 1) / NR_BN; }

// Slices for B queries and R rows: about two workgroups per CU of the 64-query grid, never a slice below one tile.
int pick_slices(int B, long R) {
    const long Tq = std::max(1, (B + 63) / 64);
    return (int)std::max<long>(1, std::min<long>((2 * NR_CUS + Tq - 1) / Tq, bank_tiles(R)));
}

bool bad_shape(int B, long R, int k) { return B < 0 || R < 1 || R >= 0xFFFFFFFFL || k < 1 || k > NR_KMAX; }

// what the tiled and the short path ask of a search alike: its extents, then (the caller returns 0 for B == 0 in between) its operands
bool bad_search_shape(int B, long R, int D, int k) { return bad_shape(B, R, k) || k > R || D < 64 || D > 1024 || D % 64; }
bool bad_search_operands(const void* Q, const void* X, const int32_t* ranges, const int32_t* exclude, const float* values,
                         const int32_t* indices) {
    if (!Q || !X || !values || !indices) return true;
    return ((uintptr_t)Q | (uintptr_t)X) & 15 || ((uintptr_t)values | (uintptr_t)indices | (uintptr_t)ranges | (uintptr_t)exclude) & 3;
}

int nearest_rows(const void* Q, int B, const void* X, long R, int D, int k, const int32_t* ranges, float* values, int32_t* indices,
                 void* scratch, long scratch_bytes, int S, hipStream_t stream, const int32_t* exclude = nullptr) {
    if (bad_search_shape(B, R, D, k) || S < 1) return OVMR_E_ARG;
    if (B == 0) return 0;
    if (bad_search_operands(Q, X, ranges, exclude, values, indices) || !scratch || (uintptr_t)scratch & 7) return OVMR_E_ARG;
    if (scratch_bytes < 0 || (unsigned long long)scratch_bytes < (unsigned long long)B * S * k * 8) return OVMR_E_ARG;
    // 64-query tiles where they fit the 160 KB of LDS and there are more than 32 queries, else 32-query tiles
    const int BM = (B > 32 && nearest_lds_bytes(64, D, exclude != nullptr) <= 160 * 1024) ? 64 : 32;
    const long Tq = (B + BM - 1) / BM, grid = (S + 7L) / 8 * 8 * Tq;     // slices in groups of eight (nearest_tiles_kernel)
    if (grid > 0x7FFFFFFFL) return OVMR_E_ARG;
    NearestArgs a;
    a.Q = (const half_t*)Q; a.X = (const half_t*)X; a.ranges = ranges; a.scratch = (key_t*)scratch;
    a.B = B; a.D = D; a.k = k; a.S = S; a.R = (unsigned)R; a.Tq = (unsigned)Tq;
    a.tiles_per_slice = (int)((bank_tiles(R) + S - 1) / S);
    a.exclude = exclude;
    const size_t lds = nearest_lds_bytes(BM, D, exclude != nullptr);
    if (exclude) {
        if (int rc = BM == 64 ? launch_tiles<2, true>(a, (int)grid, lds, stream) : launch_tiles<1, true>(a, (int)grid, lds, stream)) return rc;
    } else if (int rc = BM == 64 ? launch_tiles<2>(a, (int)grid, lds, stream) : launch_tiles<1>(a, (int)grid, lds, stream))
        return rc;
    hipLaunchKernelGGL(nearest_merge_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, (const key_t*)scratch, B, S, k, values, indices);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

long ovmr_nearest_scratch_bytes(int B, long R, int k) {
    if (bad_shape(B, R, k)) return -1;
    return (long)B * pick_slices(B, R) * k * 8;
}

int ovmr_nearest_rows(const void* queries_f16, int B, const void* bank_f16, long R, int D, int k, const int32_t* ranges, float* values,
                      int32_t* indices, void* scratch, long scratch_bytes, ovmr_stream stream) {
    if (bad_shape(B, R, k)) return OVMR_E_ARG;
    return nearest_rows(queries_f16, B, bank_f16, R, D, k, ranges, values, indices, scratch, scratch_bytes, pick_slices(B, R), (hipStream_t)stream);
}

int ovmr_debug_nearest_rows(const void* queries_f16, int B, const void* bank_f16, long R, int D, int k, const int32_t* ranges, float* values,
                            int32_t* indices, void* scratch, long scratch_bytes, int slices, ovmr_stream stream) {
    return nearest_rows(queries_f16, B, bank_f16, R, D, k, ranges, values, indices, scratch, scratch_bytes, slices, (hipStream_t)stream);
}

// ---- include/ovmr_hip_audit.h: the search with an excluded row range per query; max_range > 0 takes the one-wave-per-query launch of
// neighbours.hip, 0 the tiled launch pair above

long ovmr_neighbours_scratch_bytes(int B, long R, int k, int max_range) {
    if (bad_shape(B, R, k) || max_range < 0 || max_range > NB_MAX_RANGE) return -1;
    return max_range > 0 ? 0 : (long)B * pick_slices(B, R) * k * 8;
}

int ovmr_debug_neighbours_rows(const void* queries_f16, int B, const void* bank_f16, long R, int D, int k, const int32_t* ranges,
                               const int32_t* exclude, int max_range, float* values, int32_t* indices, void* scratch, long scratch_bytes,
                               int path, int slices, ovmr_stream stream) {
    if (path == 0)
        return nearest_rows(queries_f16, B, bank_f16, R, D, k, ranges, values, indices, scratch, scratch_bytes, slices, (hipStream_t)stream, exclude);
    if (path != 1 || bad_search_shape(B, R, D, k) || max_range < 1 || max_range > NB_MAX_RANGE) return OVMR_E_ARG;
    if (B == 0) return 0;
    if (bad_search_operands(queries_f16, bank_f16, ranges, exclude, values, indices) || !ranges) return OVMR_E_ARG;
    return launch_neighbours_short(queries_f16, B, bank_f16, R, D, k, ranges, exclude, max_range, values, indices, (hipStream_t)stream);
}

int ovmr_neighbours_rows(const void* queries_f16, int B, const void* bank_f16, long R, int D, int k, const int32_t* ranges,
                         const int32_t* exclude, int max_range, float* values, int32_t* indices, void* scratch, long scratch_bytes,
                         ovmr_stream stream) {
    if (bad_shape(B, R, k) || max_range < 0 || max_range > NB_MAX_RANGE || (max_range > 0 && !ranges)) return OVMR_E_ARG;
    return ovmr_debug_neighbours_rows(queries_f16, B, bank_f16, R, D, k, ranges, exclude, max_range, values, indices, scratch, scratch_bytes,
                                      max_range > 0 ? 1 : 0, max_range > 0 ? 1 : pick_slices(B, R), stream);
}

}  // extern "C"
