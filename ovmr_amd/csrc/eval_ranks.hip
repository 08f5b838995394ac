// Exact ranking figures from the test pass: per class, the count of the kept scores in every gap between two of the class's distinct
// positive scores and tied with each (include/ovmr_hip_ranks.h; DESIGN.md sections 4 and 6).  No counterpart in the reference.  The walk
// is eval_curves.hip's, through the same loader and the same wave-aggregated add (eval_common.h: load_tile_transposed,
// wave_histogram_add); what differs is the slot function, which is a search of the class's edge table instead of a subtraction and a
// product.
//
// eval_ranks_kernel<T>: a 256-thread workgroup owns RK_TILE = 16 consecutive classes (blockIdx.x), wave w the RK_CPW = 4 classes
// 4 w .. 4 w + 3, and walks the chunks of RK_ROWS = 64 rows blockIdx.y, blockIdx.y + gridDim.y, ... (gridDim.y at most
// RK_MAX_ROW_BLOCKS), lane = row.  Before the first chunk every wave reads the edge ranges of its four classes -- clamped as clamp_pair
// (nearest_list.h) clamps a range, and to max_edges -- and copies the edges of every class that has at most RK_STAGE of them to LDS, as
// the VALUE PART OF THE SELECTION KEY (topk_key >> 32): an unsigned whose order is the library's value order, NaN one largest value and
// -0 == +0, so that the search compares integers and converts nothing.  A class with more edges is searched through L2, converting the
// edge it reads.  Staging is decided per CLASS, not per launch: one crowded class (a test set's catch-all) leaves the other 999 in LDS.
// Per chunk and class, lane l searches row l's score: the largest pos with edge[pos - 1] above the score, by halving steps from the top
// bit of the class's edge count -- the count is wave-uniform, so every lane runs the same ceil(log2(E_c + 1)) steps and nothing
// diverges -- then one more read decides tie or gap.  ONE wave_histogram_add per class and chunk sends one atomic per distinct cell:
// after a softmax nearly every negative of a class lies below all its edges, in the last cell, which is then one atomic.
// Class tiles past C, rows past B and rows whose label is outside [0, C) are masked; a label is compared, never used as an address.
// A cell index is at most 2 lo + c + 2 (hi - lo) <= 2 E + c < 2 E + C whatever estart holds: nothing outside the state is written.
// Integer atomics: the state does not depend on arrival order.  Measured: DESIGN.md section 4.
#include "../../include/ovmr_hip_ranks.h"
#include "common.h"
#include "eval_common.h"

namespace {

constexpr int RK_TILE = 16;                 // classes per workgroup: four per wave
constexpr int RK_CPW = RK_TILE / 4;
constexpr int RK_ROWS = 64;                 // rows per chunk: one per lane
constexpr int RK_PITCH = RK_ROWS + 2;       // floats between two classes of the LDS tile (eval_common.h: load_tile_transposed)
constexpr int RK_MAX_ROW_BLOCKS = 256;      // gridDim.y at most: 16 384 rows in one sweep
constexpr int RK_STAGE = 256;               // a class with at most this many edges is searched in LDS: 16 classes x 256 keys = 16 KB

// the value part of the selection key: x above y in the library's order <=> rank_key(x) > rank_key(y); never 0
__device__ __forceinline__ unsigned rank_key(float v) { return (unsigned)(topk_key(v, 0) >> 32); }

template <typename T>
__global__ __launch_bounds__(256) void eval_ranks_kernel(const T* __restrict__ out, long ld, const int64_t* __restrict__ labels, int B, int C,
                                                         const float* __restrict__ edges, const int* __restrict__ estart, long E, int max_edges,
                                                         int* __restrict__ state) {
    __shared__ float tile[RK_TILE * RK_PITCH];
    __shared__ unsigned keys[RK_TILE * RK_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long c0 = (long)blockIdx.x * RK_TILE;                      // < C: gridDim.x is ceil(C / RK_TILE)
    const long plane = 2 * E + C;
    long first[RK_CPW];                                              // the class's first edge, 0 <= first <= E
    int count[RK_CPW];                                               // its edges, 0 <= count <= min(E - first, max_edges); all wave-uniform
#pragma unroll
    for (int i = 0; i < RK_CPW; ++i) {
        const long c = c0 + wave * RK_CPW + i;
        first[i] = 0;
        count[i] = 0;
        if (c >= C) continue;                                        // (wave-uniform)
        const long l = estart[c], u = estart[c + 1];
        const long lo = l < 0 ? 0 : (l > E ? E : l);
        const long hi = u < lo ? lo : (u > E ? E : u);
        first[i] = wave_read(lo, 0);                                 // (equal in every lane: into scalar registers)
        count[i] = wave_read((int)(hi - lo < max_edges ? hi - lo : max_edges), 0);
        if (count[i] <= RK_STAGE)
            for (int j = lane; j < count[i]; j += 64) keys[(wave * RK_CPW + i) * RK_STAGE + j] = rank_key(edges[first[i] + j]);
    }
    // (the first barrier of the loop below stands between these stores and the searches that read them)
    for (long r0 = (long)blockIdx.y * RK_ROWS; r0 < B; r0 += (long)gridDim.y * RK_ROWS) {      // (workgroup-uniform)
        load_tile_transposed<T, RK_TILE, RK_ROWS, RK_PITCH>(tile, out, ld, r0, B, c0, C, tid);
        const bool row_ok = r0 + lane < B;
        const long label = row_ok ? (long)labels[r0 + lane] : -1;
        const bool offered = row_ok && label >= 0 && label < C;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < RK_CPW; ++i) {
            const long c = c0 + wave * RK_CPW + i;
            if (c >= C) continue;                                    // (wave-uniform)
            const int n = count[i];
            const unsigned kx = rank_key(tile[(wave * RK_CPW + i) * RK_PITCH + lane]);
            int pos = 0;                                             // edges strictly above the score: edge[pos - 1] > x >= edge[pos]
            bool tie = false;
            if (n > 0) {
                const int top = 1 << (31 - __builtin_clz(n));
                if (n <= RK_STAGE) {                                 // (wave-uniform, as n is)
                    const unsigned* k = keys + (wave * RK_CPW + i) * RK_STAGE;
                    for (int step = top; step > 0; step >>= 1) {
                        const int at = pos + step;
                        if (at <= n && k[at - 1] > kx) pos = at;
                    }
                    tie = pos < n && k[pos] == kx;
                } else {
                    const float* e = edges + first[i];
                    for (int step = top; step > 0; step >>= 1) {
                        const int at = pos + step;
                        if (at <= n && rank_key(e[at - 1]) > kx) pos = at;
                    }
                    tie = pos < n && rank_key(e[pos]) == kx;
                }
            }
            const long cell = 2 * first[i] + c + 2 * pos + (tie ? 1 : 0);
            wave_histogram_add(state, (label == c ? plane : 0) + cell, offered);
        }
        __syncthreads();                                             // the tile is free again
    }
}

}  // namespace

extern "C" {

long ovmr_eval_ranks_state_cells(int C, long E) {
    if (C < 1 || E < 0) return -1;
    return 2 * (2 * E + C);
}

int ovmr_eval_ranks(const void* out, int out_is_f32, long ld, const int64_t* labels, int B, int C, const float* edges, const int* estart,
                    long E, int max_edges, int* state, ovmr_stream stream) {
    if (C < 1 || B < 0 || E < 0 || max_edges < 0 || max_edges > E || bad_out_matrix(out, out_is_f32, ld, C)) return OVMR_E_ARG;
    if (!labels || !estart || !state || (!edges && E != 0)) return OVMR_E_ARG;
    if ((uintptr_t)labels & 7 || (uintptr_t)state & 3 || (uintptr_t)estart & 3 || (uintptr_t)edges & 3) return OVMR_E_ARG;
    if (B == 0) return 0;
    const long chunks = ((long)B + RK_ROWS - 1) / RK_ROWS;
    const dim3 grid((unsigned)(((long)C + RK_TILE - 1) / RK_TILE), (unsigned)(chunks < RK_MAX_ROW_BLOCKS ? chunks : RK_MAX_ROW_BLOCKS));
    if (out_is_f32)
        hipLaunchKernelGGL(eval_ranks_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)out, ld, labels, B, C, edges, estart,
                           E, max_edges, state);
    else
        hipLaunchKernelGGL(eval_ranks_kernel<half_t>, grid, dim3(256), 0, (hipStream_t)stream, (const half_t*)out, ld, labels, B, C, edges,
                           estart, E, max_edges, state);
    return (int)hipGetLastError();
}

}  // extern "C"
