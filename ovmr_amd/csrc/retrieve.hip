// Search an image pool by class: the m best images of every class over a stream of [B, C] output matrices (include/ovmr_hip_retrieve.h;
// DESIGN.md sections 4 and 6).  No counterpart in the reference: ovmr_topk_rows (topk.hip) selects along a row of one matrix, this
// selects along the columns of many, with the lists carried from batch to batch in a state [C, m] of 64-bit keys.
//
// Order: the library's total order (eval_common.h) on topk_key((float)score, image index) -- larger score first, equal scores to the
// lower image, NaN above +inf, -0 == +0.  The keys of a class are distinct, so "the m largest" is one set in one order: the state is a
// function of what was offered, not of the batches it came in.  A list is the sorted per-wave key list of nearest_list.h (lane j holds
// rank j; a candidate must beat the m-th key: one ballot rejects a whole chunk of rows), turned by ninety degrees: lane = row of the batch.
//
// retrieve_update_kernel<T, RT_TILE>: a 256-thread workgroup owns RT_TILE = 16 consecutive classes, wave w the RT_CPW = 4 classes 4 w .. 4 w + 3,
// whose lists stay in registers for the whole kernel (loaded from the state once, stored once).  The rows of the batch are walked in
// chunks of 64:
//   * the chunk's [64 rows][16 classes] corner goes to LDS turned by ninety degrees, tile[class][row] in fp32, through
//     load_tile_transposed (eval_common.h; the pitch of 66 floats is derived there);
//   * per class, lane l reads the score of row l of the chunk and builds the key; rows at or past B and scores below the row's floor
//     (compared on the value part of the key) offer key 0 = nothing; list_offer does the rest.
// Class tiles past C and rows past B are masked: nothing outside out[0:B, 0:C], floor[0:B] and state[0:C, 0:m] is touched.
// Why 16 classes per workgroup and not 64 (a whole 128-byte line of an fp16 row): the work per class is serial in the wave that owns it,
// so the launch is as parallel as it has waves, and 1000 classes in 64-class tiles are 16 workgroups on 256 CUs.  32 bytes of a row per
// workgroup still fill whole 32-byte sectors; the lines are shared by the four neighbouring workgroups through L2.  Up to
// RT_NARROW_MAX_C = 2048 classes even that leaves the machine short of waves (1000 classes: 63 workgroups), and where every offer enters
// its list (columns rising along the stream) a wave's four classes cost 1024 serial insertions per batch of 256 rows: there the
// RT_TILE_NARROW = 4 instantiation gives every class a wave of its own (fp16: one element per thread; the matrix is half a megabyte).
// Measured: DESIGN.md section 4.
//
// retrieve_merge_kernel: one wave per class, the other list's m keys are the candidates of ONE list_offer.  retrieve_finish_kernel: one
// thread per (class, rank) decodes key -> (value, index); the index stays unsigned to the end and widens to int64 here.  It is
// key_decode of nearest_list.h written out: through the helper the kernel's register count moved (13 -> 12 VGPRs), so it keeps its own lines.
#include "../../include/ovmr_hip_retrieve.h"
#include "common.h"
#include "eval_common.h"
#include "nearest_list.h"

namespace {

typedef unsigned long long rkey_t;

constexpr int RT_KMAX = 32;
constexpr int RT_TILE = 16;                 // classes per workgroup: four per wave ...
constexpr int RT_TILE_NARROW = 4;           // ... and one per wave up to RT_NARROW_MAX_C classes, where waves are what a launch lacks
constexpr int RT_NARROW_MAX_C = 2048;
constexpr int RT_ROWS = 64;                 // rows per chunk: one per lane
constexpr int RT_PITCH = RT_ROWS + 2;       // floats between two classes of the LDS tile (eval_common.h: load_tile_transposed)
constexpr long RT_MAX_IMAGES = 0xFFFFFFFFL; // image indices are < 2^32 - 1: the low half of a key is 0xFFFFFFFF - index >= 1

using ovmr_list::list_offer; using ovmr_list::key_value;   // nearest_list.h

template <typename T, int RT_TILE>           // RT_TILE: 16 or RT_TILE_NARROW (shadows the constant above)
__global__ __launch_bounds__(256) void retrieve_update_kernel(const T* __restrict__ out, long ld, int B, int C, int m, unsigned base,
                                                              const float* __restrict__ floor, rkey_t* __restrict__ state) {
    constexpr int RT_CPW = RT_TILE / 4;                              // classes per wave
    __shared__ float tile[RT_TILE * RT_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long c0 = (long)blockIdx.x * RT_TILE;                      // < C: the grid is ceil(C / RT_TILE)
    rkey_t mine[RT_CPW];
#pragma unroll
    for (int i = 0; i < RT_CPW; ++i) {
        const long c = c0 + wave * RT_CPW + i;
        mine[i] = (c < C && lane < m) ? state[c * m + lane] : 0;
    }
    constexpr int V = 16 / (int)sizeof(T);                           // elements per 16-byte vector
    for (int r0 = 0; r0 < B; r0 += RT_ROWS) {
        if constexpr (RT_TILE < V) {                                 // a tile narrower than a vector (fp16, 4 classes): one element per thread
            if (tid < RT_ROWS * RT_TILE) {
                const int lrow = tid / RT_TILE, col = tid % RT_TILE;
                const long c = c0 + col;
                float v = 0.f;
                if (r0 + lrow < B && c < C) v = (float)out[(long)(r0 + lrow) * ld + c];
                tile[col * RT_PITCH + lrow] = v;
            }
        } else
            load_tile_transposed<T, RT_TILE, RT_ROWS, RT_PITCH>(tile, out, ld, r0, B, c0, C, tid);
        __syncthreads();
        const bool row_ok = r0 + lane < B;
        const unsigned idx = base + (unsigned)(r0 + lane);           // < 2^32 - 1 where row_ok (checked by the launcher)
        unsigned low = 0;                                            // the value part of floor's key; 0 is below every value
        if (floor && row_ok) low = (unsigned)(topk_key(floor[r0 + lane], 0) >> 32);
#pragma unroll
        for (int i = 0; i < RT_CPW; ++i) {
            if (c0 + wave * RT_CPW + i >= C) continue;               // (wave-uniform)
            const rkey_t key = topk_key(tile[(wave * RT_CPW + i) * RT_PITCH + lane], (int)idx);
            list_offer(mine[i], row_ok && (unsigned)(key >> 32) >= low ? key : 0, lane, m);
        }
        __syncthreads();                                             // the tile is free again
    }
#pragma unroll
    for (int i = 0; i < RT_CPW; ++i) {
        const long c = c0 + wave * RT_CPW + i;
        if (c < C && lane < m) state[c * m + lane] = mine[i];
    }
}

__global__ __launch_bounds__(256) void retrieve_merge_kernel(rkey_t* __restrict__ state, const rkey_t* __restrict__ other, int C, int m) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * 4 + wave;
    if (c >= C) return;                                              // (wave-uniform; no barrier below)
    rkey_t mine = lane < m ? state[c * m + lane] : 0;
    const rkey_t cand = lane < m ? other[c * m + lane] : 0;
    if (list_offer(mine, cand, lane, m) && lane < m) state[c * m + lane] = mine;
}

__global__ __launch_bounds__(256) void retrieve_finish_kernel(const rkey_t* __restrict__ state, long n, float* __restrict__ values,
                                                              int64_t* __restrict__ indices) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const rkey_t key = state[i];                                     // ovmr_list::key_decode with an int64 index, spelled out: see above
    indices[i] = key ? (int64_t)(0xFFFFFFFFu - (unsigned)key) : -1;
    values[i] = key ? key_value(key) : -INFINITY;
}

bool bad_lists(int C, int m) { return C < 1 || m < 1 || m > RT_KMAX; }

}  // namespace

extern "C" {

long ovmr_retrieve_state_bytes(int C, int m) {
    if (bad_lists(C, m)) return -1;
    return (long)C * m * 8;
}

int ovmr_retrieve_reset(void* state, int C, int m, ovmr_stream stream) {
    if (bad_lists(C, m) || !state || (uintptr_t)state & 7) return OVMR_E_ARG;
    return (int)hipMemsetAsync(state, 0, (size_t)C * m * 8, (hipStream_t)stream);
}

int ovmr_retrieve_update(const void* out, int out_is_f32, long ld, int B, int C, int m, long base, const float* floor, void* state,
                         ovmr_stream stream) {
    if (bad_lists(C, m) || B < 0 || base < 0 || base > RT_MAX_IMAGES || base + B > RT_MAX_IMAGES) return OVMR_E_ARG;
    if (bad_out_matrix(out, out_is_f32, ld, C) || !state) return OVMR_E_ARG;
    if ((uintptr_t)floor & 3 || (uintptr_t)state & 7) return OVMR_E_ARG;
    if (B == 0) return 0;
    const bool narrow = C <= RT_NARROW_MAX_C;
    const int tile = narrow ? RT_TILE_NARROW : RT_TILE;
    const dim3 grid((unsigned)(((long)C + tile - 1) / tile));
    auto launch = [&](auto kern, auto* typed) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, typed, ld, B, C, m, (unsigned)base, floor, (rkey_t*)state);
    };
    if (out_is_f32) {
        if (narrow) launch(retrieve_update_kernel<float, RT_TILE_NARROW>, (const float*)out);
        else launch(retrieve_update_kernel<float, RT_TILE>, (const float*)out);
    } else {
        if (narrow) launch(retrieve_update_kernel<half_t, RT_TILE_NARROW>, (const half_t*)out);
        else launch(retrieve_update_kernel<half_t, RT_TILE>, (const half_t*)out);
    }
    return (int)hipGetLastError();
}

int ovmr_retrieve_merge(void* state, const void* other, int C, int m, ovmr_stream stream) {
    if (bad_lists(C, m) || !state || !other || ((uintptr_t)state | (uintptr_t)other) & 7) return OVMR_E_ARG;
    if (state == other) return OVMR_E_ARG;                          // a stream merged with itself would list every image twice
    hipLaunchKernelGGL(retrieve_merge_kernel, dim3((unsigned)(((long)C + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (rkey_t*)state,
                       (const rkey_t*)other, C, m);
    return (int)hipGetLastError();
}

int ovmr_retrieve_finish(const void* state, int C, int m, float* values, int64_t* indices, ovmr_stream stream) {
    if (bad_lists(C, m) || !state || !values || !indices) return OVMR_E_ARG;
    if (((uintptr_t)state | (uintptr_t)indices) & 7 || (uintptr_t)values & 3) return OVMR_E_ARG;
    const long n = (long)C * m;
    hipLaunchKernelGGL(retrieve_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const rkey_t*)state,
                       n, values, indices);
    return (int)hipGetLastError();
}

}  // extern "C"
