// Score curves from the test pass: per class, the histogram of the scores of its own rows and of everybody else's, over a stream of
// [B, C] output matrices (include/ovmr_hip_curves.h; DESIGN.md sections 4 and 6).  No counterpart in the reference.  The work goes along
// the COLUMNS of the output, as retrieve.hip's does, through the same loader (eval_common.h: load_tile_transposed): a [64 rows][16 classes]
// corner is read along the rows and turned by ninety degrees through LDS, so that a wave takes a class with lane = row.
//
// eval_curves_kernel<T>: a 256-thread workgroup owns EC_TILE = 16 consecutive classes (blockIdx.x), wave w the EC_CPW = 4 classes
// 4 w .. 4 w + 3, and walks the chunks of EC_ROWS = 64 rows blockIdx.y, blockIdx.y + gridDim.y, ...  Unlike the lists of retrieve.hip the
// state lives in memory and is only ever ADDED to, so the rows are split over workgroups as well as the classes: a batch of 256 rows and
// 1000 classes is 63 x 4 workgroups and needs no narrower tile to fill the machine, and there is ONE tiling.  gridDim.y is capped at
// EC_MAX_ROW_BLOCKS; beyond 64 x that many rows a workgroup takes several chunks.  Per chunk:
//   * each wave reads the 64 labels of the chunk, one coalesced load, lane = row;
//   * load_tile_transposed writes the corner to LDS as fp32, tile[class][row], pitch 66 floats;
//   * per class, lane l computes the slot of row l's score and its polarity (label == class), and ONE wave_histogram_add
//     (eval_common.h) sends one atomic per DISTINCT cell: after a softmax that is one to three per (class, chunk) -- nearly every
//     negative of a class falls into one slot, which as 64 same-address atomics would serialise -- with logits it can be 64.
// Class tiles past C, rows past B and rows whose label is outside [0, C) are masked: nothing outside out[0:B, 0:C], labels[0:B] and the
// state is touched, and a label is compared, never used as an address.  Integer atomics: the state does not depend on arrival order.
// An LDS-resident histogram was not built: at 4096 bins a class is 32 KB, a workgroup would hold four, and the rows of a batch (256) are
// far fewer than the cells it would have to flush.  Measured: DESIGN.md section 4.
#include "../../include/ovmr_hip_curves.h"
#include "common.h"
#include "eval_common.h"

namespace {

constexpr int EC_MAX_BINS = 4096;
constexpr int EC_TILE = 16;                 // classes per workgroup: four per wave
constexpr int EC_CPW = EC_TILE / 4;
constexpr int EC_ROWS = 64;                 // rows per chunk: one per lane
constexpr int EC_PITCH = EC_ROWS + 2;       // floats between two classes of the LDS tile (eval_common.h: load_tile_transposed)
constexpr int EC_MAX_ROW_BLOCKS = 256;      // gridDim.y at most: 16 384 rows in one sweep

// the slot of include/ovmr_hip_curves.h; klo / khi: the value part of the selection key of lo / hi.  -ffp-contract=off (build.py): the
// subtraction and the product round once each
__device__ __forceinline__ int curve_slot(float x, float lo, float scale, unsigned klo, unsigned khi, int bins) {
    if (x != x) return bins + 2;
    const unsigned kx = (unsigned)(topk_key(x, 0) >> 32);
    if (kx < klo) return 0;
    if (kx >= khi) return bins + 1;
    const float t = (x - lo) * scale;                                // 0 <= t <= bins (1 + a few ulp): the conversion cannot overflow
    const int j = (int)floorf(t);
    return 1 + (j < bins - 1 ? j : bins - 1);
}

template <typename T>
__global__ __launch_bounds__(256) void eval_curves_kernel(const T* __restrict__ out, long ld, const int64_t* __restrict__ labels, int B, int C,
                                                          float lo, float hi, float scale, int bins, int* __restrict__ state) {
    __shared__ float tile[EC_TILE * EC_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long c0 = (long)blockIdx.x * EC_TILE;                      // < C: gridDim.x is ceil(C / EC_TILE)
    const int S = bins + 3;
    const unsigned klo = (unsigned)(topk_key(lo, 0) >> 32), khi = (unsigned)(topk_key(hi, 0) >> 32);
    for (long r0 = (long)blockIdx.y * EC_ROWS; r0 < B; r0 += (long)gridDim.y * EC_ROWS) {      // (workgroup-uniform)
        load_tile_transposed<T, EC_TILE, EC_ROWS, EC_PITCH>(tile, out, ld, r0, B, c0, C, tid);
        const bool row_ok = r0 + lane < B;
        const long label = row_ok ? (long)labels[r0 + lane] : -1;
        const bool offered = row_ok && label >= 0 && label < C;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < EC_CPW; ++i) {
            const long c = c0 + wave * EC_CPW + i;
            if (c >= C) continue;                                    // (wave-uniform)
            const int slot = curve_slot(tile[(wave * EC_CPW + i) * EC_PITCH + lane], lo, scale, klo, khi, bins);
            wave_histogram_add(state + c * 2 * S, (label == c ? S : 0) + slot, offered);
        }
        __syncthreads();                                             // the tile is free again
    }
}

bool bad_state(int C, int bins) { return C < 1 || bins < 1 || bins > EC_MAX_BINS; }

}  // namespace

extern "C" {

long ovmr_eval_curves_state_bytes(int C, int bins) {
    if (bad_state(C, bins)) return -1;
    return (long)C * 2 * (bins + 3) * 4;
}

int ovmr_eval_curves(const void* out, int out_is_f32, long ld, const int64_t* labels, int B, int C, float lo, float hi, int bins,
                     int* state, ovmr_stream stream) {
    if (bad_state(C, bins) || B < 0 || bad_out_matrix(out, out_is_f32, ld, C)) return OVMR_E_ARG;
    if (!labels || !state || (uintptr_t)labels & 7 || (uintptr_t)state & 3) return OVMR_E_ARG;
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return OVMR_E_ARG;
    const volatile float width = hi - lo;                            // rounded to fp32 here, not carried in a wider register
    const volatile float scale = (float)bins / width;
    if (!std::isfinite(scale) || !(scale > 0.f)) return OVMR_E_ARG;
    if (B == 0) return 0;
    const long chunks = ((long)B + EC_ROWS - 1) / EC_ROWS;
    const dim3 grid((unsigned)(((long)C + EC_TILE - 1) / EC_TILE), (unsigned)(chunks < EC_MAX_ROW_BLOCKS ? chunks : EC_MAX_ROW_BLOCKS));
    const float sc = scale;
    if (out_is_f32)
        hipLaunchKernelGGL(eval_curves_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)out, ld, labels, B, C, lo, hi, sc,
                           bins, state);
    else
        hipLaunchKernelGGL(eval_curves_kernel<half_t>, grid, dim3(256), 0, (hipStream_t)stream, (const half_t*)out, ld, labels, B, C, lo, hi,
                           sc, bins, state);
    return (int)hipGetLastError();
}

}  // extern "C"
