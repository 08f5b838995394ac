/* ovmr_hip_audit.h -- second extension of the C ABI of libovmr_hip.so (include/ovmr_hip.h): the nearest-exemplar search with an excluded
 * row range per query and a launch for short ranges, which is what an audit of a reference bank asks once per exemplar ("my own class
 * without myself", "everything but my own class").
 *
 * The conventions of ovmr_hip.h hold: device pointers, asynchronous on the caller's stream, no allocation, no host synchronisation
 * (graph-capturable), 0 = ok, otherwise an OVMR_E_* code or a positive hipError_t.  A header of its own because ovmr_hip.h and
 * ovmr_hip_nearest.h are each held to their table symbol by symbol; this one is held the same way to runtime.AUDIT_SIGNATURES
 * (tests/test_audit_cpu.py).
 */
#ifndef OVMR_HIP_AUDIT_H
#define OVMR_HIP_AUDIT_H

#include "ovmr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch ovmr_neighbours_rows needs: 0 for max_range in [1, 4096] (the short launch needs none), otherwise what
 * ovmr_nearest_scratch_bytes(B, R, k) says.  Pure: no device, no handle.  -1 for B < 0, R < 1, R >= 2^32 - 1, k outside [1, 32] or
 * max_range outside [0, 4096].  No counterpart in the reference. */
long ovmr_neighbours_scratch_bytes(int B, long R, int k, int max_range);

/* ovmr_nearest_rows (include/ovmr_hip_nearest.h: score, total order, outputs, clamping, sizes, no allocation, no synchronisation,
 * capturable) with two additions.
 * exclude (may be NULL) int32 [B][2] on the DEVICE: the candidates of query b are the rows lo <= r < hi that are NOT in xlo <= r < xhi.
 * It is clamped like ranges, to 0 <= xlo <= xhi <= R; it may lie outside the range, cover it or be empty.  With ranges NULL the range is
 * the whole bank.  Fewer than k candidates leave a tail of index -1, value -inf.
 * max_range is a promise of the host: every hi - lo <= max_range.  0 = no promise: the tiled launch pair of ovmr_nearest_rows, with its
 * scratch.  1 .. 4096: ONE launch, one wave per query, which reads hi' = min(hi, lo + max_range) -- a broken promise gives a truncated
 * search, never a long-running wave or an access outside the bank -- and needs no scratch (scratch may be NULL).  Its score is
 * h(sum_d Q[b, d] * X[r, d]) with fp32 accumulation in a fixed order of its own and ONE rounding to fp16: a function of the query and
 * the row alone, equal to the tiled launch's wherever the partial sums are exact, at most one fp16 step from it otherwise.
 * OVMR_E_ARG with nothing written: what ovmr_nearest_rows refuses (scratch only where it is needed), a misaligned exclude, max_range
 * outside [0, 4096], max_range > 0 with ranges NULL.  B == 0 returns 0.  No counterpart in the reference. */
int ovmr_neighbours_rows(const void* queries_f16, int B, const void* bank_f16, long R, int D, int k, const int32_t* ranges,
                         const int32_t* exclude, int max_range, float* values, int32_t* indices, void* scratch, long scratch_bytes,
                         ovmr_stream stream);

/* Test hook: ovmr_neighbours_rows with the launch forced.  path 0 = the tiled pair with `slices` bank slices (as ovmr_debug_nearest_rows:
 * scratch must hold B * slices * k 64-bit keys; max_range is ignored); path 1 = the short launch (max_range in [1, 4096], ranges not
 * NULL; slices and scratch are ignored).  No counterpart in the reference. */
int ovmr_debug_neighbours_rows(const void* queries_f16, int B, const void* bank_f16, long R, int D, int k, const int32_t* ranges,
                               const int32_t* exclude, int max_range, float* values, int32_t* indices, void* scratch, long scratch_bytes,
                               int path, int slices, ovmr_stream stream);

#ifdef __cplusplus
}
#endif
#endif
