/* ovmr_hip_nearest.h -- extension of the C ABI of libovmr_hip.so (include/ovmr_hip.h): nearest exemplars on the device.
 *
 * The conventions of ovmr_hip.h hold: device pointers, asynchronous on the caller's stream, no allocation, no host synchronisation
 * (graph-capturable), 0 = ok, otherwise an OVMR_E_* code or a positive hipError_t.  The entry points live in a header of their own
 * because ovmr_hip.h, runtime.SIGNATURES and the tables of tests/boundary_cases.py are held to each other symbol by symbol; this
 * header is held the same way to runtime.EXT_SIGNATURES (tests/test_nearest_cpu.py).
 */
#ifndef OVMR_HIP_NEAREST_H
#define OVMR_HIP_NEAREST_H

#include "ovmr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch ovmr_nearest_rows needs for B queries, a bank of R rows and k neighbours: B * S * k 64-bit keys, S = the number of bank
 * slices the launcher cuts the bank into (a function of B and R alone).  Pure: no device, no handle.  -1 for B < 0, R < 1, R >= 2^32 - 1 or
 * k outside [1, 32].  No counterpart in the reference. */
long ovmr_nearest_scratch_bytes(int B, long R, int k);

/* The k nearest bank rows of every query, in ONE pass over the bank: s[b, r] = h(sum_d Q[b, d] * X[r, d]), fp32 accumulation on the matrix
 * pipe and ONE rounding to fp16 (the rounding point of an fp16 `@`), never written to memory.  queries_f16 [B, D] and bank_f16 [R, D]: dense,
 * 16-byte aligned, D % 64 == 0, 64 <= D <= 1024, 1 <= R < 2^32 - 1 (r * D is 64-bit: a bank may exceed 2^31 bytes), 1 <= k <= min(R, 32).
 * The order is the total order of ovmr_topk_rows on (score, bank row): larger score first, equal scores to the LOWER bank row, every NaN
 * above +inf, -0.0 == +0.0.  indices int32 [B, k]: bank rows, best first; values fp32 [B, k]: the scores as fp32 (a NaN stays a NaN; a
 * -0.0 score is reported as +0.0, which the order does not tell apart).
 * ranges (may be NULL) int32 [B][2] on the DEVICE: query b considers only the rows lo <= r < hi, 0 <= lo <= hi <= R; whatever is read is
 * clamped to that, so wrong values give wrong results and never an access outside the bank.  A query with fewer than k eligible rows fills
 * its tail with index -1 and value -inf; an empty range is legal.
 * scratch: ovmr_nearest_scratch_bytes(B, R, k) bytes, 8-byte aligned, owned by the caller; its contents before the call do not matter and
 * two calls in flight need two scratch buffers.  The result is a function of queries, bank, ranges and k alone.
 * OVMR_E_ARG with nothing written: a NULL queries / bank / values / indices / scratch, a misaligned operand, D or k outside the above,
 * R < 1 or R >= 2^32 - 1, B < 0, scratch_bytes too small.  B == 0 returns 0.  Two launches; needs no handle.
 * No counterpart in the reference. */
int ovmr_nearest_rows(const void* queries_f16, int B, const void* bank_f16, long R, int D, int k, const int32_t* ranges,
                      float* values, int32_t* indices, void* scratch, long scratch_bytes, ovmr_stream stream);

/* Test hook: ovmr_nearest_rows with the number of bank slices forced (slices >= 1; slices beyond the bank's 256-row tiles stay empty).
 * scratch must hold B * slices * k 64-bit keys.  The result does not depend on slices.  No counterpart in the reference. */
int ovmr_debug_nearest_rows(const void* queries_f16, int B, const void* bank_f16, long R, int D, int k, const int32_t* ranges,
                            float* values, int32_t* indices, void* scratch, long scratch_bytes, int slices, ovmr_stream stream);

#ifdef __cplusplus
}
#endif
#endif
