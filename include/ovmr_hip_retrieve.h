/* ovmr_hip_retrieve.h -- extension of the C ABI of libovmr_hip.so (include/ovmr_hip.h): search an image pool by class.
 *
 * Where ovmr_topk_rows selects along a ROW of one [B, C] output matrix (the k best classes of an image), these entry points select along
 * its COLUMNS, over a stream of such matrices: the m best images of every class, with the lists carried from batch to batch in a state
 * buffer the caller owns.
 *
 * The conventions of ovmr_hip.h hold: device pointers, asynchronous on the caller's stream, no allocation, no host synchronisation, 0 = ok,
 * otherwise OVMR_E_ARG (nothing written) or a positive hipError_t.  No handle.  The entry points live in a header of their own for the
 * reason ovmr_hip_nearest.h gives; this header is held to runtime.RETRIEVE_SIGNATURES symbol by symbol (tests/test_retrieve_cpu.py).
 *
 * The state: C lists of m 64-bit keys, [C, m], 8-byte aligned, C * m * 8 bytes.  A key is (order-preserving bits of the score as
 * fp32) << 32 | (0xFFFFFFFF - image index), the key of ovmr_topk_rows with the image index in the place of the column: larger score first,
 * equal scores to the LOWER image index, every NaN above +inf, -0.0 == +0.0.  List c holds the m largest keys offered to class c so far,
 * largest first; 0 = an unfilled rank.  ALL-ZERO BYTES ARE THE EMPTY STATE.  The keys of one class are distinct (an image is offered
 * once), so the state after any sequence of updates and merges is a function of the SET of (image, class, score) triples offered and of m
 * alone: it does not depend on how the pool was cut into batches, on the order of the batches, or on which rank saw which batch.  Beyond
 * that the state is opaque; it is byte-copyable, so it can go through an all-gather as it is (as int64 [C, m]).
 */
#ifndef OVMR_HIP_RETRIEVE_H
#define OVMR_HIP_RETRIEVE_H

#include "ovmr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the state for C classes and m images per class: C * m * 8.  Pure: no device, no handle.  -1 for C < 1 or m outside [1, 32].
 * No counterpart in the reference. */
long ovmr_retrieve_state_bytes(int C, int m);

/* Empties every list: the state becomes all-zero bytes (a memset on the stream does the same).  OVMR_E_ARG: a NULL or misaligned state,
 * C < 1, m outside [1, 32].  No counterpart in the reference. */
int ovmr_retrieve_reset(void* state, int C, int m, ovmr_stream stream);

/* Offers one batch to the lists.  out: the [B, C] output matrix of the batch, fp16 (out_is_f32 == 0) or fp32, rows ld >= C elements apart,
 * aligned to the element size only (an odd C leaves every second fp16 row unaligned).  Row b is image base + b of the pool,
 * 0 <= base and base + B <= 2^32 - 1.  For every class c, element (b, c) is offered to list c with the key of ((float)out[b, c], base + b).
 * floor (may be NULL): fp32 [B] on the device; element (b, c) is eligible only if, in the value order of the key, it is not below
 * floor[b] -- the comparison is on the value part of the key alone, so an element equal to its floor is eligible, -0.0 equals +0.0, a NaN
 * floor admits only NaNs and a floor of -inf admits everything.  (With floor[b] = the K-th best score of row b, a class is searched among
 * the images that rank it within their K best, ties at the cut included.)
 * ONE launch; nothing outside out[0:B, 0:C], floor[0:B] and state[0:C, 0:m] is touched.  B == 0 returns 0 and leaves the state alone.
 * base is a SCALAR argument: a captured graph replays the same base, so the update is for eager streams.
 * OVMR_E_ARG with nothing written: a NULL out / state, m outside [1, 32], C < 1, B < 0, ld < C, base < 0, base + B > 2^32 - 1, out not
 * aligned to its element size, floor not 4-byte aligned, state not 8-byte aligned.
 * No counterpart in the reference. */
int ovmr_retrieve_update(const void* out, int out_is_f32, long ld, int B, int C, int m, long base, const float* floor, void* state,
                         ovmr_stream stream);

/* state becomes the state of the union of both streams, provided they hold disjoint image indices (an image offered to both would be
 * listed twice).  Commutative up to which buffer is written; merging an empty state changes nothing.  One launch, one wave per class.
 * OVMR_E_ARG: a NULL or misaligned state / other, other == state (a stream merged with itself), C < 1, m outside [1, 32].
 * No counterpart in the reference. */
int ovmr_retrieve_merge(void* state, const void* other, int C, int m, ovmr_stream stream);

/* Decodes the state: values fp32 [C, m] and indices int64 [C, m], best first.  A value is the score as fp32 (a NaN stays a NaN; a -0.0
 * score is reported as +0.0, which the order does not tell apart); an unfilled rank is index -1, value -inf.  EVERY element of both
 * outputs is written; the state is not changed.  OVMR_E_ARG: a NULL state / values / indices, state or indices not 8-byte aligned, values
 * not 4-byte aligned, C < 1, m outside [1, 32].  No counterpart in the reference. */
int ovmr_retrieve_finish(const void* state, int C, int m, float* values, int64_t* indices, ovmr_stream stream);

#ifdef __cplusplus
}
#endif
#endif
