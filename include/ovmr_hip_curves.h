/* ovmr_hip_curves.h -- extension of the C ABI of libovmr_hip.so (include/ovmr_hip.h): score curves from the test pass.
 *
 * ovmr_eval_counts and ovmr_eval_detail keep what the ARGMAX of a row decides.  These entry points keep what every SCORE says: per class,
 * the distribution of the scores of its own images (the rows whose label is that class) and of everybody else's, as one integer
 * histogram per (class, polarity).  Average precision, AUROC and the best-F1 operating point of every class are sums over that state
 * (ovmr_amd/evaluator.py); the state itself is integers, adds across batches and ranks, and depends on what was offered alone.
 *
 * The conventions of ovmr_hip.h hold: device pointers, asynchronous on the caller's stream, no allocation, no host synchronisation, 0 = ok,
 * otherwise OVMR_E_ARG (nothing written) or a positive hipError_t.  No handle.  The entry points live in a header of their own for the
 * reason ovmr_hip_nearest.h gives; this header is held to runtime.CURVES_SIGNATURES symbol by symbol (tests/test_curves_cpu.py).
 *
 * The state: int32 [C][2][S] with S = bins + 3, 4-byte aligned, C * 2 * S * 4 bytes.  Plane 0 of class c counts its NEGATIVES (rows whose
 * label is another class), plane 1 its POSITIVES (rows whose label is c), each by the slot of out[b, c].  ALL-ZERO BYTES ARE THE EMPTY
 * STATE.  A cell counts rows, and a test set holds fewer than 2^31 images, so no cell overflows; sums over ranks are sums of int32.
 *
 * The slot of a score x = (float)out[b, c], for finite lo < hi and 1 <= bins <= 4096:
 *     x is NaN                 -> S - 1      (every NaN, of either sign: NaN is largest, as in the library's total order)
 *     otherwise x below lo     -> 0          (-inf included)
 *     otherwise x at or above hi -> S - 2    (+inf included)
 *     otherwise                -> 1 + min(bins - 1, (int)floorf(t)),   t = (x - lo) * scale
 * The subtraction and the product are each rounded once to fp32: no fused multiply-add.  scale = (float)bins / (hi - lo) is computed by
 * the launcher on the HOST in fp32 (one subtraction, one division, each rounded once).  The two comparisons are made in the value order of
 * the library's selection key (the order of ovmr_topk_rows and of the floor of ovmr_retrieve_update): -0.0 == +0.0, and a denormal is a
 * number of its own, never flushed to zero.  The min is not decoration: for (lo, hi, bins) = (-100, 100, 1024) and (-1, 1, 4096) the
 * largest fp32 below hi gives t == bins exactly.  The map x -> slot is NON-DECREASING in that order (each of the three steps is), so a
 * cut between two slots is a cut between two sets of scores.  The nominal lower edge of slot s in [1, bins] is lo + (s - 1) * (hi - lo) /
 * bins; it is nominal: the slot function above is what decides.
 */
#ifndef OVMR_HIP_CURVES_H
#define OVMR_HIP_CURVES_H

#include "ovmr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the state for C classes and `bins` bins: C * 2 * (bins + 3) * 4.  Pure: no device, no handle.  -1 for C < 1 or bins outside
 * [1, 4096].  No counterpart in the reference. */
long ovmr_eval_curves_state_bytes(int C, int bins);

/* Counts one batch into the state.  out: the [B, C] output matrix of the batch, fp16 (out_is_f32 == 0) or fp32, rows ld >= C elements
 * apart, aligned to the element size only (an odd C leaves every second fp16 row unaligned).  labels: int64 [B].  For every row b with
 * 0 <= labels[b] < C and every class c:  state[c][labels[b] == c][slot(out[b, c])] += 1.  A row whose label is outside [0, C) is offered
 * to NO class (ovmr_eval_counts counts such rows, and the evaluator raises on them).  A label is only ever COMPARED with a class index
 * and never used as an address: a wrong label cannot reach outside the state.
 * The call ACCUMULATES: the state after any sequence of calls is a function of the multiset of (class, is-own-label, slot) offered, not
 * of how the rows were cut into batches, of the order of the batches, or of which rank saw which batch.
 * ONE launch; nothing outside out[0:B, 0:C], labels[0:B] and state[0:C] is touched.  B == 0 returns 0 and leaves the state alone.  All
 * arguments but the buffers' contents are scalars, so the call may be captured in a graph.
 * OVMR_E_ARG with nothing written: a NULL out / labels / state, C < 1, B < 0, ld < C, bins outside [1, 4096], lo or hi not finite,
 * lo >= hi, a scale that is not finite or not positive (hi - lo overflows or is too small for bins), out not aligned to its element
 * size, labels not 8-byte aligned, state not 4-byte aligned.
 * No counterpart in the reference. */
int ovmr_eval_curves(const void* out, int out_is_f32, long ld, const int64_t* labels, int B, int C, float lo, float hi, int bins,
                     int* state, ovmr_stream stream);

#ifdef __cplusplus
}
#endif
#endif
