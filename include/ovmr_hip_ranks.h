/* ovmr_hip_ranks.h -- extension of the C ABI of libovmr_hip.so (include/ovmr_hip.h): exact per-class ranking figures from the test pass.
 *
 * ovmr_eval_curves (include/ovmr_hip_curves.h) keeps the scores of a class BINNED over a range somebody chose, and its average precision
 * and AUROC are figures of the bins.  For one class every EXACT figure -- what a sort of the raw scores would give -- depends only on
 * where each negative falls relative to the class's own positive scores.  So the figures need one integer histogram per class whose
 * edges are the class's DISTINCT POSITIVE SCORES: the count of negatives in every gap between two of them and the count tied with each.
 * The edges are known when the pass ends; the caller keeps the [B, C] outputs until then and offers them to this entry point once.
 * Average precision, AUROC and the best-F1 operating point of every class are sums over that state (ovmr_amd/evaluator.py:
 * rank_figures); the state itself is integers, adds across batches and ranks, and depends on what was offered alone.
 *
 * The conventions of ovmr_hip.h hold: device pointers, asynchronous on the caller's stream, no allocation, no host synchronisation, 0 = ok,
 * otherwise OVMR_E_ARG (nothing written) or a positive hipError_t.  No handle.  The entry points live in a header of their own for the
 * reason ovmr_hip_nearest.h gives; this header is held to runtime.RANKS_SIGNATURES symbol by symbol (tests/test_ranks_cpu.py).
 *
 * The edges: fp32 [E] on the device, 4-byte aligned.  Class c owns edges[estart[c] : estart[c + 1]], E_c of them; estart is int32 [C + 1]
 * on the device, 4-byte aligned, non-decreasing from 0 to E.  A class's edges are its distinct positive scores, STRICTLY DESCENDING in the
 * value order of the library's selection key (the order of ovmr_topk_rows): NaN is largest and ONE value (every NaN, of either sign),
 * -0.0 == +0.0, and a denormal is a number of its own, never flushed to zero.  fp16 scores convert exactly to fp32, so one fp32 edge table
 * serves both output dtypes.
 *
 * The state: int32 [2][2 E + C], 4-byte aligned.  Plane 0 counts NEGATIVES (rows whose label is another class), plane 1 POSITIVES (rows
 * whose label is the class).  Within a plane class c's cells start at 2 estart[c] + c, and there are 2 E_c + 1 of them.  ALL-ZERO BYTES
 * ARE THE EMPTY STATE.  A cell counts rows, and a test set holds fewer than 2^31 images, so no cell overflows; sums over ranks are sums
 * of int32.
 *
 * The cell of a score x = (float)out[b, c] within its class: let k be the number of the class's edges strictly above x in that order.
 *     k < E_c and edge[k] equals x  -> 2 k + 1    (a tie with edge k)
 *     otherwise                     -> 2 k        (the gap above edge k; 2 E_c: below every edge)
 * A class without a positive has the one cell 0.  The map x -> cell is NON-INCREASING in that order.
 */
#ifndef OVMR_HIP_RANKS_H
#define OVMR_HIP_RANKS_H

#include "ovmr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* int32 cells of the state for C classes and E edges in all: 2 * (2 E + C).  Pure: no device, no handle.  -1 for C < 1 or E < 0.
 * No counterpart in the reference. */
long ovmr_eval_ranks_state_cells(int C, long E);

/* Counts one batch into the state.  out: the [B, C] output matrix of the batch, fp16 (out_is_f32 == 0) or fp32, rows ld >= C elements
 * apart, aligned to the element size only (an odd C leaves every second fp16 row unaligned).  labels: int64 [B].  For every row b with
 * 0 <= labels[b] < C and every class c:  state[labels[b] == c][2 estart[c] + c + cell_c(out[b, c])] += 1.  A row whose label is outside
 * [0, C) is offered to NO class.  A label is only ever COMPARED with a class index and never used as an address.
 * The call ACCUMULATES with integer atomics: the state after any sequence of calls is a function of the multiset of (class, is-own-label,
 * cell) offered, not of how the rows were cut into batches, of the order of the batches, or of which rank saw which batch.
 * max_edges: the caller's promise of the largest E_c; a class is searched against its first min(E_c, max_edges) edges.  Every estart
 * value read is clamped (0 <= lo <= hi <= E, hi - lo <= max_edges): garbage in estart or edges can miscount, but nothing outside
 * out[0:B, 0:C], labels[0:B], estart[0:C + 1], edges[0:E] is read and nothing outside the state is written.
 * ONE launch, no allocation, no synchronisation.  B == 0 returns 0 and leaves the state alone.  All arguments but the buffers' contents
 * are scalars, so the call may be captured in a graph.
 * OVMR_E_ARG with nothing written: a NULL out / labels / estart / state, a NULL edges unless E == 0, C < 1, B < 0, ld < C, E < 0,
 * max_edges < 0, max_edges > E, out not aligned to its element size, labels not 8-byte aligned, edges / estart / state not 4-byte
 * aligned.
 * No counterpart in the reference. */
int ovmr_eval_ranks(const void* out, int out_is_f32, long ld, const int64_t* labels, int B, int C, const float* edges, const int* estart,
                    long E, int max_edges, int* state, ovmr_stream stream);

#ifdef __cplusplus
}
#endif
#endif
