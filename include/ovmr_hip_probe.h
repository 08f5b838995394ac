/* ovmr_hip_probe.h -- extension of the C ABI of libovmr_hip.so (include/ovmr_hip.h): the linear probe, a multinomial logistic regression
 * on image features (lpclip/linear_probe.py of the reference fits it with scikit-learn on the CPU).
 *
 * The objective is scikit-learn's up to a constant factor:
 *     f(W, b) = inv_n * sum over rows n of (lse(z_n) - z_n[y_n])  +  l2 / 2 * ||W||^2,      z_n = W x_n + b,
 * W fp32 [C, D] dense, b fp32 [C] (not penalised), X fp32 [N, D] with rows ldx elements apart, labels int64 [N].  With inv_n = 1 / N and
 * l2 = 1 / (c N) its minimiser is that of LogisticRegression(C=c, penalty="l2").  A row whose label is outside [0, C) contributes
 * nothing to the loss or the gradient; a label is only ever COMPARED with a class index and never used as an address.
 *
 * The conventions of ovmr_hip.h hold: device pointers, asynchronous on the caller's stream, no allocation, no host synchronisation, 0 = ok,
 * otherwise OVMR_E_ARG (nothing written) or a positive hipError_t.  No handle.  The entry points live in a header of their own for the
 * reason ovmr_hip_nearest.h gives; this header is held to runtime.PROBE_SIGNATURES symbol by symbol (tests/test_probe_cpu.py).
 *
 * Every float operand is fp32.  x, W, gW and the workspace are 16-byte aligned, b, gb and row_loss 4-byte, labels 8-byte; D is a multiple
 * of 32 and ldx a multiple of 4, at least D (the constraints of the fp32 GEMM the logits go through).
 *
 * What ovmr_probe_loss_grad promises beyond its values:
 *   NO FLOATING-POINT ATOMICS.  The result is a function of the inputs alone, bit for bit, run after run.
 *   INDEPENDENT OF THE WORKSPACE.  Every workspace element that is read was written by the same call.
 *   INDEPENDENT OF HOW THE ROWS ARE CUT.  Every element of gW and gb is ONE fused-multiply-add chain over the rows in their order,
 *   continued from the value the element starts with; so the call over rows [0, N) equals, bit for bit, the call over [0, n1) followed
 *   by an accumulate = 1 call over [n1, N), for every n1 that is a multiple of ovmr_probe_row_quantum().  A caller cuts the rows this
 *   way to bound the workspace.
 */
#ifndef OVMR_HIP_PROBE_H
#define OVMR_HIP_PROBE_H

#include "ovmr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The scores of a probe: out[n, c] = sum_d x[n, d] W[c, d] + b[c] for B rows, out fp32 with rows ldo >= C elements apart, 4-byte aligned.
 * ONE launch of the library's fp32 GEMM with its bias epilogue (the kernel ovmr_debug_gemm(f32 = 1) runs): the fit and the test pass
 * share it, so a probe is evaluated on the scores it was trained on.  Nothing outside out[0:B, 0:C] is written.  B == 0 returns 0.
 * OVMR_E_ARG with nothing written: a NULL or misaligned pointer, B < 0, C < 1, D < 32, D % 32 != 0, ldx < D, ldx % 4 != 0, ldo < C.
 * Replaces clf.predict of lpclip/linear_probe.py (the scores behind it). */
int ovmr_probe_logits(const float* x, long ldx, int B, const float* W, const float* b, int C, int D, float* out, long ldo,
                      ovmr_stream stream);

/* Rows a caller cuts at (see above): a positive constant.  Pure: no device, no handle.  No counterpart in the reference. */
int ovmr_probe_row_quantum(void);

/* Bytes of workspace ovmr_probe_loss_grad needs for N rows: 4 N ceil4(C), the logits of the rows, C rounded up to a multiple of 4.
 * Pure: no device, no handle.  -1 for N < 0, C < 1, D < 32 or D % 32 != 0.  No counterpart in the reference. */
long ovmr_probe_workspace_bytes(int N, int C, int D);

/* Loss terms and gradient of the objective above over N rows.  A fixed sequence of at most three launches:
 *   1. the logits of the N rows into the workspace (the GEMM of ovmr_probe_logits);
 *   2. every logits row in place into its residual r = (softmax(z) - onehot(y)) * inv_n -- the row maximum subtracted first, exp
 *      evaluated once per element -- and row_loss[n] = lse(z_n) - z_n[y_n]; a row with a foreign label becomes zeros with loss 0;
 *   3. gW[c, d] (+)= sum_n r[n, c] x[n, d] and gb[c] (+)= sum_n r[n, c] on v_mfma_f32_16x16x4_f32, the contraction running over the rows
 *      with no transposed copy of either operand.
 * accumulate == 0: gW starts from l2 * W and gb from 0 (what they held is never read).  accumulate == 1: both continue from what they
 * hold, and W, b only serve the logits.  row_loss fp32 [N] is written, never accumulated: the sum of the loss is the caller's.
 * C == 1 gives row_loss == 0 and adds exact zeros.  N == 0 launches step 3 alone when accumulate == 0 (gW = l2 * W, gb = 0) and
 * nothing otherwise; x, labels, row_loss and the workspace may then be NULL.  Rows past N are masked, never clamped into another row.
 * Nothing outside x[0:N], labels[0:N], W, b and the first ovmr_probe_workspace_bytes(N, C, D) bytes of the workspace is read; nothing
 * outside that workspace, row_loss[0:N], gW [C, D] and gb [C] is written.
 * OVMR_E_ARG with nothing written: a NULL or misaligned pointer (but see N == 0), N < 0, C < 1, D < 32, D % 32 != 0, ldx < D,
 * ldx % 4 != 0, accumulate not 0 or 1.
 * Replaces the loss and gradient scikit-learn's L-BFGS evaluates behind LogisticRegression.fit in lpclip/linear_probe.py. */
int ovmr_probe_loss_grad(const float* x, long ldx, const int64_t* labels, int N, int C, int D, const float* W, const float* b, float inv_n,
                         float l2, int accumulate, float* workspace, float* row_loss, float* gW, float* gb, ovmr_stream stream);

#ifdef __cplusplus
}
#endif
#endif
