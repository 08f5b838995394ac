"""Times of the linear probe (`probe.hip`): ONE loss-and-gradient evaluation (runtime.probe_loss_grad: logits GEMM,
residual rows, TN gradient GEMM) and ONE whole fit (probe.fit at C = 1, tol 1e-4), at 1000 classes x 16 shots x 512 features and at
100 x 8 x 512, beside

    torch     the same evaluation written in torch-ROCm fp32 on the same GPU (two matrix products, a softmax, and the same driver on top of
              it for the fit): the yardstick
    sklearn   LogisticRegression(solver="lbfgs", C=1, tol=1e-4, max_iter=1000) on the host's CPUs, at the small size only

in the method of tools/curves_bench.py: HIP events on the launch stream around one call, 20 timed calls after 5, one process, the forms
ALTERNATING call by call.  The rows are sep * centroid[y] + N(0, I), unit length, rounded to fp16 (tests/probe_cases.py: problem).  Also
printed: the three launches of one evaluation timed apart, and the TN GEMM's share of the fp32 MFMA roof (157.3 TFLOP/s).

    python tools/probe_bench.py            # one JSON line per size
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ovmr_amd import probe, runtime  # noqa: E402
from curves_bench import alternating, timed_us  # noqa: E402

SIZES = ((1000, 16, 512), (100, 8, 512))
ROOF_TFLOPS = 157.3


def rows_of(C, shots, D, sep=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    cent = torch.randn((C, D), generator=g)
    y = torch.arange(C).repeat_interleave(shots)
    x = sep * cent[y] + torch.randn((C * shots, D), generator=g)
    return (x / x.norm(dim=1, keepdim=True)).half().float(), y


def torch_loss_grad(X, y):
    rows = torch.arange(len(y), device=X.device)

    def loss_grad(W, b, c):
        inv_n, l2 = probe.objective_scalars(len(y), c)
        z = torch.addmm(b, X, W.t())
        lse = torch.logsumexp(z, dim=1)
        r = torch.softmax(z, dim=1)
        row_loss = lse - z[rows, y]
        r[rows, y] -= 1.0
        r *= inv_n
        loss = row_loss.sum(dtype=torch.float64) * inv_n + W.double().square().sum() * (0.5 * l2)
        return loss, torch.addmm(W, r.t(), X, beta=l2), r.sum(dim=0)
    return loss_grad


def median_ms(fn, n=5):
    fn()
    t = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 2), round(min(t), 2), round(max(t), 2)


def case(C, shots, D):
    X, y = rows_of(C, shots, D)
    N = len(y)
    dX, dy = X.cuda(), y.cuda()
    g = torch.Generator().manual_seed(1)
    W, b = (torch.randn((C, D), generator=g) * 0.1).cuda(), (torch.randn((C,), generator=g) * 0.1).cuda()
    ours, theirs = probe.device_loss_grad(dX, dy), torch_loss_grad(dX, dy)
    a, t = ours(W, b, 1.0), theirs(W, b, 1.0)
    row = {"C": C, "shots": shots, "D": D, "N": N,
           "grad_max_abs_diff_vs_torch": float(max((a[1] - t[1]).abs().max(), (a[2] - t[2]).abs().max())), "loss_diff_vs_torch": abs(float(a[0]) - float(t[0]))}
    r = alternating({"loss_grad": lambda: ours(W, b, 1.0), "torch_fp32": lambda: theirs(W, b, 1.0)})
    for n, (med, mn, mx) in r.items():
        row[n + "_us"], row[n + "_min_us"], row[n + "_max_us"] = med, mn, mx
    # the launches apart: the logits GEMM alone; what is left of an evaluation is the residual rows, the TN GEMM and the fp64 loss sum
    lib = runtime.load_library()
    out = torch.empty((N, C), device="cuda")
    logits_us = sorted(timed_us(lambda: runtime.probe_logits(dX, W, b, out=out)) for _ in range(20))[10]
    row["logits_us"] = round(logits_us, 1)
    flops = 2.0 * N * C * D
    row["logits_tflops"] = round(flops / logits_us / 1e6, 1)
    rest_us = max(row["loss_grad_us"] - logits_us, 1e-3)
    row["residual_plus_tn_us"] = round(rest_us, 1)
    row["tn_tflops_at_least"] = round(flops / rest_us / 1e6, 1)           # (the residual rows and the fp64 loss sum are inside rest_us)
    row["tn_share_of_fp32_mfma_roof_at_least"] = round(flops / rest_us / 1e6 / ROOF_TFLOPS, 3)
    row["row_quantum"], row["workspace_MB"] = lib.ovmr_probe_row_quantum(), round(lib.ovmr_probe_workspace_bytes(N, C, D) / 1e6, 2)
    # whole fits
    fits = {}

    def fit_with(name, lg):
        fits[name] = probe.fit(lg, C, D, 1.0, tol=1e-4, device="cuda")
    row["fit_ms"], row["fit_min_ms"], row["fit_max_ms"] = median_ms(lambda: fit_with("ours", ours))
    row["torch_fit_ms"], row["torch_fit_min_ms"], row["torch_fit_max_ms"] = median_ms(lambda: fit_with("torch", theirs))
    for name, f in fits.items():
        row[("" if name == "ours" else "torch_") + "fit_iterations"], row[("" if name == "ours" else "torch_") + "fit_evaluations"] = f.n_iter, f.n_eval
        assert f.converged, name
    if C <= 100:
        from sklearn.linear_model import LogisticRegression
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            sk = LogisticRegression(solver="lbfgs", C=1.0, tol=1e-4, max_iter=1000).fit(X.numpy(), y.numpy())
            t.append((time.perf_counter() - t0) * 1e3)
        row["sklearn_fit_ms"], row["sklearn_iterations"], row["sklearn_cpus"] = round(statistics.median(t), 2), int(sk.n_iter_[0]), len(os.sched_getaffinity(0))
        mine = (X @ fits["ours"].W.cpu().T + fits["ours"].b.cpu()).argmax(dim=1).numpy()
        row["train_predictions_equal_sklearn"] = bool((mine == sk.predict(X.numpy())).all())
    print(json.dumps(row), flush=True)
    return row


def main():
    runtime.load_library()
    np.random.seed(0)
    return [case(*s) for s in SIZES]


if __name__ == "__main__":
    main()
