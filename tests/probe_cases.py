"""The linear probe's loss and gradient: the fp64 statement, the fp32 error budget, honest fp32 evaluations, planted defects, and the
synthetic few-shot problems of the fit tests.  Plain numpy / torch, importable without a GPU (test_probe_cpu.py, test_hip_probe.py).

The objective (include/ovmr_hip_probe.h):  f = inv_n * sum_n (lse(z_n) - z_n[y_n]) + l2 / 2 * ||W||^2,  z_n = W x_n + b; a row whose
label is outside [0, C) counts for nothing.  reference() evaluates row_loss, gW and gb in fp64 and, beside each, the most an honest fp32
evaluation may differ from it.

THE BUDGET, in the manner of gemm_ln_exact.py: every rounding the kernels make is stated once, to first order in u = 2^-24, with the
worst-case factor n u for a sum of n terms in ANY order; no constant is tuned to a run.

  z      a D-term dot product and the bias add:            |dz|  <= (D + 1) u (|W| |x| + |b|)           =: ez[n, c];  Ez[n] = max_c ez
  t      t = z - max_c z, one subtraction:                 |dt|  <= 2 Ez + u |t|                        =: et[n] with T = max_c |t|
  e      e = exp(t), EXP_ULP units in the last place:      rel   <= et + 2 EXP_ULP u
  s      s = sum_c e, C positive terms, wave butterfly:    rel   <= et + 2 EXP_ULP u + (C + 6) u        =: es[n]
  p      p = e * (1 / s): a reciprocal and a product:      rel   <= (et + 2 EXP_ULP u) + es + 2 u       =: ep[n]
  r      r = (p - [c == y]) * inv_n, two roundings, and an e or p below fp32's smallest normal number may be flushed to zero:
                                                           |dr|  <= inv_n (p ep + 2 u |p - [c == y]| + 2^-125)   =: er[n, c]
  gW     start g0 = l2 * W (one rounding; none when it is the accumulate = 1 input), then an N-term sum of products:
                                                           |dgW| <= er^T |x| + (N + 1) u (|g0| + |r|^T |x|) + u |g0|
  gb     an N-term sum:                                    |dgb| <= sum_n er + N u (|gb0| + sum_n |r|)
  loss   log(s) - (z[y] - max):                            |dl|  <= es + 2 LOG_ULP u |log s| + 2 Ez + u |z[y] - max| + u |loss|

EXP_ULP = LOG_ULP = 3: what the OpenCL full profile allows expf and logf, which the device's math library follows.
"""
import numpy as np
import torch

U = 2.0 ** -24
EXP_ULP = 3
LOG_ULP = 3
UNDER = 2.0 ** -125   # two values (e, p) that may each be flushed below 2^-126
QUANTUM = 32          # ovmr_probe_row_quantum(): PR_ROWS of csrc/probe.hip (held by test_probe_cpu.py)


# ---- the fp64 statement and the budget -------------------------------------------------------------------------------------------------

def reference(x, y, W, b, inv_n, l2, gW0=None, gb0=None):
    """x [N, D], y [N] int, W [C, D], b [C] (any float dtype; the VALUES are what the kernels see), inv_n and l2 the fp32 scalars handed
    over.  gW0 / gb0: the accumulate = 1 inputs (None: the start is l2 * W and 0).  -> dict of fp64 arrays row_loss, gW, gb and their
    budgets e_row_loss, e_gW, e_gb."""
    x, W, b = (np.asarray(a, dtype=np.float64) for a in (x, W, b))
    y = np.asarray(y, dtype=np.int64)
    N, D = x.shape
    C = W.shape[0]
    inv_n, l2 = float(np.float32(inv_n)), float(np.float32(l2))
    ok = (y >= 0) & (y < C)
    hot = np.zeros((N, C))
    hot[np.nonzero(ok)[0], y[ok]] = 1.0
    z = x @ W.T + b
    ez = (D + 1) * U * (np.abs(x) @ np.abs(W).T + np.abs(b))
    m = z.max(axis=1, keepdims=True) if N else np.zeros((0, 1))
    t = z - m
    Ez = ez.max(axis=1, keepdims=True) if N else np.zeros((0, 1))
    et = 2 * Ez + U * (np.abs(t).max(axis=1, keepdims=True) if N else 0)
    e = np.exp(t)
    s = e.sum(axis=1, keepdims=True)
    es = et + 2 * EXP_ULP * U + (C + 6) * U
    ep = et + 2 * EXP_ULP * U + es + 2 * U
    p = e / s
    okc = ok[:, None]
    r = np.where(okc, (p - hot) * inv_n, 0.0)
    er = np.where(okc, inv_n * (p * ep + 2 * U * np.abs(p - hot) + UNDER), 0.0)
    zy = (z * hot).sum(axis=1, keepdims=True)
    loss = np.where(okc, np.log(s) - (zy - m), 0.0)
    e_loss = np.where(okc, es + 2 * LOG_ULP * U * np.abs(np.log(s)) + 2 * Ez + U * np.abs(zy - m) + U * np.abs(loss), 0.0)
    if gW0 is None:
        g0, gb0_, e0 = l2 * W, np.zeros(C), U * np.abs(l2 * W)
    else:
        g0, gb0_, e0 = np.asarray(gW0, dtype=np.float64), np.asarray(gb0, dtype=np.float64), 0.0
    ax = np.abs(x)
    return dict(row_loss=loss[:, 0], gW=g0 + r.T @ x, gb=gb0_ + r.sum(axis=0),
                e_row_loss=e_loss[:, 0], e_gW=er.T @ ax + (N + 1) * U * (np.abs(g0) + np.abs(r).T @ ax) + e0,
                e_gb=er.sum(axis=0) + N * U * (np.abs(gb0_) + np.abs(r).sum(axis=0)))


def mismatch(got, ref):
    """None where row_loss, gW and gb of `got` (arrays or tensors) lie within the budget of reference()'s `ref`, else what differs."""
    for k in ("row_loss", "gW", "gb"):
        g = np.asarray(got[k].detach().cpu() if isinstance(got[k], torch.Tensor) else got[k], dtype=np.float64)
        if g.shape != ref[k].shape:
            return f"{k}: shape {g.shape}, expected {ref[k].shape}"
        if not np.isfinite(g).all():
            return f"{k}: {int((~np.isfinite(g)).sum())} of {g.size} entries are not finite"
        over = np.abs(g - ref[k]) - ref["e_" + k]
        if g.size and over.max() > 0:
            i = np.unravel_index(int(over.argmax()), g.shape)
            return (f"{k}: {int((over > 0).sum())} of {g.size} entries beyond the budget, the worst at {tuple(int(j) for j in i)}: got {g[i]!r}, "
                    f"expected {ref[k][i]!r}, |difference| {abs(g[i] - ref[k][i]):.3e} against a budget of {ref['e_' + k][i]:.3e}")
    return None


def worst(got, ref):
    """{name: (largest |difference|, its budget, largest difference / budget)}: what a test prints before it asserts."""
    out = {}
    for k in ("row_loss", "gW", "gb"):
        g = np.asarray(got[k].detach().cpu() if isinstance(got[k], torch.Tensor) else got[k], dtype=np.float64)
        d = np.abs(g - ref[k])
        if not d.size:
            out[k] = (0.0, 0.0, 0.0)
            continue
        i = np.unravel_index(int(d.argmax()), d.shape)
        out[k] = (float(d[i]), float(ref["e_" + k][i]), float((d / np.maximum(ref["e_" + k], 1e-300)).max()))
    return out


# ---- operands of the kernel tests ------------------------------------------------------------------------------------------------------

def operands(N, C, D, reach=None, seed=0, pad=4):
    """x fp32 [N, D] unit rows inside a buffer of row stride D + pad, labels int64 [N] a tenth of them -1 or C, W fp32 [C, D], b fp32 [C]
    non-zero.  reach: W scaled so that the largest |W x| is `reach`.  At 80 the exponentials span e^-160 .. 1 after the max subtraction
    and underflow; WITHOUT it they reach e^80 = 5.5e34, which fp32 still holds (it overflows at e^88.7) -- so the overflow case proper is
    reach = 100, and both are run."""
    g = torch.Generator().manual_seed(seed * 7919 + N * 131 + C * 17 + D)
    buf = torch.zeros((N, D + pad), dtype=torch.float32)
    x = torch.randn((N, D), generator=g)
    buf[:, :D] = x / x.norm(dim=1, keepdim=True).clamp_min(1e-6)
    x = buf[:, :D]
    W = torch.randn((C, D), generator=g)
    b = torch.randn((C,), generator=g) * 0.5 + 0.25
    if reach and N:
        W = W * (float(reach) / float((x.double() @ W.double().T).abs().max()))
    y = torch.randint(0, C, (N,), generator=g)
    bad = torch.rand((N,), generator=g) < 0.1
    y[bad] = torch.where(torch.rand((int(bad.sum()),), generator=g) < 0.5, -1, C)
    return x, y, W.contiguous(), b


# ---- honest fp32 evaluations and planted defects ---------------------------------------------------------------------------------------

DEFECTS = ("no_max", "no_minus_one", "minus_one_wrong_column", "inv_n_twice", "inv_n_missing", "bias_grad_dropped", "l2_dropped",
           "tail_dropped", "tail_clamped", "foreign_counted")
ORDERS = ("blas", "chain", "reversed", "tiles")


def model(x, y, W, b, inv_n, l2, order="blas", defect=None):
    """An fp32 evaluation in numpy: `order` picks how the sums run (blas: numpy's products; chain: row after row, the kernel's order;
    reversed: features and rows from the far end; tiles: QUANTUM rows at a time, partial sums added).  defect: one of DEFECTS."""
    f = np.float32
    x, W, b = (np.asarray(a, dtype=f) for a in (x, W, b))
    y = np.asarray(y, dtype=np.int64)
    N, D = x.shape
    C = W.shape[0]
    inv_n, l2 = f(inv_n), f(l2)
    z = (x[:, ::-1] @ W[:, ::-1].T if order == "reversed" else x @ W.T).astype(f) + b
    ok = (y >= 0) & (y < C)
    yy = np.where(ok, y, 0)
    if defect == "foreign_counted":
        ok, yy = np.ones(N, dtype=bool), np.clip(y, 0, C - 1)
    m = np.zeros((N, 1), dtype=f) if defect == "no_max" else z.max(axis=1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(z - m, dtype=f)
        s = e.sum(axis=1, keepdims=True, dtype=f)
        p = e * (f(1) / s)
        hot = np.zeros((N, C), dtype=f)
        if defect != "no_minus_one":
            hot[np.arange(N), (yy + 1) % C if defect == "minus_one_wrong_column" else yy] = 1
        scale = {"inv_n_twice": inv_n * inv_n, "inv_n_missing": f(1)}.get(defect, inv_n)
        r = ((p - hot) * scale * ok[:, None]).astype(f)
        loss = ((np.log(s, dtype=f) - (z[np.arange(N), yy][:, None] - m))[:, 0] * ok).astype(f)
    rows = np.arange(N)
    if defect == "tail_dropped":
        rows = rows[:N // QUANTUM * QUANTUM]
    if defect == "tail_clamped" and N % QUANTUM:
        rows = np.minimum(np.arange((N + QUANTUM - 1) // QUANTUM * QUANTUM), N - 1)
    r, xs = r[rows], x[rows]
    gW = np.zeros((C, D), dtype=f) if defect == "l2_dropped" else (l2 * W).astype(f)
    gb = np.zeros(C, dtype=f)
    if order == "chain":
        for n in range(len(rows)):
            gW = (gW + np.outer(r[n], xs[n]).astype(f)).astype(f)
            gb = (gb + r[n]).astype(f)
    elif order == "tiles":
        for a in range(0, len(rows), QUANTUM):
            gW = (gW + (r[a:a + QUANTUM].T @ xs[a:a + QUANTUM]).astype(f)).astype(f)
            gb = (gb + r[a:a + QUANTUM].sum(axis=0, dtype=f)).astype(f)
    elif order == "reversed":
        gW, gb = (gW + (r[::-1].T @ xs[::-1]).astype(f)).astype(f), r[::-1].sum(axis=0, dtype=f)
    else:
        gW, gb = (gW + (r.T @ xs).astype(f)).astype(f), r.sum(axis=0, dtype=f)
    if defect == "bias_grad_dropped":
        gb = np.zeros(C, dtype=f)
    return dict(row_loss=loss, gW=gW, gb=gb)


# ---- the few-shot problems of the fit tests --------------------------------------------------------------------------------------------

PROBLEMS = ((13, 5, 64, 1.0), (37, 3, 96, 1.0), (101, 4, 128, 0.8))          # C x shots x D, sep
HELD_OUT = 20                                                               # rows per class


def problem(C, shots, D, sep, seed=0):
    """-> (X fp32 [C * shots, D], y, X_held fp32 [C * HELD_OUT, D], y_held): rows sep * centroid[y] + N(0, I), normalised to unit length
    and rounded to fp16 -- what the bank holds."""
    g = torch.Generator().manual_seed(1000 * seed + C)
    cent = torch.randn((C, D), generator=g)

    def draw(per):
        y = torch.arange(C).repeat_interleave(per)
        x = sep * cent[y] + torch.randn((C * per, D), generator=g)
        return (x / x.norm(dim=1, keepdim=True)).half().float(), y
    X, y = draw(shots)
    Xh, yh = draw(HELD_OUT)
    return X, y, Xh, yh


def scalars(n_rows, c):
    """(inv_n, l2) of probe.objective_scalars, restated: the fp32 values 1 / N and 1 / (c N) the kernels are handed."""
    return float(np.float32(1.0 / n_rows)), float(np.float32(1.0 / (c * n_rows)))


def torch_loss_grad(X, y):
    """The CPU stand-in of probe.device_loss_grad for the driver's tests: fp32 torch, loss as an fp64 0-dim tensor."""
    def loss_grad(W, b, c):
        inv_n, l2 = scalars(len(y), c)
        z = X @ W.T + b
        m = z.max(dim=1, keepdim=True).values
        e = torch.exp(z - m)
        s = e.sum(dim=1, keepdim=True)
        r = e / s
        r[torch.arange(len(y)), y] -= 1.0
        r *= inv_n
        row_loss = torch.log(s[:, 0]) - (z[torch.arange(len(y)), y] - m[:, 0])
        loss = row_loss.sum(dtype=torch.float64) * inv_n + W.double().square().sum() * (0.5 * l2)
        return loss, l2 * W + r.T @ X, r.sum(dim=0)
    return loss_grad


def grad_fp64(X, y, W, b, inv_n, l2):
    """max |g| of the objective in fp64 at (W, b), and the budget of an fp32 evaluation there (largest entry of e_gW, e_gb)."""
    ref = reference(X, y, W, b, inv_n, l2)
    return max(float(np.abs(ref["gW"]).max()), float(np.abs(ref["gb"]).max())), max(float(ref["e_gW"].max()), float(ref["e_gb"].max()))
