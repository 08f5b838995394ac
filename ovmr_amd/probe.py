"""The linear probe: a multinomial logistic regression on image features, fitted on the device (DESIGN.md sections 4 and 6).

The reference fits it with scikit-learn on the CPU (lpclip/linear_probe.py); here the loss and the gradient are three launches of
libovmr_hip.so (runtime.probe_loss_grad, include/ovmr_hip_probe.h) and the optimiser below keeps its vectors on the device.

    fit            an L-BFGS driver over any callable that evaluates the objective: the device's, or a CPU stand-in in tests
    search_c       the reference's search of the regularisation strength C: a 7-point sweep, then rounds of left / right comparison
    LinearProbeState   what a fitted probe is, and its file linear_probe.pt
"""
from __future__ import annotations

import math
import os
import os.path as osp
from typing import Callable, List, NamedTuple, Optional

import numpy as np
import torch

PROBE_FORMAT = 1
PROBE_FILE = "linear_probe.pt"

SWEEP = (1e6, 1e4, 1e2, 1, 1e-2, 1e-4, 1e-6)                  # lpclip/linear_probe.py:54
VAL_SHOTS = {1: 1, 2: 2, 4: 4, 8: 4, 16: 4}                   # lpclip/linear_probe.py:25


def val_shots(shots: int) -> int:
    """Validation images per class for a probe fitted on `shots` per class: the reference's table, min(shots, 4) beyond it."""
    return VAL_SHOTS.get(int(shots), min(int(shots), 4))


def objective_scalars(n_rows: int, c: float):
    """(inv_n, l2) that make the library's objective scikit-learn's LogisticRegression(C=c) over n_rows rows divided by n_rows: 1 / N and
    1 / (c N), as the fp32 values the kernels are handed."""
    if n_rows < 1 or not c > 0 or not math.isfinite(c):
        raise ValueError(f"objective_scalars: n_rows must be positive and c a positive finite number, got {n_rows} and {c!r}")
    return float(np.float32(1.0 / n_rows)), float(np.float32(1.0 / (c * n_rows)))


def device_loss_grad(features: torch.Tensor, labels: torch.Tensor, max_bytes: Optional[int] = None) -> Callable:
    """loss_grad(W, b, c) -> (loss, gW, gb) over fixed rows on the GPU: features fp32 [N, D], labels int64 [N].  One workspace (capped at
    max_bytes: runtime.probe_workspace) and one set of outputs serve every evaluation; the outputs are overwritten by the next one."""
    from . import runtime
    N, D = features.shape
    state = {}

    def loss_grad(W, b, c):
        inv_n, l2 = objective_scalars(N, c)
        if not state:
            C = W.shape[0]
            kw = {} if max_bytes is None else dict(max_bytes=max_bytes)
            state.update(workspace=runtime.probe_workspace(N, C, D, features.device, **kw),
                         gW=torch.empty((C, D), dtype=torch.float32, device=features.device),
                         gb=torch.empty((C,), dtype=torch.float32, device=features.device),
                         row_loss=torch.empty((N,), dtype=torch.float32, device=features.device))
        loss, gW, gb, _ = runtime.probe_loss_grad(features, labels, W, b, inv_n, l2, **state)
        return loss, gW, gb
    return loss_grad


class FitResult(NamedTuple):
    W: torch.Tensor           # fp32 [C, D]
    b: torch.Tensor           # fp32 [C]
    n_iter: int
    n_eval: int
    converged: bool
    loss: float
    max_grad: float


ARMIJO = 1e-4                 # sufficient decrease
CURVATURE = 0.9               # the approximate Wolfe test's curvature factor
FLAT = 8 * 2.0 ** -24         # two losses closer than this, relatively, are equal to an fp32 evaluation
MAX_HALVINGS = 30


def fit(loss_grad: Callable, C: int, D: int, c: float, tol: float = 1e-4, max_iter: int = 1000, history: int = 10,
        device=None) -> FitResult:
    """Minimises the objective loss_grad evaluates by L-BFGS (two-loop recursion over `history` curvature pairs), from zeros as
    scikit-learn starts.  loss_grad(W, b, c) -> (loss, gW, gb): loss a 0-dim tensor, gW [C, D], gb [C], all on W's device; they may be
    overwritten by the next call.  W, b, the pairs and the direction are device tensors; the host reads back ONE vector of scalars per
    evaluation (loss, directional derivative, max |g|, |g|, and the directional derivative the step started from).

    Stops with converged = True when max |g| <= tol (scikit-learn's gtol, on the same 1 / N-scaled objective); with converged = False
    after max_iter iterations, or when the line search finds no step that decreases the loss -- at tolerances below what fp32 resolves
    the loss is noise long before the gradient is small, and a search that keeps halving would never end.  The line search backs off from
    a unit step (1 / |g| at first) until the loss has decreased sufficiently; where two losses are equal to fp32's resolution it takes the
    step whose directional derivative has risen instead (the approximate Wolfe test).  A pair with s.y <= 0 is skipped.  The point
    returned is the last accepted one: the loss never rises, so it is the best seen."""
    CD = C * D
    theta = torch.zeros(CD + C, dtype=torch.float32, device=device)
    n_eval = 0

    def evaluate(th, d, dd0):
        nonlocal n_eval
        n_eval += 1
        loss, gW, gb = loss_grad(th[:CD].view(C, D), th[CD:], c)
        g = torch.cat([gW.reshape(-1), gb.reshape(-1)])
        g64 = g.double()
        dd = (g64 * d.double()).sum() if d is not None else torch.zeros((), dtype=torch.float64, device=g.device)
        extra = dd0 if dd0 is not None else torch.zeros((), dtype=torch.float64, device=g.device)
        scalars = torch.stack([loss.double().reshape(()), dd, g64.abs().max(), g64.square().sum().sqrt(), extra]).tolist()   # the one read
        return g, scalars

    g, (f, _, gmax, gnorm, _) = evaluate(theta, None, None)
    pairs: List[tuple] = []                                       # (s, y, 1 / s.y) on the device, oldest first
    gamma = None                                                  # s.y / y.y of the newest pair, on the device
    n_iter, converged = 0, gmax <= tol
    while not converged and n_iter < max_iter and math.isfinite(f):
        q = g.clone()
        alphas = []
        for s, y, rho in reversed(pairs):
            a = rho * (s.double() * q.double()).sum()
            q -= (a * y.double()).float()
            alphas.append(a)
        if gamma is not None:
            q *= gamma.float()
        for (s, y, rho), a in zip(pairs, reversed(alphas)):
            beta = rho * (y.double() * q.double()).sum()
            q += ((a - beta) * s.double()).float()
        d = -q
        dd0_dev = (g.double() * d.double()).sum()
        t = 1.0 if pairs else min(1.0, 1.0 / max(gnorm, 1e-30))
        accepted = False
        for _ in range(MAX_HALVINGS):
            trial = theta + t * d
            g_new, (f_new, dd_new, gmax_new, gnorm_new, dd0) = evaluate(trial, d, dd0_dev)
            if not dd0 < 0:                                       # not a descent direction: the history misleads
                break
            if math.isfinite(f_new) and (f_new <= f + ARMIJO * t * dd0
                                         or (f_new <= f + FLAT * abs(f) and CURVATURE * dd0 <= dd_new <= (1 - 2 * ARMIJO) * -dd0)):
                accepted = True
                break
            t *= 0.5
        if not accepted:
            if pairs:                                             # once more from the plain gradient before giving up
                pairs, gamma = [], None
                continue
            break
        s, y = trial - theta, g_new - g
        sy = t * (dd_new - dd0)
        if sy > 0:
            sy_dev = (s.double() * y.double()).sum()
            pairs.append((s, y, 1.0 / sy_dev))
            gamma = sy_dev / y.double().square().sum()
            del pairs[:-history]
        theta, g, f, gmax, gnorm = trial, g_new, f_new, gmax_new, gnorm_new
        n_iter += 1
        converged = gmax <= tol
    return FitResult(theta[:CD].view(C, D), theta[CD:], n_iter, n_eval, bool(converged), float(f), float(gmax))


def search_c(fit_at: Callable, accuracy_at: Callable, steps: int = 8):
    """The reference's search of C (lpclip/linear_probe.py:53-118).  fit_at(c) -> a fitted probe, accuracy_at(probe) -> its validation
    accuracy.  First the sweep 1e6, 1e4 ... 1e-6; the peak is the FIRST best of it, and the bounds start a decade to either side.  Every
    round fits at both bounds and keeps the better, the LEFT one on a tie; the bounds move in log10: the loser to the midpoint, the winner
    stays -- and, as in the reference, both pass through log10 and back from the second round on, so a kept bound is 10 ** log10(c), not
    always c to the bit.  -> (c, probe, trace): the last round's choice and its probe, and per round (c_left, c_right, chosen, accuracy).
    steps == 0: the sweep's peak."""
    fitted = [fit_at(c) for c in SWEEP]
    acc = [accuracy_at(p) for p in fitted]
    peak = int(np.argmax(acc))
    c_final, final = float(SWEEP[peak]), fitted[peak]
    c_left, c_right = 1e-1 * SWEEP[peak], 1e1 * SWEEP[peak]
    trace = []
    for _ in range(int(steps)):
        left, right = fit_at(float(c_left)), fit_at(float(c_right))
        a_left, a_right = accuracy_at(left), accuracy_at(right)
        lo, hi = np.log10(c_left), np.log10(c_right)
        if a_left < a_right:
            c_final, final, a = float(c_right), right, a_right
            lo = 0.5 * (hi + lo)
        else:
            c_final, final, a = float(c_left), left, a_left
            hi = 0.5 * (hi + lo)
        trace.append((float(c_left), float(c_right), c_final, float(a)))
        c_left, c_right = np.power(10, lo), np.power(10, hi)
    return c_final, final, trace


# ---- the file ------------------------------------------------------------------------------------------------------------------------

FIELDS = ("format", "W", "b", "c", "tol", "n_iter", "converged", "classnames", "shots", "search")


class LinearProbeState:
    """A fitted probe: W fp32 [C, D], b fp32 [C], the strength c it was fitted at, the tolerance, iterations and whether the fit
    converged, the class names, the shots per class (int64 [C]) and the search trace (None for a fixed c)."""

    def __init__(self, W, b, c, tol, n_iter, converged, classnames, shots, search=None):
        self.W, self.b = W.detach().float().cpu().contiguous(), b.detach().float().cpu().contiguous()
        self.c, self.tol, self.n_iter, self.converged = float(c), float(tol), int(n_iter), bool(converged)
        self.classnames = [str(n) for n in classnames]
        self.shots = torch.as_tensor(shots, dtype=torch.int64).cpu()
        self.search = None if search is None else [tuple(float(v) for v in row) for row in search]
        self.check("LinearProbeState")

    def check(self, where: str):
        C = self.W.shape[0] if self.W.dim() == 2 else -1
        for field, ok, why in (("W", self.W.dim() == 2 and C >= 1, f"must be of shape [C, D], got {list(self.W.shape)}"),
                               ("b", tuple(self.b.shape) == (C,), f"must be of shape [{C}] as W has {C} rows, got {list(self.b.shape)}"),
                               ("classnames", len(self.classnames) == C, f"must name {C} classes as W has {C} rows, got {len(self.classnames)}"),
                               ("shots", tuple(self.shots.shape) == (C,), f"must be of shape [{C}] as W has {C} rows, got {list(self.shots.shape)}"),
                               ("c", self.c > 0 and math.isfinite(self.c), f"must be a positive finite number, got {self.c!r}")):
            if not ok:
                raise ValueError(f'"{where}": {field} {why}')

    def write(self, path: str) -> None:
        """torch.save under a scratch name next to `path`, moved into place whole (as bank.write does)."""
        d = osp.dirname(osp.abspath(path))
        os.makedirs(d, exist_ok=True)
        scratch = osp.join(d, f".partial.{os.getpid()}.{osp.basename(path)}")
        try:
            torch.save(dict(format=PROBE_FORMAT, W=self.W, b=self.b, c=self.c, tol=self.tol, n_iter=self.n_iter, converged=self.converged,
                            classnames=self.classnames, shots=self.shots, search=self.search), scratch)
            os.replace(scratch, path)
        finally:
            if osp.exists(scratch):
                os.remove(scratch)

    @classmethod
    def read(cls, path: str) -> "LinearProbeState":
        """Reads a probe with the restricted reader (checkpoint._torch_load: nothing in the file can run code).  ValueError naming the
        file and the field for a file that is not a probe, a newer format, a missing field or shapes that do not agree."""
        from . import checkpoint
        obj = checkpoint._torch_load(path)

        def refuse(field, why):
            raise ValueError(f'"{path}": {field} {why}')
        if not isinstance(obj, dict) or not isinstance(obj.get("format"), int) or isinstance(obj.get("format"), bool):
            refuse("format", "is missing: not a linear probe (a LinearProbe run writes one)")
        if obj["format"] > PROBE_FORMAT:
            refuse("format", f"is {obj['format']}, this build reads linear probes up to format {PROBE_FORMAT}")
        for k in FIELDS:
            if k not in obj:
                refuse(k, "is missing: not a linear probe")
        for k in ("W", "b", "shots"):
            if not isinstance(obj[k], torch.Tensor):
                refuse(k, f"must be a tensor, got {type(obj[k]).__name__}")
        for k, dt in (("W", torch.float32), ("b", torch.float32), ("shots", torch.int64)):
            if obj[k].dtype != dt:
                refuse(k, f"must be {dt}, got {obj[k].dtype}")
        if not isinstance(obj["classnames"], (list, tuple)):
            refuse("classnames", f"must be a list, got {type(obj['classnames']).__name__}")
        if obj["search"] is not None and not isinstance(obj["search"], (list, tuple)):
            refuse("search", f"must be a list or None, got {type(obj['search']).__name__}")
        self = cls.__new__(cls)
        self.W, self.b, self.shots = obj["W"].contiguous(), obj["b"].contiguous(), obj["shots"]
        try:
            self.c, self.tol, self.n_iter, self.converged = float(obj["c"]), float(obj["tol"]), int(obj["n_iter"]), bool(obj["converged"])
        except (TypeError, ValueError):
            refuse("c", "tol, n_iter and converged must be numbers")
        self.classnames = [str(n) for n in obj["classnames"]]
        self.search = None if obj["search"] is None else [tuple(float(v) for v in row) for row in obj["search"]]
        self.check(path)
        return self
