"""The linear probe without a GPU: the header against runtime.PROBE_SIGNATURES and the library's exports, the comparator of probe_cases.py
against honest fp32 evaluations and planted defects, the L-BFGS driver on a torch-CPU stand-in against its stop rule in fp64 and against
scikit-learn, the search of C on stubs, the Python boundary of the three wrappers, and the file."""
import contextlib
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import probe_cases as K
from conftest import REPO

# ---- the header, its table and the library ---------------------------------------------------------------------------------------------

NAMES = {"ovmr_probe_logits", "ovmr_probe_row_quantum", "ovmr_probe_workspace_bytes", "ovmr_probe_loss_grad"}


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import build, runtime
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    return runtime.load_library()


def test_probe_header_table_and_exports(lib):
    from ovmr_amd import build, runtime
    text = open(os.path.join(REPO, "include", "ovmr_hip_probe.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = dict(re.findall(r"\b(ovmr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(decls) == set(runtime.PROBE_SIGNATURES) == NAMES
    others = [runtime.SIGNATURES, runtime.EXT_SIGNATURES, runtime.AUDIT_SIGNATURES, runtime.RETRIEVE_SIGNATURES, runtime.CURVES_SIGNATURES,
              runtime.RANKS_SIGNATURES]
    assert not any(set(runtime.PROBE_SIGNATURES) & set(o) for o in others)
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    for name, params in decls.items():
        res, args = runtime.PROBE_SIGNATURES[name]
        assert hasattr(lib, name), f"{name} declared in include/ovmr_hip_probe.h but not exported"
        ps = [q.strip() for q in params.split(",")]
        want = [] if ps == ["void"] else [ctypes.c_void_p if "*" in p or "ovmr_stream" in p else ctype[p.split()[0]] for p in ps]
        assert args == want, f"{name}: {args} != {want}"
        assert res is (ctypes.c_long if name == "ovmr_probe_workspace_bytes" else ctypes.c_int)
        assert list(getattr(lib, name).argtypes or []) == args
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in NAMES:                                            # every entry point says where it stands against the reference
        mine = [c for c in comments if text.index(c) < text.index(name + "(") ][-1]
        assert "No counterpart in the reference" in mine or "lpclip/linear_probe.py" in mine, name
    flat = " ".join(re.sub(r"\n \* ?", " ", text).split())
    for phrase in ("NO FLOATING-POINT ATOMICS", "INDEPENDENT OF THE WORKSPACE", "INDEPENDENT OF HOW THE ROWS ARE CUT", "never used as an address",
                   "masked, never clamped", "v_mfma_f32_16x16x4_f32"):
        assert phrase in flat, phrase
    assert "ovmr_hip_probe.h" in inspect.getsource(build.build), "the build lists the header among its dependencies"
    assert '#include "ovmr_hip.h"' in code
    src = open(os.path.join(REPO, "ovmr_amd", "csrc", "probe.hip")).read()
    assert int(re.search(r"constexpr int PR_ROWS = (\d+);", src).group(1)) == K.QUANTUM == lib.ovmr_probe_row_quantum()
    assert "atomic" not in re.sub(r"//.*", "", src), "no atomics of any kind"
    assert "launch_gemm_f32(" in src and "EPI_BIAS" in src and "__builtin_amdgcn_mfma_f32_16x16x4f32" in src


def test_pure_functions_and_argument_errors(lib):
    f = lib.ovmr_probe_workspace_bytes
    assert f(0, 5, 32) == 0 and f(7, 5, 32) == 7 * 8 * 4 and f(7, 8, 64) == 7 * 8 * 4 and f(640_000, 10_000, 512) == 640_000 * 10_000 * 4
    for N, C, D in ((-1, 5, 32), (4, 0, 32), (4, 5, 0), (4, 5, 48), (4, 5, -32)):
        assert f(N, C, D) == -1
    E_ARG = -1
    x, y, W, b, ws, rl, gW, gb = (ctypes.c_void_p(a) for a in range(0x10000, 0x90000, 0x10000))          # never dereferenced
    ok = dict(x=x, ldx=68, y=y, N=4, C=10, D=64, W=W, b=b, acc=0, ws=ws, rl=rl, gW=gW, gb=gb)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ovmr_probe_loss_grad(a["x"], a["ldx"], a["y"], a["N"], a["C"], a["D"], a["W"], a["b"], 0.25, 0.1, a["acc"], a["ws"], a["rl"],
                                        a["gW"], a["gb"], None)

    bad = [dict(x=None), dict(y=None), dict(ws=None), dict(rl=None), dict(W=None), dict(b=None), dict(gW=None), dict(gb=None), dict(N=-1),
           dict(C=0), dict(D=0), dict(D=48), dict(ldx=60), dict(ldx=66), dict(acc=2), dict(acc=-1), dict(x=ctypes.c_void_p(0x10004)),
           dict(W=ctypes.c_void_p(0x50008)), dict(gW=ctypes.c_void_p(0x70004)), dict(ws=ctypes.c_void_p(0x40008)),
           dict(y=ctypes.c_void_p(0x20004)), dict(b=ctypes.c_void_p(0x60002)), dict(gb=ctypes.c_void_p(0x80001)), dict(rl=ctypes.c_void_p(0x50002))]
    for kw in bad:
        assert call(**kw) == E_ARG, kw
    for kw in bad[4:]:
        if "N" not in kw:
            assert call(**dict(dict(N=0, acc=1), **kw)) == E_ARG, ("N == 0 excuses no argument but the row operands", kw)
    assert call(N=0, acc=1) == 0 and call(N=0, acc=1, x=None, y=None, ws=None, rl=None) == 0, "no row, accumulate: nothing to launch"

    def logits(**kw):
        a = dict(dict(x=x, ldx=68, B=4, W=W, b=b, C=10, D=64, out=gW, ldo=10), **kw)
        return lib.ovmr_probe_logits(a["x"], a["ldx"], a["B"], a["W"], a["b"], a["C"], a["D"], a["out"], a["ldo"], None)

    for kw in (dict(x=None), dict(W=None), dict(b=None), dict(out=None), dict(B=-1), dict(C=0), dict(D=16), dict(D=80), dict(ldx=63), dict(ldx=70),
               dict(ldo=9), dict(x=ctypes.c_void_p(0x10008)), dict(out=ctypes.c_void_p(0x70002))):
        assert logits(**kw) == E_ARG, kw
        assert logits(**dict(dict(B=0), **kw)) == E_ARG, ("B == 0 excuses no argument", kw)
    assert logits(B=0) == 0


# ---- the comparator: honest evaluations pass, planted defects fail -----------------------------------------------------------------------

Q = K.QUANTUM
# name -> (N, C, D, reach): a partial last row tile (N % Q != 0, N > Q), classes that fill no tile
CASES = {"unit": (2 * Q + 3, 13, 64, None), "more classes": (Q + 1, 65, 32, None), "logits to 80": (2 * Q + 3, 13, 64, 80.0),
         "logits to 100": (2 * Q + 3, 13, 64, 100.0)}
REJECTED_ON = {d: "unit" for d in K.DEFECTS}
REJECTED_ON["no_max"] = "logits to 100"        # e^80 = 5.5e34 is still an fp32 (probe_cases.operands): the overflow case proper is 100


def _evaluate(case, order="blas", defect=None):
    N, C, D, reach = CASES[case]
    x, y, W, b = K.operands(N, C, D, reach=reach, seed=1)
    assert int(((y < 0) | (y >= C)).sum()) >= 2, "foreign labels are among the rows"
    inv_n, l2 = np.float32(1.0 / N), np.float32(0.01)
    ref = K.reference(x, y, W, b, inv_n, l2)
    got = K.model(x, y, W, b, inv_n, l2, order, defect)
    return got, ref


@pytest.mark.parametrize("order", K.ORDERS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_honest_fp32_passes_in_every_order(case, order):
    got, ref = _evaluate(case, order)
    for k, (d, e, ratio) in K.worst(got, ref).items():
        print(f"{case} / {order}: {k} worst |difference| {d:.3e}, its budget {e:.3e}, worst ratio {ratio:.3f}")
    assert K.mismatch(got, ref) is None


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_defect_is_rejected(defect):
    got, ref = _evaluate(REJECTED_ON[defect], "chain", defect)
    msg = K.mismatch(got, ref)
    assert msg is not None and ("beyond the budget" in msg or "not finite" in msg), f"{defect} passes on {REJECTED_ON[defect]!r}"


def test_defect_table_and_the_budget_is_tight_enough_to_matter():
    assert set(REJECTED_ON) == set(K.DEFECTS) and len(K.DEFECTS) == 10
    got, ref = _evaluate("unit")
    assert float(np.abs(ref["gW"]).max()) > 1e-3 and float(ref["e_gW"].max()) < 1e-3 * float(np.abs(ref["gW"]).max()), "a budget orders below the entries"
    got["gW"][3, 5] += 4 * ref["e_gW"][3, 5]
    assert "gW" in K.mismatch(got, ref)
    x, y, W, b = K.operands(5, 3, 32, seed=2)
    start = (np.ones((3, 32)), np.full(3, -2.0))
    a, z = K.reference(x, y, W, b, 0.2, 0.5, *start), K.reference(x, y, W, b, 0.2, 0.0)
    assert np.allclose(a["gW"] - 1.0, z["gW"], atol=1e-15) and np.allclose(a["gb"] + 2.0, z["gb"], atol=1e-15), "accumulate continues from its input"
    empty = K.reference(x[:0], y[:0], W, b, 1.0, 0.5)
    assert np.array_equal(empty["gW"], 0.5 * W.double().numpy()) and not empty["gb"].any() and empty["row_loss"].shape == (0,)


def test_reference_gradient_is_the_derivative():
    x, y, W, b = K.operands(9, 4, 32, seed=3)
    y = y.clamp(0, 3)
    inv_n, l2 = float(np.float32(1 / 9)), float(np.float32(0.05))

    def f(Wm, bm):
        r = K.reference(x, y, Wm, bm, inv_n, l2)
        return inv_n * r["row_loss"].sum() + 0.5 * l2 * (np.asarray(Wm, dtype=np.float64) ** 2).sum()
    ref = K.reference(x, y, W, b, inv_n, l2)
    W64, b64, h = W.double().numpy(), b.double().numpy(), 1e-6
    for (c, d) in ((0, 0), (3, 31), (2, 7)):
        Wp, Wm = W64.copy(), W64.copy()
        Wp[c, d] += h
        Wm[c, d] -= h
        assert abs((f(Wp, b64) - f(Wm, b64)) / (2 * h) - ref["gW"][c, d]) < 1e-8
    bp, bm = b64.copy(), b64.copy()
    bp[1] += h
    bm[1] -= h
    assert abs((f(W64, bp) - f(W64, bm)) / (2 * h) - ref["gb"][1]) < 1e-8


# ---- the driver ----------------------------------------------------------------------------------------------------------------------

IDS = [f"{c}x{s}x{d}" for c, s, d, _ in K.PROBLEMS]


@pytest.mark.parametrize("spec", K.PROBLEMS, ids=IDS)
def test_fit_meets_the_stop_rule_in_fp64(spec):
    from ovmr_amd import probe
    C, shots, D, _ = spec
    X, y, _, _ = K.problem(*spec)
    assert X.shape == (C * shots, D) and torch.equal(X, X.half().float()) and float((X.norm(dim=1) - 1).abs().max()) < 1e-3
    for c in (1e-2, 1.0, 1e2):
        r = probe.fit(K.torch_loss_grad(X, y), C, D, c, tol=1e-4)
        gmax, budget = K.grad_fp64(X, y, r.W, r.b, *K.scalars(len(y), c))
        print(f"{spec} c {c}: {r.n_iter} iterations, {r.n_eval} evaluations, converged {r.converged}, max |g| {r.max_grad:.3e}, in fp64 {gmax:.3e}, "
              f"budget {budget:.3e}")
        assert r.converged and r.max_grad <= 1e-4 and gmax <= 1e-4 + budget
        assert r.W.shape == (C, D) and r.b.shape == (C,) and r.W.dtype == r.b.dtype == torch.float32 and 1 <= r.n_iter < r.n_eval <= 1000


@pytest.mark.parametrize("spec", K.PROBLEMS, ids=IDS)
def test_fit_predicts_what_sklearn_predicts(spec):
    from sklearn.linear_model import LogisticRegression
    from ovmr_amd import probe
    C, shots, D, _ = spec
    X, y, Xh, _ = K.problem(*spec)
    sk = LogisticRegression(solver="lbfgs", tol=1e-10, max_iter=20000, C=1.0).fit(X.double().numpy(), y.numpy())
    z = sk.decision_function(Xh.double().numpy())
    top = np.sort(z, axis=1)
    gap = top[:, -1] - top[:, -2]
    keep = gap >= 0.05
    r = probe.fit(K.torch_loss_grad(X, y), C, D, 1.0, tol=1e-4)
    mine = Xh @ r.W.T + r.b
    print(f"{spec}: sklearn's smallest top-two gap {gap.min():.3f}, {int((~keep).sum())} of {len(gap)} rows under 0.05; sklearn {int(sk.n_iter_[0])} "
          f"iterations, the driver {r.n_iter}; largest logit difference {float((mine.double() - torch.from_numpy(z)).abs().max()):.3e}")
    assert Xh.shape == (C * K.HELD_OUT, D) and (~keep).mean() <= 0.02
    assert (mine.argmax(dim=1).numpy()[keep] == z.argmax(axis=1)[keep]).all()


def test_fit_stops_without_raising():
    from ovmr_amd import probe
    C, shots, D, _ = K.PROBLEMS[0]
    X, y, _, _ = K.problem(*K.PROBLEMS[0])
    lg = K.torch_loss_grad(X, y)
    r = probe.fit(lg, C, D, 1.0, max_iter=3)
    start = float(lg(torch.zeros((C, D)), torch.zeros(C), 1.0)[0])
    assert (r.n_iter, r.converged) == (3, False) and r.loss < start and r.max_grad > 1e-4
    assert float(lg(r.W, r.b, 1.0)[0]) == r.loss, "the point returned is the one the loss belongs to: the best seen"
    # a tolerance fp32 cannot resolve: no iteration halves for ever (each is bounded), and the fit says it did not converge
    noisy = probe.fit(lg, C, D, 1e2, tol=1e-12, max_iter=300)
    print(f"tol 1e-12: {noisy.n_iter} iterations, {noisy.n_eval} evaluations, max |g| {noisy.max_grad:.3e}")
    assert not noisy.converged and noisy.n_eval <= 1 + (noisy.n_iter + 1) * 2 * probe.MAX_HALVINGS and noisy.max_grad < 1e-4
    # a loss no step decreases (the gradient of a bowl, the loss of a hill): the line search gives up, nothing is raised
    def hill(W, b, c):
        return -0.5 * ((W.double() - 1).square().sum() + (b.double() - 1).square().sum()), W - 1, b - 1
    r = probe.fit(hill, 2, 32, 1.0)
    assert (r.n_iter, r.converged, r.n_eval) == (0, False, 1 + probe.MAX_HALVINGS) and not bool(r.W.any()) and r.max_grad == 1.0
    # a pair without positive curvature is skipped: a concave stand-in never stores one and the driver still ends
    calls = []

    def concave(W, b, c):
        calls.append(1)
        return -(W.double().square().sum() + b.double().square().sum()) - b.double().sum(), -2 * W, -2 * b - 1
    r = probe.fit(concave, 2, 32, 1.0, max_iter=5)
    assert not r.converged and r.n_iter == 5 and len(calls) == r.n_eval


def test_fit_reads_one_vector_per_evaluation(monkeypatch):
    from ovmr_amd import probe
    C, shots, D, _ = K.PROBLEMS[0]
    X, y, _, _ = K.problem(*K.PROBLEMS[0])
    reads = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (reads.append(tuple(t.shape)), real(t))[1])
    for name in ("item", "__float__", "__bool__", "numpy", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, lambda t, *a, _n=name, **k: pytest.fail(f"the driver read a tensor back through {_n}"))
    r = probe.fit(K.torch_loss_grad(X, y), C, D, 1.0)
    assert len(reads) == r.n_eval and set(reads) == {(5,)}


# ---- the search of C ---------------------------------------------------------------------------------------------------------------------

def _search(acc_of, steps):
    from ovmr_amd import probe
    fits = []
    c, model, trace = probe.search_c(lambda c: (fits.append(c), ("probe", c))[1], lambda m: acc_of(m[1]), steps=steps)
    assert model == ("probe", c)
    return c, trace, fits


def test_search_c_on_a_peak_off_the_grid():
    # accuracy 1 - |log10 c - 0.6| / 10: unimodal, the peak at c = 10^0.6 between the grid's 1 and 100.
    # Sweep (linear_probe.py:54-60): 1e6 .. 1e-6 give 0.46, 0.66, 0.86, 0.94, 0.74, 0.54, 0.34 -> the peak is 1 (index 3), and the bounds
    # start at 0.1 and 10 (:67).
    # Round 1: left 0.1 -> 0.84, right 10 -> 0.96: right wins (:81-86): left <- the midpoint (0 in log10), right stays at 1 -> [1, 10].
    # Round 2: left 1 -> 0.94, right 10 -> 0.96: right wins: left <- 0.5, right stays                                  -> [10^0.5, 10].
    # Round 3: left 10^0.5 -> 0.99, right 10 -> 0.96: left wins (:87-92): right <- the midpoint 0.75, left stays   -> [10^0.5, 10^0.75].
    # Round 4: left 10^0.5 -> 0.99, right 10^0.75 -> 0.985: left wins: right <- 0.625                               -> [10^0.5, 10^0.625].
    acc = lambda c: 1 - abs(np.log10(c) - 0.6) / 10             # noqa: E731
    c, trace, fits = _search(acc, 4)
    assert fits[:7] == [1e6, 1e4, 1e2, 1, 1e-2, 1e-4, 1e-6] and len(fits) == 7 + 2 * 4
    want = [(0.1, 10.0, 10.0), (1.0, 10.0, 10.0), (10 ** 0.5, 10.0, 10 ** 0.5), (10 ** 0.5, 10 ** 0.75, 10 ** 0.5)]
    for (cl, cr, chosen, a), (wl, wr, wc) in zip(trace, want):
        assert abs(np.log10(cl) - np.log10(wl)) < 1e-12 and abs(np.log10(cr) - np.log10(wr)) < 1e-12 and chosen in (cl, cr)
        assert abs(np.log10(chosen) - np.log10(wc)) < 1e-12 and a == acc(chosen)
    assert c == trace[-1][2] and fits[7:] == [v for row in trace for v in row[:2]], "every round fits at its two bounds, left first"
    # the quirk (:85-86, :91-92, :106-107): the first round's bounds are the products 0.1 * peak and 10 * peak as they are; from the second
    # round on BOTH bounds went through log10 and np.power(10, .), the kept one too
    assert trace[0][:2] == (1e-1 * 1, 1e1 * 1)
    assert trace[1][0] == float(np.power(10, 0.5 * (np.log10(10.0) + np.log10(0.1)))) and trace[1][1] == float(np.power(10, np.log10(10.0)))
    assert trace[3][0] == float(np.power(10, np.log10(trace[2][0]))), "a kept bound is 10 ** log10(c)"
    lo = 0.1 * 1e-2                                              # where it shows: 10 ** log10(0.001) is not 0.001 to the bit
    assert float(np.power(10, np.log10(lo))) != lo or float(np.power(10, np.log10(1e-3))) == 1e-3


def test_search_c_on_a_plateau_goes_left():
    # accuracy 0.5 everywhere: np.argmax takes the FIRST best of the sweep, 1e6 (:65), so the bounds start at 1e5 and 1e7.  Every round is a
    # tie, and `if acc_left < acc_right` (:81) is false on a tie: the left bound is chosen and kept, the right moves to the midpoint:
    # log10 bounds [5, 7] -> [5, 6] -> [5, 5.5] -> [5, 5.25].
    c, trace, fits = _search(lambda c: 0.5, 3)
    assert fits[7] == 1e-1 * 1e6 and fits[8] == 1e1 * 1e6
    assert [round(float(np.log10(r[1])), 9) for r in trace] == [7.0, 6.0, 5.5] and all(abs(np.log10(r[0]) - 5) < 1e-12 for r in trace)
    assert all(r[2] == r[0] and r[3] == 0.5 for r in trace) and c == trace[-1][0]
    c0, trace0, fits0 = _search(lambda c: 0.5, 0)
    assert (c0, trace0, len(fits0)) == (1e6, [], 7), "no round: the sweep's peak"
    # a plateau with a step: 0.9 for c >= 1, else 0.1 -> the first best of the sweep is still 1e6
    c, trace, _ = _search(lambda c: 0.9 if c >= 1 else 0.1, 2)
    assert trace[0][:3] == (1e5, 1e7, 1e5)


def test_validation_shots_follow_the_reference():
    from ovmr_amd import probe
    assert [probe.val_shots(s) for s in (1, 2, 4, 8, 16)] == [1, 2, 4, 4, 4] and [probe.val_shots(s) for s in (3, 5, 64)] == [3, 4, 4]
    assert probe.objective_scalars(80, 2.0) == K.scalars(80, 2.0) == (float(np.float32(1 / 80)), float(np.float32(1 / 160)))
    with pytest.raises(ValueError, match="objective_scalars"):
        probe.objective_scalars(80, 0.0)


# ---- the Python boundary ---------------------------------------------------------------------------------------------------------------

class _Recorder:
    """Stands where the library stands: the pure functions answer as the header says, every other call is recorded and says yes."""

    def __init__(self):
        self.calls = []

    def ovmr_probe_row_quantum(self):
        return K.QUANTUM

    def ovmr_probe_workspace_bytes(self, N, C, D):
        return -1 if N < 0 or C < 1 or D < 32 or D % 32 else 4 * N * ((C + 3) // 4 * 4)

    def __getattr__(self, name):
        if not name.startswith("ovmr_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def stub(monkeypatch):
    from ovmr_amd import runtime
    rec, log, ptrs = _Recorder(), [], []
    real_ptr = runtime._ptr
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    monkeypatch.setattr(runtime, "_same_device", lambda a, b: True)
    monkeypatch.setattr(runtime, "_ptr", lambda t: (ptrs.append(t), real_ptr(t))[1])
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: (log.append("stream"), SimpleNamespace(cuda_stream=0))[1])
    return SimpleNamespace(rec=rec, log=log, ptrs=ptrs, runtime=runtime)


def _al(shape, dtype=torch.float32):
    """A tensor whose first element is 16-byte aligned."""
    n = int(np.prod(shape))
    raw = torch.zeros(n + 4, dtype=dtype)
    off = (-raw.data_ptr() // raw.element_size()) % (16 // raw.element_size())
    return raw[off:off + n].view(shape)


def _ok(N=6, C=10, D=64):
    return dict(x=_al((N, D)), labels=torch.zeros(N, dtype=torch.int64), W=_al((C, D)), b=torch.zeros(C), inv_n=1.0 / max(N, 1), l2=0.01,
                workspace=_al((N * 12,)))


def _off(shape):
    return _al((int(np.prod(shape)) + 4,))[1:1 + int(np.prod(shape))].view(shape)


GRAD_VIOLATIONS = [
    ("x", "fp16", lambda: dict(x=_al((6, 64), torch.float16))),
    ("x", "fp64", lambda: dict(x=_al((6, 64), torch.float64))),
    ("x", "three dimensions", lambda: dict(x=_al((6, 2, 32)))),
    ("x", "D % 32 != 0", lambda: dict(x=_al((6, 48)), W=_al((10, 48)))),
    ("x", "no column", lambda: dict(x=_al((6, 0)), W=_al((10, 0)))),
    ("x", "ldx < D (an expanded row)", lambda: dict(x=_al((1, 64)).expand(6, 64))),
    ("x", "a column stride", lambda: dict(x=_al((6, 128))[:, ::2])),
    ("x", "ldx % 4 != 0", lambda: dict(x=_al((6, 66))[:, :64])),
    ("x", "misaligned", lambda: dict(x=_off((6, 64)))),
    ("x", "a numpy array", lambda: dict(x=np.zeros((6, 64), dtype=np.float32))),
    ("labels", "int32", lambda: dict(labels=torch.zeros(6, dtype=torch.int32))),
    ("labels", "a row short", lambda: dict(labels=torch.zeros(5, dtype=torch.int64))),
    ("labels", "strided", lambda: dict(labels=torch.zeros(12, dtype=torch.int64)[::2])),
    ("W", "[C, D + 32]", lambda: dict(W=_al((10, 96)))),
    ("W", "flat", lambda: dict(W=_al((640,)))),
    ("W", "fp16", lambda: dict(W=_al((10, 64), torch.float16))),
    ("W", "strided", lambda: dict(W=_al((10, 128))[:, :64])),
    ("W", "no row", lambda: dict(W=_al((0, 64)), b=torch.zeros(0))),
    ("W", "misaligned", lambda: dict(W=_off((10, 64)))),
    ("b", "C + 1 entries", lambda: dict(b=torch.zeros(11))),
    ("b", "fp64", lambda: dict(b=torch.zeros(10, dtype=torch.float64))),
    ("workspace", "too small", lambda: dict(workspace=_al((6 * 12 - 1,)), x=_al((6, 64)))),
    ("workspace", "fp16", lambda: dict(workspace=_al((144,), torch.float16))),
    ("workspace", "two dimensions", lambda: dict(workspace=_al((6, 12)))),
    ("workspace", "misaligned", lambda: dict(workspace=_off((80,)))),
    ("gW", "[D, C]", lambda: dict(gW=_al((64, 10)))),
    ("gW", "misaligned", lambda: dict(gW=_off((10, 64)))),
    ("gb", "C - 1 entries", lambda: dict(gb=torch.zeros(9))),
    ("row_loss", "fp64", lambda: dict(row_loss=torch.zeros(6, dtype=torch.float64))),
    ("inv_n", "negative", lambda: dict(inv_n=-1.0)),
    ("l2", "nan", lambda: dict(l2=float("nan"))),
    ("l2", "a tensor", lambda: dict(l2=torch.zeros(()))),
]


@pytest.mark.parametrize("arg,what,make", GRAD_VIOLATIONS, ids=[f"{a}: {w}" for a, w, _ in GRAD_VIOLATIONS])
def test_loss_grad_violation_is_refused_before_anything_reaches_the_library(arg, what, make, stub):
    with pytest.raises(ValueError) as err:
        stub.runtime.probe_loss_grad(**dict(_ok(), **make()))
    msg = str(err.value)
    assert msg.startswith("probe_loss_grad: ") and re.search(rf"(?<![\w]){re.escape(arg)}(?![\w\[])", msg), msg
    assert "must be" in msg and "got" in msg, msg
    assert stub.rec.calls == [] and stub.log == [] and stub.ptrs == [], (stub.rec.calls, stub.log)


LOGIT_VIOLATIONS = [(a, w, m) for a, w, m in GRAD_VIOLATIONS if a in ("x", "W", "b")] + [
    ("out", "fp16", lambda: dict(out=torch.zeros((6, 10), dtype=torch.float16))),
    ("out", "a row short", lambda: dict(out=torch.zeros((5, 10)))),
    ("out", "a column stride", lambda: dict(out=torch.zeros((6, 20))[:, ::2])),
    ("out", "transposed", lambda: dict(out=torch.zeros((10, 6)).T)),
]


@pytest.mark.parametrize("arg,what,make", LOGIT_VIOLATIONS, ids=[f"{a}: {w}" for a, w, _ in LOGIT_VIOLATIONS])
def test_logits_violation_is_refused_before_anything_reaches_the_library(arg, what, make, stub):
    ok = {k: v for k, v in _ok().items() if k in ("x", "W", "b")}
    with pytest.raises(ValueError) as err:
        stub.runtime.probe_logits(**dict(ok, **make()))
    msg = str(err.value)
    assert msg.startswith("probe_logits: ") and re.search(rf"(?<![\w]){re.escape(arg)}(?![\w\[])", msg) and "must be" in msg and "got" in msg, msg
    assert stub.rec.calls == [] and stub.log == [] and stub.ptrs == []


def test_workspace_violations(stub):
    rt = stub.runtime
    for kw, arg in ((dict(N=-1, C=10, D=64), "N"), (dict(N=4, C=0, D=64), "C"), (dict(N=4, C=10, D=48), "D"), (dict(N=4.0, C=10, D=64), "N")):
        with pytest.raises(ValueError, match=rf"probe_workspace: {arg} must be"):
            rt.probe_workspace(device="cpu", **kw)
    assert stub.rec.calls == [] and stub.ptrs == []
    assert rt.probe_workspace(6, 10, 64, "cpu").numel() == 6 * 12 and rt.PROBE_WORKSPACE_CAP == 1 << 30
    assert rt.probe_rows_per_call(640_000, 10_000, 512) == (1 << 30) // (40_000 * 32) * 32 == 26_816, "10 000 classes x 64 shots: cut under 1 GiB"
    assert rt.probe_rows_per_call(16_000, 1000, 512) == 16_000 and rt.probe_rows_per_call(100, 10, 64, max_bytes=1) == 32


def test_device_mismatch_is_refused(monkeypatch):
    from ovmr_amd import runtime
    rec = _Recorder()
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    with pytest.raises(ValueError, match="probe_loss_grad: x must be on cuda"):
        runtime.probe_loss_grad(**_ok())
    with pytest.raises(ValueError, match="probe_logits: x must be on cuda"):
        runtime.probe_logits(_al((6, 64)), _al((10, 64)), torch.zeros(10))
    monkeypatch.setattr(runtime, "_same_device", lambda a, b: b == "cuda" or torch.device(b).type == a.type)
    for name in ("labels", "W", "b", "workspace"):
        a = _ok()
        a[name] = a[name].to("meta")
        with pytest.raises(ValueError, match=rf"probe_loss_grad: {name} must be on cpu"):
            runtime.probe_loss_grad(**a)
    assert rec.calls == []


def test_accepted_calls_hand_over_what_the_header_asks(stub, lib):
    rt = stub.runtime
    a = _ok()
    wide = _al((8, 72))
    a["x"] = wide[1:7, 4:68]                                     # a window of a wider matrix: 16 bytes in, rows 72 apart
    loss, gW, gb, row_loss = rt.probe_loss_grad(**a)
    (name, g), = stub.rec.calls
    assert name == "ovmr_probe_loss_grad" and len(g) == 16
    assert g[0].value == a["x"].data_ptr() and g[1] == 72 and g[2].value == a["labels"].data_ptr() and g[3:6] == (6, 10, 64)
    assert g[6].value == a["W"].data_ptr() and g[7].value == a["b"].data_ptr() and g[8:11] == (a["inv_n"], 0.01, 0)
    assert g[11].value == a["workspace"].data_ptr() and g[12].value == row_loss.data_ptr() and g[13].value == gW.data_ptr() and g[14].value == gb.data_ptr()
    assert gW.shape == (10, 64) and gb.shape == (10,) and row_loss.shape == (6,) and loss.dtype == torch.float64 and loss.dim() == 0
    assert a["workspace"].numel() * 4 == lib.ovmr_probe_workspace_bytes(6, 10, 64), "the workspace covers what the header derives"
    assert {t.data_ptr() for t in stub.ptrs} == {v.value for v in g if isinstance(v, ctypes.c_void_p) and v.value}, "every address went through runtime._ptr"
    # a workspace of one quantum for 70 rows: three calls, the later ones continuing
    stub.rec.calls.clear()
    b = _ok(N=70)
    b["workspace"] = _al((K.QUANTUM * 12 + 5,))
    out = dict(gW=_al((10, 64)), gb=torch.zeros(10), row_loss=torch.zeros(70))
    rt.probe_loss_grad(**b, **out)
    calls = [g for _, g in stub.rec.calls]
    assert [(g[3], g[10]) for g in calls] == [(32, 0), (32, 1), (6, 1)]
    assert [g[0].value for g in calls] == [b["x"][n:].data_ptr() for n in (0, 32, 64)] and [g[2].value for g in calls] == [b["labels"][n:].data_ptr() for n in (0, 32, 64)]
    assert [g[12].value for g in calls] == [out["row_loss"][n:].data_ptr() for n in (0, 32, 64)]
    assert all(g[11].value == b["workspace"].data_ptr() and g[13].value == out["gW"].data_ptr() and g[14].value == out["gb"].data_ptr() for g in calls)
    # no row: one call for the start, with no row operand
    stub.rec.calls.clear()
    rt.probe_loss_grad(**dict(_ok(N=0), workspace=None))
    g = stub.rec.calls[0][1]
    assert len(stub.rec.calls) == 1 and g[0] is None and g[2] is None and g[3] == 0 and g[10] == 0 and g[11] is None and g[12] is None
    # the scores
    stub.rec.calls.clear()
    buf = torch.zeros((8, 16))
    got = rt.probe_logits(a["x"], a["W"], a["b"], out=buf[1:7, 2:12])
    (name, g), = stub.rec.calls
    assert name == "ovmr_probe_logits" and g[0].value == a["x"].data_ptr() and g[1:3] == (72, 6) and g[5:7] == (10, 64)
    assert g[7].value == buf[1:, 2:].data_ptr() == got.data_ptr() and g[8] == 16
    stub.rec.calls.clear()
    assert rt.probe_logits(_al((0, 64)), a["W"], a["b"]).shape == (0, 10) and stub.rec.calls == [], "an empty batch launches nothing"


# ---- the file ------------------------------------------------------------------------------------------------------------------------

def _state(C=5, D=32, search=None):
    from ovmr_amd.probe import LinearProbeState
    g = torch.Generator().manual_seed(0)
    return LinearProbeState(torch.randn((C, D), generator=g), torch.randn((C,), generator=g), 0.5, 1e-4, 17, True, [f"class {i}" for i in range(C)],
                            [4] * C, search)


def test_file_round_trips_through_the_restricted_reader(tmp_path, monkeypatch):
    from ovmr_amd import checkpoint, probe
    path = str(tmp_path / "out" / probe.PROBE_FILE)
    s = _state(search=[(0.1, 10.0, 10.0, 0.75), (1.0, 10.0, 1.0, 0.8)])
    s.write(path)
    assert os.listdir(tmp_path / "out") == ["linear_probe.pt"], "no scratch file stays behind"
    used = []
    real = checkpoint._torch_load
    monkeypatch.setattr(checkpoint, "_torch_load", lambda p: (used.append(p), real(p))[1])
    r = probe.LinearProbeState.read(path)
    assert used == [path]
    assert torch.equal(r.W, s.W) and torch.equal(r.b, s.b) and r.W.dtype == torch.float32 and torch.equal(r.shots, s.shots) and r.shots.dtype == torch.int64
    assert (r.c, r.tol, r.n_iter, r.converged, r.classnames, r.search) == (0.5, 1e-4, 17, True, s.classnames, s.search)
    raw = torch.load(path, weights_only=True)
    assert set(raw) == set(probe.FIELDS) and raw["format"] == probe.PROBE_FORMAT == 1
    _state().write(path)
    assert probe.LinearProbeState.read(path).search is None


def test_file_refusals_name_file_and_field(tmp_path):
    from ovmr_amd import probe
    path = str(tmp_path / probe.PROBE_FILE)
    _state().write(path)
    good = torch.load(path, weights_only=True)

    def refused(change, field, why):
        obj = dict(good)
        change(obj)
        torch.save(obj, path)
        with pytest.raises(ValueError) as err:
            probe.LinearProbeState.read(path)
        assert str(err.value).startswith(f'"{path}": {field} ') and why in str(err.value), str(err.value)

    refused(lambda o: o.update(format=2), "format", "is 2, this build reads linear probes up to format 1")
    refused(lambda o: o.pop("format"), "format", "is missing")
    refused(lambda o: o.update(b=torch.zeros(4)), "b", "as W has 5 rows")
    refused(lambda o: o.update(W=torch.zeros((6, 32))), "b", "as W has 6 rows")
    refused(lambda o: o.update(W=torch.zeros(160)), "W", "must be of shape [C, D]")
    refused(lambda o: o.update(classnames=["a"] * 4), "classnames", "must name 5 classes")
    refused(lambda o: o.update(shots=torch.zeros(6, dtype=torch.int64)), "shots", "as W has 5 rows")
    refused(lambda o: o.update(W=good["W"].double()), "W", "must be torch.float32")
    refused(lambda o: o.update(c=-1.0), "c", "positive finite")
    for field in ("W", "b", "c", "tol", "n_iter", "converged", "classnames", "shots", "search"):
        refused(lambda o, f=field: o.pop(f), field, "is missing")
    torch.save([1, 2, 3], path)
    with pytest.raises(ValueError, match="format is missing: not a linear probe"):
        probe.LinearProbeState.read(path)
    with pytest.raises(ValueError, match="classnames must name 5 classes"):
        probe.LinearProbeState(good["W"], good["b"], 1.0, 1e-4, 3, True, ["a"], [1] * 5)


# ---- the runner --------------------------------------------------------------------------------------------------------------------------

def test_runner_refusals(tmp_path):
    from ovmr_amd import cli, config
    w = ["--clip-weights", "clip.pt"]
    lp = w + ["--eval-only", "--trainer", "LinearProbe"]
    assert cli.check_probe(cli.parse(lp), "LinearProbe") == (1.0, None) and cli.PROBE_TRAINER == "LinearProbe"
    assert cli.check_probe(cli.parse(lp + ["--probe-c", "0.25"]), "LinearProbe") == (0.25, None)
    assert cli.check_probe(cli.parse(lp + ["--probe-c", "search", "--probe-val-split", "val"]), "LinearProbe") == ("search", 8)
    assert cli.check_probe(cli.parse(lp + ["--probe-c", "search", "--probe-val-split", "val", "--probe-steps", "3"]), "LinearProbe") == ("search", 3)
    assert cli.check_probe(cli.parse(w), "MM_CLS_OP") == (None, None)
    probe_file = tmp_path / "linear_probe.pt"
    probe_file.write_bytes(b"")
    assert cli.check_probe(cli.parse(lp + ["--probe", str(probe_file)]), "LinearProbe") == (None, None)
    for argv, msg in (
            (lp + ["--probe-steps", "4"], "--probe-steps N belongs to --probe-c search: the rounds of its left / right comparison"),
            (lp + ["--probe-c", "2", "--probe-steps", "4"], "--probe-steps N belongs to --probe-c search: the rounds of its left / right comparison"),
            (lp + ["--probe", str(probe_file), "--probe-c", "1"], "--probe FILE installs a fitted probe: not together with --probe-c, which fits one"),
            (lp + ["--probe-val-split", "val"], "--probe-val-split NAME belongs to --probe-c search: the split that scores its candidates"),
            (lp + ["--probe-c", "search"], "--probe-c search needs --probe-val-split NAME: the split that scores its candidates"),
            (lp + ["--predict", "pics", "--nearest", "2"], "--nearest / --audit-bank: --trainer LinearProbe keeps no exemplar features to search (MM_CLS_OP only)"),
            (lp + ["--audit-bank"], "--nearest / --audit-bank: --trainer LinearProbe keeps no exemplar features to search (MM_CLS_OP only)"),
            (lp + ["--save-bank"], "--save-bank: --trainer LinearProbe generates no vocabulary (MM_CLS_OP only)"),
            (lp + ["--probe", str(tmp_path / "gone.pt")], f"--probe {str(tmp_path / 'gone.pt')!r}: no such file"),
            (lp + ["--probe", str(probe_file), "--bank", "b.pt"], "--probe FILE installs a fitted probe: not together with --bank, which is fitted from"),
            (lp + ["--probe-c", "0"], "--probe-c 0: VALUE must be a positive number, or `search`"),
            (lp + ["--probe-c", "-2"], "--probe-c -2: VALUE must be a positive number, or `search`"),
            (lp + ["--probe-c", "nan"], "--probe-c nan: VALUE must be a positive number, or `search`"),
            (lp + ["--probe-c", "many"], "--probe-c many: VALUE must be a positive number, or `search`"),
            (lp + ["--probe-c", "search", "--probe-val-split", "val", "--probe-steps", "-1"], "--probe-steps -1: N must lie in [0, 64]")):
        with pytest.raises(SystemExit) as err:
            cli.check_probe(cli.parse(argv), "LinearProbe")
        assert str(err.value) == msg
    for flag in (["--probe-c", "1"], ["--probe-val-split", "val"], ["--probe-steps", "2"], ["--probe", str(probe_file)]):
        for name in ("MM_CLS_OP", "ZeroshotCLIP"):
            with pytest.raises(SystemExit) as err:
                cli.check_probe(cli.parse(w + flag), name)
            assert str(err.value) == f"{flag[0]} belongs to --trainer LinearProbe: the logistic regression on the exemplars' image features"
    # main refuses before anything is listed or loaded: the paths do not exist, the weights do not exist
    for argv, msg in ((lp + ["--probe-steps", "4"], "--probe-steps N belongs to --probe-c search"),
                      (w + ["--eval-only", "--trainer", "MM_CLS_OP", "--probe-c", "1"], "--probe-c belongs to --trainer LinearProbe"),
                      (lp + ["--score-curves"], "--trainer LinearProbe returns logits, which have no natural range: give --score-range LO HI"),
                      (w + ["--trainer", "LinearProbe"], "are on the hot path")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(argv)
    # the plan
    base = ["--clip-weights", "none.pt", "--root", "nowhere", "--eval-only", "--trainer", "LinearProbe"]
    tail = ["DATASET.NUM_SHOTS", "2"]
    for extra, want in (([], ("test", "probe-fit", 1.0, None, False)), (["--probe-c", "search", "--probe-val-split", "v"], ("test", "probe-fit", "search", 8, False)),
                        (["--probe", str(probe_file)], ("test", "probe-file", None, None, True)), (["--eval_mode", "all"], ("test", "probe-fit", 1.0, None, False))):
        args = cli.parse(base + extra + tail)
        p = cli.plan_job(args, config.setup_cfg(args))
        assert (p.mode, p.vocabulary, p.probe_c, p.probe_steps, p.lift_shots) == want and p.probe and not p.zeroshot and not p.skip
    args = cli.parse(["--clip-weights", "none.pt", "--root", "nowhere", "--eval-only", "--trainer", "MM_CLS_OP"] + tail)
    p = cli.plan_job(args, config.setup_cfg(args))
    assert (p.probe, p.probe_c, p.probe_steps, p.vocabulary) == (False, None, None, "generate")
    from ovmr_amd import trainer
    assert trainer.TRAINER_REGISTRY["LinearProbe"] is trainer.LinearProbe and issubclass(trainer.LinearProbe, trainer._EvalTrainer)
