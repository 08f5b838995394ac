"""The linear probe's kernels on the GPU (`pytest -m gpu`), through the C ABI of include/ovmr_hip_probe.h: ovmr_probe_loss_grad against
the fp64 statement of probe_cases.py under its derived budget, the properties the header promises (bit-equal on a repeat, over any
workspace contents and over any cut of the rows at the quantum; guards untouched; C == 1; N == 0), ovmr_probe_logits against the fp32
GEMM it must be, and the L-BFGS fit on the device under the bounds of the CPU test."""
import ctypes

import numpy as np
import pytest
import torch

import poison
import probe_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def rt():
    from ovmr_amd import runtime
    runtime.load_library()
    return runtime


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _call(rt, x, y, W, b, inv_n, l2, accumulate, ws, row_loss, gW, gb):
    N, D = x.shape
    rc = rt.load_library().ovmr_probe_loss_grad(_p(x), x.stride(0) if N > 1 else max(D, x.stride(0)), _p(y), N, W.shape[0], D, _p(W), _p(b),
                                                float(inv_n), float(l2), int(accumulate), _p(ws), _p(row_loss), _p(gW), _p(gb), rt._stream())
    assert rc == 0, rc


def _device(x, y, W, b):
    """The operands on the GPU: x keeps its padded row stride."""
    N, D = x.shape
    buf = torch.zeros((max(N, 1), x.stride(0) if N > 1 else D + 4), dtype=torch.float32, device=DEV)
    buf[:N, :D] = x
    return buf[:N, :D], y.to(DEV), W.to(DEV), b.to(DEV)


def _workspace(rt, N, C, D):
    n = rt.load_library().ovmr_probe_workspace_bytes(N, C, D)
    assert n == 4 * N * ((C + 3) // 4 * 4)
    return torch.empty(max(n // 4, 4), dtype=torch.float32, device=DEV)


def _run(rt, x, y, W, b, inv_n, l2, start=None, ws=None):
    """One call on device operands -> dict of row_loss, gW, gb.  start = (gW0, gb0): accumulate = 1 from them."""
    N, D = x.shape
    C = W.shape[0]
    ws = _workspace(rt, N, C, D) if ws is None else ws
    row_loss = torch.full((N,), 7.0, dtype=torch.float32, device=DEV)
    if start is None:
        gW, gb = (poison.fill_(torch.empty(s, dtype=torch.float32, device=DEV), "ones") for s in ((C, D), (C,)))
    else:
        gW, gb = start[0].clone(), start[1].clone()
    _call(rt, x, y, W, b, inv_n, l2, start is not None, ws, row_loss, gW, gb)
    return dict(row_loss=row_loss, gW=gW, gb=gb)


Q = K.QUANTUM
# (N, C, D): every N of {1, 5, 63, 65, q + 1, 2q + 3}, every C of {1, 2, 13, 65, 130}, every D of {32, 96, 512}, the two corners, and one
# shape whose class tiles are 64 wide (at least 256 of them: csrc/probe.hip, PR_SMALL_GRID) with a partial last tile
SHAPES = [(1, 1, 32), (5, 2, 96), (63, 13, 32), (65, 65, 96), (Q + 1, 130, 32), (2 * Q + 3, 130, 512), (2 * Q + 3, 13, 512), (5, 65, 512),
          (2 * Q + 3, 1990, 512)]


def test_quantum_is_the_cases(rt):
    assert rt.load_library().ovmr_probe_row_quantum() == Q


@pytest.mark.parametrize("reach", [None, 80.0, 100.0], ids=["unit", "logits to 80", "logits to 100"])
@pytest.mark.parametrize("N,C,D", SHAPES)
def test_loss_grad_against_fp64(rt, N, C, D, reach):
    x, y, W, b = K.operands(N, C, D, reach=reach, seed=1)
    if reach:
        assert abs(float((x.double() @ W.double().T).abs().max()) - reach) < 1e-3
    inv_n, l2 = np.float32(1.0 / max(N, 1)), np.float32(0.01)
    dx, dy, dW, db = _device(x, y, W, b)
    g = torch.Generator().manual_seed(5)
    start = (torch.randn((C, D), generator=g) * 0.01, torch.randn((C,), generator=g) * 0.01)
    for s in (None, start):
        got = _run(rt, dx, dy, dW, db, inv_n, l2, None if s is None else tuple(t.to(DEV) for t in s))
        ref = K.reference(x, y, W, b, inv_n, l2, *(s or (None, None)))
        for k, (d, e, ratio) in K.worst(got, ref).items():
            print(f"N {N} C {C} D {D} reach {reach} accumulate {s is not None}: {k} worst |difference| {d:.3e}, its budget {e:.3e}, worst ratio {ratio:.3f}")
        assert K.mismatch(got, ref) is None
        bad = (y < 0) | (y >= C)
        assert bool((got["row_loss"].cpu()[bad] == 0).all()), "a foreign label: loss exactly 0"


def _big_case(rt):
    N, C, D = 2 * Q + 3, 130, 96
    x, y, W, b = K.operands(N, C, D, seed=2)
    return (N, C, D) + _device(x, y, W, b)


def _same(a, b):
    for k in ("row_loss", "gW", "gb"):
        msg = poison.same_bits(a[k], b[k])
        assert msg is None, f"{k}: {msg}"


def test_repeat_and_workspace_contents(rt):
    N, C, D, x, y, W, b = _big_case(rt)
    first = _run(rt, x, y, W, b, 1.0 / N, 0.01)
    _same(first, _run(rt, x, y, W, b, 1.0 / N, 0.01))
    for fill in poison.FILLS:
        ws = poison.fill_(_workspace(rt, N, C, D), fill)
        _same(first, _run(rt, x, y, W, b, 1.0 / N, 0.01, ws=ws))
    start = (torch.full((C, D), 0.25, device=DEV), torch.full((C,), -0.5, device=DEV))
    again = _run(rt, x, y, W, b, 1.0 / N, 0.01, start)
    for fill in poison.FILLS:
        _same(again, _run(rt, x, y, W, b, 1.0 / N, 0.01, start, ws=poison.fill_(_workspace(rt, N, C, D), fill)))


@pytest.mark.parametrize("C,D", [(130, 96), (1990, 512)], ids=["32-class tiles", "64-class tiles"])
def test_two_calls_at_every_quantum_equal_one(rt, C, D):
    N = 2 * Q + 3
    x, y, W, b = _device(*K.operands(N, C, D, seed=3))
    whole = _run(rt, x, y, W, b, 1.0 / N, 0.01)
    for n1 in range(Q, N, Q):
        head = _run(rt, x[:n1], y[:n1], W, b, 1.0 / N, 0.01)
        tail = _run(rt, x[n1:], y[n1:], W, b, 1.0 / N, 0.01, (head["gW"], head["gb"]))
        _same(whole, dict(row_loss=torch.cat([head["row_loss"], tail["row_loss"]]), gW=tail["gW"], gb=tail["gb"]))


def test_wrapper_cuts_the_rows_under_a_cap(rt):
    N, C, D, x, y, W, b = _big_case(rt)
    whole = _run(rt, x, y, W, b, np.float32(1.0 / N), np.float32(0.01))
    per_row = rt.load_library().ovmr_probe_workspace_bytes(1, C, D)
    for cap in (per_row * Q, per_row * (Q + 5), per_row * 2 * Q, 1):
        ws = rt.probe_workspace(N, C, D, x.device, max_bytes=cap)
        assert ws.numel() * 4 == per_row * (2 * Q if cap == per_row * 2 * Q else Q), "whole quanta, at least one"
        loss, gW, gb, row_loss = rt.probe_loss_grad(x, y, W, b, float(np.float32(1.0 / N)), float(np.float32(0.01)), workspace=ws)
        _same(whole, dict(row_loss=row_loss, gW=gW, gb=gb))
        want = whole["row_loss"].double().sum() * float(np.float32(1.0 / N)) + W.double().square().sum() * (0.5 * float(np.float32(0.01)))
        assert loss.dtype == torch.float64 and loss.is_cuda and float(loss) == float(want)


def test_guards_stay_untouched(rt):
    N, C, D = 2 * Q + 3, 13, 32
    x, y, W, b = K.operands(N, C, D, seed=4)
    for fill in ("nan16", "big"):
        arena = poison.Arena(fill, DEV, guard=poison.guard_elems(D + 4))
        xb = arena.take(N * (D + 4), "f32").view(N, D + 4)
        xb[:, :D] = x.to(DEV)
        dy, dW, db = arena.place(y.to(DEV)), arena.place(W.to(DEV)), arena.place(b.to(DEV))
        gW, gb, row_loss = arena.take(C * D, "f32").view(C, D), arena.take(C, "f32"), arena.take(N, "f32")
        ws = arena.take(N * 16, "f32")
        for acc in (0, 1):
            _call(rt, xb[:, :D], dy, dW, db, 1.0 / N, 0.01, acc, ws, row_loss, gW, gb)
        torch.cuda.synchronize()
        assert arena.intact(), f"a guard was written under {fill}"
        pad = xb[:, D:]
        assert poison.same_bits(pad, poison.fill_(torch.empty_like(pad), fill)) is None, "the slack of x's rows is not written"
        xb[:, D:] = 0                                            # what lies in the slack is not read either
        ref = K.reference(x, y, W, b, np.float32(1.0 / N), np.float32(0.01))
        first = _run(rt, xb[:, :D], dy, dW, db, 1.0 / N, 0.01)
        assert K.mismatch(first, ref) is None
        poison.fill_(pad, fill)
        _same(first, _run(rt, xb[:, :D], dy, dW, db, 1.0 / N, 0.01))


def test_one_class_gives_exact_zeros(rt):
    N, D = 37, 64
    x, y, W, b = _device(*K.operands(N, 1, D, seed=6))
    got = _run(rt, x, y, W, b, 1.0 / N, 0.0)
    assert bool((got["row_loss"] == 0).all()) and bool((got["gW"] == 0).all()) and bool((got["gb"] == 0).all())
    start = (torch.randn((1, D), device=DEV) + 3.0, torch.ones((1,), device=DEV))
    got = _run(rt, x, y, W, b, 1.0 / N, 0.3, start)
    assert poison.same_bits(got["gW"], start[0]) is None and poison.same_bits(got["gb"], start[1]) is None, "exact zeros were added"
    got = _run(rt, x, y, W, b, 1.0 / N, 0.3)
    assert poison.same_bits(got["gW"], W * torch.tensor(0.3, device=DEV)) is None and bool((got["gb"] == 0).all())


def test_no_row(rt):
    C, D = 13, 96
    _, _, W, b = _device(*K.operands(4, C, D, seed=7))
    lib = rt.load_library()
    gW, gb = torch.full((C, D), 2.0, device=DEV), torch.full((C,), 3.0, device=DEV)
    args = (None, D, None, 0, C, D, _p(W), _p(b), 1.0, 0.5)
    assert lib.ovmr_probe_loss_grad(*args, 1, None, None, _p(gW), _p(gb), rt._stream()) == 0
    assert bool((gW == 2.0).all()) and bool((gb == 3.0).all()), "accumulate = 1 over no row: nothing is written"
    assert lib.ovmr_probe_loss_grad(*args, 0, None, None, _p(gW), _p(gb), rt._stream()) == 0
    assert poison.same_bits(gW, W * 0.5) is None and bool((gb == 0).all()), "accumulate = 0 over no row: the start, l2 * W and 0"
    loss, gW2, gb2, row_loss = rt.probe_loss_grad(torch.zeros((0, D), device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), W, b, 1.0, 0.5)
    assert poison.same_bits(gW2, gW) is None and bool((gb2 == 0).all()) and row_loss.shape == (0,)
    assert float(loss) == float(W.double().square().sum() * 0.25)


def test_logits_are_the_fp32_gemm(rt):
    lib = rt.load_library()
    for B, C, D in ((1, 1, 32), (65, 130, 96), (130, 13, 512)):
        x, _, W, b = _device(*K.operands(B, C, D, seed=8))
        want = torch.empty((B, C), dtype=torch.float32, device=DEV)
        dense = x.contiguous()
        assert lib.ovmr_debug_gemm(1, 0, _p(dense), _p(W), _p(b), None, None, _p(want), B, C, D, C, 1, 1.0, 0, 0, rt._stream()) == 0
        got = rt.probe_logits(x, W, b)
        assert got.shape == (B, C) and poison.same_bits(got, want) is None
        ref = x.double() @ W.double().T + b.double()
        assert float((got.double() - ref).abs().max()) <= (D + 1) * K.U * float((x.double().abs() @ W.double().abs().T + b.double().abs()).max())
        wide = poison.fill_(torch.empty((B + 2, C + 5), dtype=torch.float32, device=DEV), "nan16")
        keep = wide.clone()
        out = rt.probe_logits(x, W, b, out=wide[1:B + 1, 3:3 + C])
        assert out.data_ptr() == wide[1:, 3:].data_ptr() and poison.same_bits(wide[1:B + 1, 3:3 + C], want) is None
        keep[1:B + 1, 3:3 + C] = want
        assert poison.same_bits(wide, keep) is None, "the rest of the caller's buffer is left alone"


# ---- the fit on the device ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sklearn_gaps():
    """problem -> (sklearn's predictions on the held-out rows, its top-two logit gap there): fitted once."""
    from sklearn.linear_model import LogisticRegression
    out = {}
    for spec in K.PROBLEMS:
        X, y, Xh, _ = K.problem(*spec)
        sk = LogisticRegression(solver="lbfgs", tol=1e-10, max_iter=20000, C=1.0).fit(X.double().numpy(), y.numpy())
        z = sk.decision_function(Xh.double().numpy())
        top = np.sort(z, axis=1)
        out[spec] = (z.argmax(axis=1), top[:, -1] - top[:, -2])
    return out


@pytest.mark.parametrize("spec", K.PROBLEMS, ids=[f"{c}x{s}x{d}" for c, s, d, _ in K.PROBLEMS])
def test_fit_on_the_device(rt, spec, sklearn_gaps):
    from ovmr_amd import probe
    C, shots, D, _ = spec
    X, y, Xh, _ = K.problem(*spec)
    dX, dy = X.to(DEV), y.to(DEV)
    for c in (1e-2, 1.0, 1e2):
        r = probe.fit(probe.device_loss_grad(dX, dy), C, D, c, tol=1e-4, device=DEV)
        gmax, budget = K.grad_fp64(X, y, r.W.cpu(), r.b.cpu(), *K.scalars(len(y), c))
        print(f"{spec} c {c}: {r.n_iter} iterations, {r.n_eval} evaluations, converged {r.converged}, max |g| {r.max_grad:.3e}, in fp64 {gmax:.3e}, "
              f"budget {budget:.3e}")
        assert r.converged and r.W.is_cuda and gmax <= 1e-4 + budget
        if c == 1.0:
            pred, gap = sklearn_gaps[spec]
            keep = gap >= 0.05
            print(f"{spec}: sklearn's smallest top-two gap {gap.min():.3f}, {int((~keep).sum())} of {len(gap)} rows under 0.05")
            assert (~keep).mean() <= 0.02
            mine = rt.probe_logits(Xh.to(DEV), r.W, r.b).argmax(dim=1).cpu().numpy()
            assert (mine[keep] == pred[keep]).all()
            again = probe.fit(probe.device_loss_grad(dX, dy), C, D, c, tol=1e-4, device=DEV)
            assert again.n_iter == r.n_iter and again.n_eval == r.n_eval
            assert poison.same_bits(again.W, r.W) is None and poison.same_bits(again.b, r.b) is None, "two fits in one process: the same bits"
