"""The LayerNorm-folding GEMM epilogues (EPI_LN_BIAS, EPI_LN_BIAS_QGELU) and the kernels that produce their operands, held to decided
bits: every case of gemm_ln_exact.CASES under every variant it lists (0, 6, 8, 9; epilogue 7 also 100, 106, 108), against the fp64
formula on exact inputs under the derived budget E (gemm_ln_exact.py: the method, the derivation, the operands and which branch each
case takes; test_gemm_ln_exact_cpu.py: honest fp32 evaluations pass, each planted defect is rejected).

  * "epi" cases: ovmr_debug_gemm with the statistics, ln_g and ln_b handed in -- the tile kernel's two prologues and its epilogue alone;
  * "rows" / "stats" / "stride" cases: ovmr_debug_lnfold without and with the first GEMM, ovmr_debug_gemm_strided with row_step: the
    producing kernels in front.  x1 of a "stats" case is compared bit for bit; a strided launch is bit-equal to the gathered one.
    A chain that fails names the producing kernels and the row's expected (su, sq);
  * epilogue 7: QuickGELU keeps its inexact tail; gemm_exact.gelu_forms_of(x) under test_hip_gemm_exact._run_qgelu's bounds on the
    ordinary rows (on degenerate rows x itself is only known to E: the same bounds widened by 1.1 (E + an fp16 step), _check_qgelu);
  * every output buffer is filled with a sentinel, PAD_ROWS rows behind it, and must keep it outside the written block.

Per case the test prints the worst observed error over E (gemm_ln_exact.observed: what the fp16 output shows of the fp32 error) on
ordinary and on degenerate rows, and the seconds taken.  Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes
import time

import pytest
import torch

import gemm_exact as G
import gemm_ln_exact as L
from conftest import usable_threads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.set_num_threads(usable_threads())
    return runtime.load_library()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_qgelu(got16, ref, forms, variant, what):
    """test_hip_gemm_exact._run_qgelu's bounds, unchanged, on the ordinary rows.  On a degenerate row x itself is only known to E: the
    kernel's x^ is within E of x, so its fp16 value is within E + one fp16 step of h(x), and QuickGELU, whose slope stays within
    [-0.1, 1.1], carries at most 1.1 times that to the output: the same bounds widened by 1.1 (E + one fp16 step at |x| + E)."""
    exact, ref16 = forms
    got = got16.double()
    assert bool(torch.isfinite(got).all()), what
    slack = torch.where(ref.deg[:, None], 1.1 * (ref.E + 2 * L.half_step(ref.x.abs() + ref.E)), torch.zeros_like(ref.E))

    def where(t):
        r, col = (int(i) for i in (t == t.max()).nonzero()[0])
        return f"{what}: {float(t.max())} at ({r}, {col}), {'a degenerate' if bool(ref.deg[r]) else 'an ordinary'} row: got {float(got[r, col])}, x = {float(ref.x[r, col])}"
    if variant < 100:
        tol = 2e-3 * max(1.0, float(ref16[~ref.deg].abs().max()))
        err = (got - ref16).abs() - slack
        far = float((err[~ref.deg] > tol / 8).float().mean())
        print(f"\n{what}: max err {float(err.max()):.3e} (bound {tol:.3e}), beyond an eighth {far:.3%}")
        assert float(err.max()) <= tol, where(err)
        assert far < 0.02, what
    else:
        step = torch.clamp(2.0 ** (torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** -14))) - 10), min=2.0 ** -24)
        over_, rel_ = (got - exact).abs() - step - slack, ((got - ref16).abs() - slack) / ref16.abs().clamp_min(1.0)
        over, rel = float(over_.max()), float(rel_.max())
        print(f"\n{what}: |got - g| - step at most {over:.3e} (bound 2e-5), against the fp16 form {rel:.3e} (bound 8e-3)")
        assert over <= 2e-5, where(over_)
        assert rel <= 8e-3, where(rel_)


def _check(c, variant, buf, ref, forms, worst, what, producers=None, sums=None):
    msg = G.outside_untouched(buf, c.M, c.N)
    assert msg is None, f"{what}: {msg}"
    got = buf[:c.M]
    if c.epi == G.EPI_LN_BIAS_QGELU:
        return _check_qgelu(got, ref, forms, variant, what)
    o, od = L.worst_observed(got, ref)
    worst[0], worst[1] = max(worst[0], o), max(worst[1], od)
    msg = L.ln_mismatch(got, ref, producers, sums)
    assert msg is None, f"{what}: {msg}"


@pytest.mark.parametrize("c", L.CASES, ids=lambda c: c.id)
def test_gemm_ln_exact(lib, c):
    t0 = time.time()
    ops = L.operands(c)
    ref = L.expected(c)[0]
    forms = tuple(t.cuda() for t in G.gelu_forms_of(ref.x)) if c.epi == G.EPI_LN_BIAS_QGELU else None
    ref = ref.to("cuda")
    sums = (ops.su, ops.sq)
    worst = [0.0, 0.0]
    Ad, Wd = ops.A.cuda(), ops.W.cuda()
    if c.kind == "epi":
        gd, bd, st = ops.g.cuda(), ops.b.cuda(), L.stats_buffer(ops).cuda()
    else:
        raw = ops.raw
        W2d, gammad, betad, b2d = (raw[k].cuda() for k in ("W2", "gamma", "beta", "b2"))
    if c.kind == "stats":
        c1 = raw["c1"]
        A1d, W1d, b1d = (t.cuda() for t in raw["ops1"][:3])
        res1d, x1_want = raw["ops1"][3].cuda(), raw["x1"].cuda()
    for variant in c.variants:
        what = f"{c.id}, variant {variant}: {G.route(variant, c.M, c.N, c.K, c.epi)}"
        buf = G.sentinel_buffer(c.M + G.PAD_ROWS, c.N, torch.float16, "cuda")
        if c.kind == "epi":
            rc = lib.ovmr_debug_gemm(0, variant, _p(Ad), _p(Wd), _p(bd), _p(st), _p(gd), _p(buf), c.M, c.N, c.K, c.N, c.epi, 1.0, 0, 0, _s())
        elif c.kind == "rows":
            x1 = Ad.clone()
            rc = lib.ovmr_debug_lnfold(variant, None, None, None, None, c.M, c.K, 0, _p(W2d), _p(gammad), _p(betad), _p(b2d), c.N, 0, _p(x1), _p(buf), _s())
        elif c.kind == "stats":
            x1 = G.sentinel_buffer(c.M + G.PAD_ROWS, c.K, torch.float16, "cuda")
            x1[:c.M] = res1d                                             # the residual, in place
            rc = lib.ovmr_debug_lnfold(variant, _p(A1d), _p(W1d), _p(b1d), _p(x1), c.M, c.K, c.K1, _p(W2d), _p(gammad), _p(betad), _p(b2d), c.N, 0,
                                       _p(x1), _p(buf), _s())
        else:
            rc = lib.ovmr_debug_gemm_strided(variant, _p(Ad), c.step * c.K, _p(W2d), c.K, _p(b2d), None, 0, _p(buf), c.N, c.M, c.N, c.K, c.epi, 1.0,
                                             _p(gammad), _p(betad), c.step, _s())
        assert rc == 0, f"{what}: rc {rc}"
        torch.cuda.synchronize()
        if c.kind == "rows":
            assert torch.equal(G.bits(x1), G.bits(Ad)), f"{what}: the input rows were written"
        if c.kind == "stats":
            msg = G.outside_untouched(x1, c.M, c.K) or G.bits_mismatch(x1[:c.M], x1_want)
            assert msg is None, f"{what}: x1 of the first GEMM ({G.route(variant, c.M, c.K, c.K1, c1.epi, stats=True)}): {msg}"
        _check(c, variant, buf, ref, forms, worst, what, L.PRODUCERS.get(c.kind), sums)
        if c.kind == "stride":                                           # the same launch on the gathered rows: bit-equal
            xg = Ad[::c.step].contiguous()
            gath = G.sentinel_buffer(c.M + G.PAD_ROWS, c.N, torch.float16, "cuda")
            rc = lib.ovmr_debug_lnfold(variant, None, None, None, None, c.M, c.K, 0, _p(W2d), _p(gammad), _p(betad), _p(b2d), c.N, 0, _p(xg), _p(gath), _s())
            assert rc == 0, f"{what}: gathered rc {rc}"
            torch.cuda.synchronize()
            msg = G.bits_mismatch(buf, gath)
            assert msg is None, f"{what}: strided != gathered: {msg}"
    print(f"\n{c.id}: worst observed error over E {worst[0]:.3f} on ordinary rows, {worst[1]:.3f} on degenerate rows; {time.time() - t0:.2f} s")
