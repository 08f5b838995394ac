"""The GEMM family held to exact values: every case of gemm_exact.CASES -- one per branch of the GEMM dispatcher (gemm_f16_route), plus
the fp32 kernel -- on operands for which every partial sum is exact in fp32 (gemm_exact.py: the method, the case table and which branch
each case takes; test_gemm_exact_cpu.py: the comparator rejects a lost product, a changed rounding point, a neighbour's bias).  The
expected output is ONE bit pattern whatever the K order, so for every case and every variant in {0, 6, 8, 9}

  * the output equals the reference bit for bit (fp16 as int16, fp32 as int32): every variant that takes a shape produces the same tensor;
  * the output buffer is filled with a sentinel, PAD_ROWS rows behind it: the rows behind M, the columns from N on where ldc > N, the
    CLS rows of EPI_PATCH and a residual that is not in place stay untouched, bit for bit;
  * stats_out: the (sum, sum of squares) pairs of the integer operand set equal the exact sums bit for bit;
  * QuickGELU, whose tail is the device's exp: the reference's fp16 form under test_gemm_f16's bound for the plain variants, the
    one-rounding form (variants + 100) under test_gemm_quickgelu_one_rounding's two bounds -- both evaluated on the exact x.

On a mismatch the message gives the count, the first (row, column), both modulo 256 and 64, got against want.
Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes
import time

import pytest
import torch

import gemm_exact as G
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


def _launch(lib, c, variant, A, W, bias, res, pos, C, stats=None):
    """One launch through the debug hook.  res: the residual's own buffer, or None for in place (res = C, ldres = ldc)."""
    ldc = C.shape[1]
    if c.kind == "strided":
        r, ldres = (C, ldc) if res is None else (res, res.shape[1])
        return lib.ovmr_debug_gemm_strided(variant, _p(A), c.K, _p(W), c.K, _p(bias), _p(r) if c.epi == G.EPI_BIAS_RES else None, ldres,
                                           _p(C), ldc, c.M, c.N, c.K, c.epi, G.SCALE, None, None, 1, _s())
    assert res is None and ldc == c.N
    extra = stats if stats is not None else pos
    return lib.ovmr_debug_gemm(int(c.kind == "f32"), variant, _p(A), _p(W), _p(bias), _p(C) if c.epi == G.EPI_BIAS_RES else None, _p(extra),
                               _p(C), c.M, c.N, c.K, ldc, c.epi, G.SCALE, c.rows[0], c.rows[1], _s())


def _run_exact(lib, c, ops, variants, with_stats=False):
    """Launch the case under every variant and compare output (and statistics) with the reference, bit for bit."""
    A, W, bias, res, pos = ops
    want, _ = G.expected(c, ops)
    dtype = want.dtype
    keep = G.compared_rows(c)
    want = want.cuda()
    G.bits(want)[~keep.cuda()] = G.SENTINEL                        # EPI_PATCH: the CLS rows must keep the sentinel
    st_want = G.expected_stats(want.cpu()).cuda() if with_stats else None
    Ad, Wd, bd = A.cuda(), W.cuda(), bias.cuda()
    rd = res.cuda() if c.epi == G.EPI_BIAS_RES else None
    pd = pos.cuda() if pos is not None else None
    for variant in variants:
        what = f"{c.id}, variant {variant}: {G.route(variant, c.M, c.N, c.K, c.epi, c.ldc, c.ldres, c.kind == 'stats') if c.kind != 'f32' else 'fp32'}"
        buf = G.sentinel_buffer(c.out_rows + G.PAD_ROWS, c.ldc or c.N, dtype, "cuda")
        own = None
        if c.epi == G.EPI_BIAS_RES and c.inplace:
            buf[:c.M, :c.N] = rd
        elif c.epi == G.EPI_BIAS_RES:
            own = G.sentinel_buffer(c.M + G.PAD_ROWS, c.ldres, dtype, "cuda")
            own[:c.M, :c.N] = rd
            own_before = own.clone()
        st = G.sentinel_buffer(c.M + G.PAD_ROWS, c.N // 256 * 2, torch.float32, "cuda") if c.kind == "stats" else None
        rc = _launch(lib, c, variant, Ad, Wd, bd, own, pd, buf, st)
        assert rc == 0, f"{what}: rc {rc}"
        torch.cuda.synchronize()
        msg = G.outside_untouched(buf, c.out_rows, c.N)
        assert msg is None, f"{what}: {msg}"
        msg = G.bits_mismatch(buf[:c.out_rows, :c.N], want)
        assert msg is None, f"{what}: {msg}"
        if own is not None:
            assert torch.equal(G.bits(own), G.bits(own_before)), f"{what}: the residual buffer was written"
        if st is not None:
            assert bool((G.bits(st[c.M:]) == G.SENTINEL32).all()), f"{what}: statistics written behind row {c.M}"
            if with_stats:
                msg = G.bits_mismatch(st[:c.M], st_want.view(c.M, -1))
                assert msg is None, f"{what}: statistics (columns: slot * 2 + (sum, sum of squares)): {msg}"
            else:
                assert bool(torch.isfinite(st[:c.M]).all()) and not bool((G.bits(st[:c.M]) == G.SENTINEL32).any()), f"{what}: unwritten statistics"


def _run_qgelu(lib, c, ops):
    """QuickGELU on the exact x = acc + b: the reference's fp16 form for the plain variants (test_gemm_f16's bound: 2e-3 * max(1, |ref|max),
    at most 2 % of the elements beyond an eighth of it), the one-rounding form for variants + 100 (test_gemm_quickgelu_one_rounding:
    within one fp16 step of the function + 2e-5, and within 8e-3 * max(1, |g|) of the fp16 form).  fp32: test_gemm_f32's tolerance."""
    A, W, bias, res, pos = ops
    acc = G.product(A, W)
    exact, ref16 = (t.cuda() for t in G.gelu_forms(acc, bias))
    Ad, Wd, bd = A.cuda(), W.cuda(), bias.cuda()
    f32 = c.kind == "f32"
    for variant in ((0,) if f32 else G.GEMM_VARIANTS + (100, 106, 108)):
        what = f"{c.id}, variant {variant}"
        buf = G.sentinel_buffer(c.M + G.PAD_ROWS, c.N, torch.float32 if f32 else torch.float16, "cuda")
        rc = _launch(lib, c, variant, Ad, Wd, bd, None, None, buf)
        assert rc == 0, f"{what}: rc {rc}"
        torch.cuda.synchronize()
        msg = G.outside_untouched(buf, c.M, c.N)
        assert msg is None, f"{what}: {msg}"
        got = buf[:c.M].double()
        assert bool(torch.isfinite(got).all()), what
        if f32:
            torch.testing.assert_close(buf[:c.M], exact.float(), atol=2e-4, rtol=2e-4)
        elif variant < 100:
            tol = 2e-3 * max(1.0, float(ref16.abs().max()))
            err = (got - ref16).abs()
            print(f"\n{what}: max err {float(err.max()):.3e} (bound {tol:.3e}), beyond an eighth {float((err > tol / 8).float().mean()):.3%}")
            assert float(err.max()) <= tol, f"{what}: max err {float(err.max())}"
            assert float((err > tol / 8).float().mean()) < 0.02, what
        else:
            step = torch.clamp(2.0 ** (torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** -14))) - 10), min=2.0 ** -24)
            over = float(((got - exact).abs() - step).max())
            rel = float(((got - ref16).abs() / ref16.abs().clamp_min(1.0)).max())
            print(f"\n{what}: |got - g| - step at most {over:.3e} (bound 2e-5), against the fp16 form {rel:.3e} (bound 8e-3)")
            assert over <= 2e-5, f"{what}: {over}"
            assert rel <= 8e-3, f"{what}: {rel}"


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.id)
def test_gemm_exact(lib, c):
    t0 = time.time()
    ops = G.operands(c)
    if c.epi == G.EPI_BIAS_QGELU:
        _run_qgelu(lib, c, ops)
    else:
        _run_exact(lib, c, ops, (0,) if c.kind == "f32" else G.GEMM_VARIANTS)
        if c.kind == "stats":
            _run_exact(lib, c, G.operands(c, integer=True), G.GEMM_VARIANTS, with_stats=True)
    print(f"\n{c.id}: {time.time() - t0:.2f} s")
