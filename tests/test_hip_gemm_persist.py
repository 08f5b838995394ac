"""The tile loop of the LayerNorm-folding ping-pong GEMMs (gemm_f16_v5.hip "Tile loop": in_proj and c_fc as a persistent kernel).

ovmr_debug_gemm_persist runs the 256-row ping-pong kernel on a shape of a few tiles with its grid capped, so that one workgroup
walks several tiles: both constant blocks, both K buffers and the staging area are reused, the next tile's operands are in flight
under every epilogue, and between consecutive tiles of a workgroup both tm and tn change.

  * shapes: M = 3 * 256 + 17 (a ragged last row tile), N = 512 / 768 (two / three N tiles), K = 128 / 256 (one / two passes of the
    K loop's unrolled body); epilogue 6, and 7 in both QuickGELU forms (variants 8 and 108); dense statistics and one strided launch
    (lda = 3 K, ln_stride = 3 slots, the rows in between other values, their statistics NaN);
  * grids of 1, 2, 5 and `tiles` workgroups: every capped result equals the one-tile-per-workgroup result BIT FOR BIT, and that one
    passes gemm_ln_exact's comparator (decided bits) on operands built by gemm_ln_exact's builders (K = 128 has no 256-column slot:
    its statistics are one slot holding row_sums itself);
  * the output buffer carries a sentinel in PAD_ROWS rows behind M and 64 columns behind N, which must survive;
  * one shape runs the one-workgroup launch 20 times with a 256 MiB buffer rewritten in between: every output equals the first
    (tools/race_screen.py's method, bounded).

The entry point is a test hook of the library without a row in runtime.SIGNATURES: its signature is bound here.
Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes
import functools

import pytest
import torch

import gemm_exact as G
import gemm_ln_exact as L
from conftest import usable_threads
from test_hip_gemm_ln_exact import _check_qgelu

pytestmark = pytest.mark.gpu

M = 3 * 256 + 17
PAD_COLS = 64
FORMS = {"ln": (G.EPI_LN_BIAS, 8), "lnqgelu": (G.EPI_LN_BIAS_QGELU, 8), "lnqgelu-one-rounding": (G.EPI_LN_BIAS_QGELU, 108)}
c_i, c_p = ctypes.c_int, ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.set_num_threads(usable_threads())
    lib = runtime.load_library()
    lib.ovmr_debug_gemm_persist.restype = c_i
    lib.ovmr_debug_gemm_persist.argtypes = [c_i, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]
    return lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _problem(N, K):
    """(A, W, ln_g, ln_b, statistics [M, slots, 2]) on the device and gemm_ln_exact's Reference: computed once per shape, never written."""
    if K >= 256:
        c = L.Case("epi", M, N, K, G.EPI_LN_BIAS, {})
        ops, ref = L.operands(c), L.expected(c)[0]
        A, W, g, b, stats = ops.A, ops.W, ops.g, ops.b, ops.stats
    else:
        A, W = G._aw(M, N, K, False)
        G.assert_exact(A, W, f"{M}x{N}x{K}")
        g, b = L.columns(N, M * 13 + N * 5 + K * 3 + 7)
        su, sq, deg, mean, var = L.row_sums(M, K)
        L.assert_rows_distinct(mean, var)
        stats = torch.stack([su, sq], 1)[:, None, :].float()
        assert torch.equal(stats.double()[:, 0], torch.stack([su, sq], 1))
        ref = L.reference(G.product(A, W), su, sq, g, b, K, deg)
    return tuple(t.cuda() for t in (A, W, g, b, stats)), ref.to("cuda")


def _launch(lib, form, dev, N, K, wgs, step=1):
    """One launch with at most `wgs` workgroups into a sentinel buffer [M + PAD_ROWS, N + PAD_COLS]."""
    epi, variant = FORMS[form]
    A, W, g, b, stats = dev
    buf = G.sentinel_buffer(M + G.PAD_ROWS, N + PAD_COLS, torch.float16, "cuda")
    slots = stats.shape[1]
    rc = lib.ovmr_debug_gemm_persist(variant, _p(A), step * K, _p(W), _p(b), _p(stats), slots, step * slots if step > 1 else 0, _p(g), _p(buf), N + PAD_COLS,
                                     M, N, K, epi, 1, wgs, _s())
    assert rc == 0, f"rc {rc}"
    torch.cuda.synchronize()
    msg = G.outside_untouched(buf, M, N)
    assert msg is None, f"{wgs} workgroups: {msg}"
    return buf


def _strided(dev, K, step):
    """The operands with `step` - 1 rows between consecutive A rows (other values) and between their statistics (NaN)."""
    A, W, g, b, stats = dev
    R = (M - 1) * step + 1
    Ad = (torch.arange(R * K, device="cuda") % 7 - 3).half().reshape(R, K)
    Ad[::step] = A
    st = torch.full((R + G.PAD_ROWS, stats.shape[1], 2), float("nan"), device="cuda")
    st[:R:step] = stats
    return Ad, W, g, b, st


def _check_tiles_form(form, want, ref, what):
    epi, variant = FORMS[form]
    got = want[:M, :ref.x.shape[1]].contiguous()
    if epi == G.EPI_LN_BIAS_QGELU:
        _check_qgelu(got, ref, tuple(t.cuda() for t in G.gelu_forms_of(ref.x.cpu())), variant, what)
    else:
        msg = L.ln_mismatch(got, ref)
        assert msg is None, f"{what}: {msg}"


@pytest.mark.parametrize("K", (128, 256))
@pytest.mark.parametrize("N", (512, 768))
@pytest.mark.parametrize("form", list(FORMS))
def test_capped_grids_equal_one_tile_per_workgroup(lib, form, N, K):
    dev, ref = _problem(N, K)
    tiles = 4 * (N // 256)
    want = _launch(lib, form, dev, N, K, tiles)
    _check_tiles_form(form, want, ref, f"{form} {M}x{N}x{K}, {tiles} workgroups")
    for wgs in (1, 2, 5):
        msg = G.bits_mismatch(_launch(lib, form, dev, N, K, wgs), want)
        assert msg is None, f"{form} {M}x{N}x{K}: {wgs} workgroups against {tiles}: {msg}"


def test_strided_rows_and_statistics(lib):
    N, K, step = 768, 256, 3
    dev, ref = _problem(N, K)
    want = _launch(lib, "ln", dev, N, K, 12)
    sdev = _strided(dev, K, step)
    for wgs in (12, 1, 2, 5):
        msg = G.bits_mismatch(_launch(lib, "ln", sdev, N, K, wgs, step), want)
        assert msg is None, f"row step {step}, {wgs} workgroups against the dense launch: {msg}"


def test_one_workgroup_repeats_itself(lib):
    N, K = 768, 256
    dev, _ = _problem(N, K)
    junk = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")            # 256 MiB: beyond the L2s and the Infinity Cache
    first = _launch(lib, "lnqgelu-one-rounding", dev, N, K, 1)
    for rep in range(1, 20):
        junk.add_(1.0)
        msg = G.bits_mismatch(_launch(lib, "lnqgelu-one-rounding", dev, N, K, 1), first)
        assert msg is None, f"launch {rep} differs from the first: {msg}"
