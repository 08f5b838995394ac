"""The tile loop of the LayerNorm-folding ping-pong GEMMs (gemm_f16_v5.hip "Tile loop") on gemm_persist_cases.py's table: the kernels
production runs (the store hint: <6, 8, 528>, <7, 8, 2576>), the production grid, ragged N, groups of 4 + 4 + 1 N tiles, 3 .. 8 statistics
slots (the late-read path from five on), row tiles without a guard and of five rows.  test_hip_gemm_persist.py stays as it is.

  * every case, epilogue 6 (and 7 in both QuickGELU forms on 785 x 576 x 256 and the two hinted cases): the launch of `tiles` workgroups
    passes gemm_ln_exact's comparator (decided bits; _check_qgelu for epilogue 7), every capped grid of gemm_persist_cases.grids equals
    it BIT FOR BIT, and PAD_ROWS sentinel rows behind M and 256 sentinel columns behind N survive every launch;
  * the hinted cases: the production launch (max_wgs = 0, persist = 1: one workgroup per CU) equals the launch with persist = 0 bit for
    bit and both pass the comparator; ovmr_debug_gemm_plan must say persist = 1, nt_store = 1, loop = ping-pong for the shape, so that a
    change to the route cannot make this pass without the loop running;
  * one strided launch with six slots (785 x 576 x 1024, row step 3; the rows in between other values, their statistics NaN) at 12, 1
    and 5 workgroups against the dense result;
  * the production launch of 8200 x 3072 x 256, epilogue 7, variant 108, ten times with a 256 MiB buffer rewritten in between: every
    output equals the first;
  * the engine: `small` (width 256, 17 tokens per image) on 1450 images -- in_proj 97 x 3 = 291 tiles, c_fc 97 x 4 = 388 tiles with the
    store hint at 50.5 MB, both planned as the loop at the M the engine's chunk gives -- encode_image under gemm_persist 0 and 1: bit-equal.

Seconds per test on an MI355X (pytest --durations, references built on 16 CPUs; the first test of a shape builds its reference):
    cases: 785x576x256 ln 0.86 (the first test: the library and the device come up in it), lnqgelu 0.15, one-rounding 0.05; each of the
    six other small cases 0.01 .. 0.03; 8200x3072x256 ln 1.45, lnqgelu 0.37, one-rounding 0.02; 10989x2304x256 ln 1.45, lnqgelu 0.38,
    one-rounding 0.02; strided 0.12; repeat below 0.01; engine 0.70; the 18 tests 7.7 in all (within the whole suite: 1.43 and 1.26 for
    the two slowest).
Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes
import functools

import pytest
import torch

import gemm_exact as G
import gemm_ln_exact as L
import gemm_persist_cases as P
from conftest import usable_threads
from test_gemm_persist_route_cpu import LOOP_PINGPONG, PLAN
from test_hip_gemm_ln_exact import _check_qgelu

pytestmark = pytest.mark.gpu

c_i, c_p = ctypes.c_int, ctypes.c_void_p
KERNEL_TILE = 3                         # GemmKernel (csrc/gemm_route.h)


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.set_num_threads(usable_threads())
    lib = runtime.load_library()
    lib.ovmr_debug_gemm_persist.restype = c_i
    lib.ovmr_debug_gemm_persist.argtypes = [c_i, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]
    lib.ovmr_debug_gemm_plan.restype = c_i
    lib.ovmr_debug_gemm_plan.argtypes = [c_i] * 10 + [ctypes.POINTER(c_i)]
    return lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plan(lib, variant, M, N, K, epi, persist):
    out = (c_i * len(PLAN))()
    assert lib.ovmr_debug_gemm_plan(variant, M, N, K, epi, N, N, 0, 0, persist, out) == 0
    return dict(zip(PLAN, out))


def _assert_loop_planned(lib, variant, M, N, K, epi, nt_store, what):
    p = _plan(lib, variant, M, N, K, epi, 1)
    assert (p["kernel"], p["rc"], p["tile_rows"], p["loop"], p["persist"]) == (KERNEL_TILE, 0, 256, LOOP_PINGPONG, 1), f"{what}: the route plans {p}"
    assert p["nt_store"] == nt_store, f"{what}: the route plans {p}"
    assert _plan(lib, variant, M, N, K, epi, 0)["persist"] == 0


@functools.lru_cache(maxsize=None)
def _problem(c):
    """(A, W, ln_g, ln_b, statistics [M, slots, 2]) on the device and the Reference: computed once per case, never written."""
    pr = P.problem(c)
    return tuple(t.cuda() for t in (pr.A, pr.W, pr.g, pr.b, pr.stats)), pr.ref.to("cuda")


@functools.lru_cache(maxsize=None)
def _gelu_forms(c):
    return tuple(t.cuda() for t in G.gelu_forms_of(P.problem(c).ref.x))


def _launch(lib, form, c, dev, wgs, persist=1, step=1):
    """One launch with at most `wgs` workgroups (0: as the route plans it under the option `persist`) into a sentinel buffer
    [M + PAD_ROWS, N + PAD_COLS]."""
    epi, variant = P.FORMS[form]
    A, W, g, b, stats = dev
    buf = G.sentinel_buffer(c.M + G.PAD_ROWS, c.N + P.PAD_COLS, torch.float16, "cuda")
    rc = lib.ovmr_debug_gemm_persist(variant, _p(A), step * c.K, _p(W), _p(b), _p(stats), c.slots, step * c.slots if step > 1 else 0, _p(g), _p(buf),
                                     c.N + P.PAD_COLS, c.M, c.N, c.K, epi, persist, wgs, _s())
    assert rc == 0, f"rc {rc}"
    torch.cuda.synchronize()
    msg = G.outside_untouched(buf, c.M, c.N)
    assert msg is None, f"{c.id} {form}, {wgs} workgroups, persist {persist}: {msg}"
    return buf


def _check(form, c, buf, ref, what):
    epi, variant = P.FORMS[form]
    got = buf[:c.M, :c.N].contiguous()
    if epi == G.EPI_LN_BIAS_QGELU:
        _check_qgelu(got, ref, _gelu_forms(c), variant, what)
    else:
        msg = L.ln_mismatch(got, ref)
        assert msg is None, f"{what}: {msg}"


@pytest.mark.parametrize("c,form", [(c, f) for c in P.CASES for f in P.forms_of(c)], ids=lambda v: v if isinstance(v, str) else v.id)
def test_every_grid_equals_one_tile_per_workgroup(lib, c, form):
    dev, ref = _problem(c)
    epi, variant = P.FORMS[form]
    want = _launch(lib, form, c, dev, c.tiles)
    _check(form, c, want, ref, f"{form} {c.id}, {c.tiles} workgroups")
    for wgs in P.grids(c):
        if wgs == c.tiles:
            continue
        if wgs == P.PRODUCTION and c.hinted:
            _assert_loop_planned(lib, variant, c.M, c.N, c.K, epi, 1, f"{form} {c.id}")
            off, on = _launch(lib, form, c, dev, 0, persist=0), _launch(lib, form, c, dev, 0, persist=1)
            _check(form, c, off, ref, f"{form} {c.id}, the route's launch with gemm_persist 0")
            _check(form, c, on, ref, f"{form} {c.id}, the production launch")
            msg = G.bits_mismatch(on, off)
            assert msg is None, f"{form} {c.id}: the production launch against gemm_persist 0: {msg}"
            got = on
        else:
            got = _launch(lib, form, c, dev, wgs)
        msg = G.bits_mismatch(got, want)
        assert msg is None, f"{form} {c.id}: {wgs} workgroups against {c.tiles}: {msg}"


def _strided(c, dev, step):
    """The operands with `step` - 1 rows between consecutive A rows (other values) and between their statistics (NaN)."""
    A, W, g, b, stats = dev
    R = (c.M - 1) * step + 1
    Ad = (torch.arange(R * c.K, device="cuda") % 7 - 3).half().reshape(R, c.K)
    Ad[::step] = A
    st = torch.full((R + G.PAD_ROWS, c.slots, 2), float("nan"), device="cuda")
    st[:R:step] = stats
    return Ad, W, g, b, st


def test_strided_rows_with_late_slots(lib):
    c, step = P.STRIDED, 3
    assert c.slots > 4 and c.N % 256
    dev, _ = _problem(c)
    want = _launch(lib, "ln", c, dev, c.tiles)
    sdev = _strided(c, dev, step)
    for wgs in (12, 1, 5):
        msg = G.bits_mismatch(_launch(lib, "ln", c, sdev, wgs, step=step), want)
        assert msg is None, f"{c.id}, row step {step}, {wgs} workgroups against the dense launch: {msg}"


def test_the_production_launch_repeats_itself(lib):
    c, form = P.HINTED[0], "lnqgelu-one-rounding"
    dev, _ = _problem(c)
    _assert_loop_planned(lib, P.FORMS[form][1], c.M, c.N, c.K, P.FORMS[form][0], 1, c.id)
    junk = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")            # 256 MiB: beyond the L2s and the Infinity Cache
    first = _launch(lib, form, c, dev, 0)
    for rep in range(1, 10):
        junk.add_(1.0)
        msg = G.bits_mismatch(_launch(lib, form, c, dev, 0), first)
        assert msg is None, f"launch {rep} differs from the first: {msg}"


def test_engine_features_do_not_depend_on_the_option(lib):
    import engine_replay as ER
    from ovmr_amd import synth
    from ovmr_amd.runtime import Engine
    B, spec = 1450, ER.SPECS["small"]
    sd, pl = ER.state_dicts("small")
    e = Engine(spec, ER.N_CTX)
    e.load_state_dict(sd, pl)
    e.finalize(B, 8, 8)
    assert e.encode_plan(B) == [e.encode_chunk], (e.encode_plan(B), e.encode_chunk)
    W, L_tok = spec.vision_width, (spec.image_resolution // spec.vision_patch_size) ** 2 + 1
    M = e.encode_chunk * L_tok
    assert (W, L_tok) == (256, 17) and (M + 255) // 256 == 97
    # variant 8 is the engine's default, + 100 its one-rounding QuickGELU; in_proj below the store hint, c_fc above it
    _assert_loop_planned(lib, 8, M, 3 * W, W, G.EPI_LN_BIAS, 0, f"in_proj at M = {M}")
    _assert_loop_planned(lib, 108, M, 4 * W, W, G.EPI_LN_BIAS_QGELU, 1, f"c_fc at M = {M}")
    img = torch.from_numpy(synth.images(B, spec.image_resolution, seed=4321)).cuda()
    out = {}
    for opt in (0, 1, 0):
        e.set_option("gemm_persist", opt)
        f = e.encode_image(img)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(f).all())
        assert opt not in out or G.bits_mismatch(f, out[opt]) is None
        out[opt] = f.clone()
    msg = G.bits_mismatch(out[1], out[0])
    assert msg is None, f"encode_image on {B} images, gemm_persist 1 against 0: {msg}"
    assert float(out[0].float().std()) > 0
