"""Which fp16 GEMM kernel a launch runs, and with which options.  Every kernel computes the same values, so a routing mistake changes no
output bit, only the time: the exact-value tests cannot see it.  Here the library's routing function (gemm_f16_route in
csrc/gemm_f16.hip, exported as ovmr_debug_gemm_route) is held to gemm_exact.route -- the dispatcher as it stood before there was a
routing function, restated in Python -- on the case table of the exact-value tests and on a grid around every threshold, and the set of
plans is held to the tile kernel's instantiation table (csrc/gemm_f16_v5.hip, ovmr_debug_gemm_tile_kernels): none unreachable, none
missing.  Loads the library as test_abi_cpu.py does: no launch, no GPU."""
import ctypes
import os

import pytest

import gemm_exact as G

VARIANTS = (0, 6, 7, 8, 9)
FIELDS = ("kernel", "rc", "depth", "groups", "tile_rows", "loop", "a_nt", "nt_store", "n_group", "gelu_mode")
LOOPS = ("double", "boundary", "pingpong")
OPT_BITS = {"a_nt": 1, "boundary": 4, "pingpong": 16, "nt": 512, "gelu": 2048}      # gemm_f16_v5.hip: part of the kernels' names

# the grid: M around 64 / 256 and the large row counts of the case table, N around 128, N & 7, 256, 1024, 2048, 3072
GRID_M = (63, 64, 65, 255, 256, 257, 300, 1100, 4333, 4353, 5613, 8200, 10800, 11245, 32700, 43600, 130900)
GRID_N = (120, 127, 128, 129, 136, 255, 256, 257, 264, 520, 768, 1000, 1016, 1024, 1032, 2040, 2048, 2056, 3064, 3072, 3080)
GRID_K = (64, 128, 192, 256, 320, 384, 768, 2048, 3072, 4096)
GRID_VARIANTS = VARIANTS + (108,)
IM2COL_R = 224              # 14 x 14 patches of 16 x 16 pixels: rows_in = 196

# (variant, M, N, K, epi, ldc, ldres, stats, im2col) -> plan, read from the launchers before there was a routing function
SPOT = {
    (8, 0, 128, 128, 0, 128, 128, 0, 0): ("err", 0),                                   # empty
    (8, 300, 256, 96, 1, 256, 256, 0, 0): ("err", -2),                                 # K % 64
    (3, 4333, 2048, 128, 1, 2048, 2048, 0, 0): ("err", -5),                            # no such K loop, on a shape the tile kernel takes
    (3, 127, 2048, 128, 1, 2048, 2048, 0, 0): ("t128",),                               # ... on one it refuses: handed on
    (8, 300, 256, 128, 9, 256, 256, 0, 0): ("err", -3),
    (0, 4333, 2048, 128, 9, 2048, 2048, 0, 0): ("err", -3),
    (0, 255, 2048, 256, 6, 2048, 2048, 0, 0): ("err", -4),                             # LayerNorm fold below one row tile
    (9, 300, 520, 256, 7, 520, 520, 0, 0): ("err", -2),                                # ... N % 64
    (8, 300, 136, 128, 8, 136, 136, 0, 0): ("v5", 128, "double", "", "", ""),          # argmax on a ragged N, variant 8 past the split-K kernel
    (8, 300, 256, 128, 1, 256, 256, 1, 0): ("err", -2),                                # statistics of another epilogue than BIAS_RES
    (0, 300, 264, 128, 3, 264, 264, 1, 0): ("err", -2),                                # ... N % 256
    (7, 300, 256, 256, 3, 256, 256, 0, 0): ("v5", 128, "double", "", "", ""),          # 7: variant 8 without the split-K kernel
    (8, 300, 256, 256, 3, 256, 256, 0, 0): ("s64", 2, 1),
    (8, 8 * 196, 768, 768, 4, 768, 768, 0, IM2COL_R): ("v5", 128, "double", "", "", ""),
    (0, 64 * 196, 768, 768, 4, 768, 768, 0, IM2COL_R): ("v5", 256, "pingpong", "", "", ""),
    (8, 8 * 196, 768, 128, 4, 768, 768, 0, IM2COL_R): ("err", -2),                     # patch rows are K = 768
    (8, 8 * 196, 768, 768, 1, 768, 768, 0, IM2COL_R): ("err", -2),
    (8, 8 * 196, 768, 768, 4, 768, 768, 0, 100): ("err", -2),                          # R % 16
    (9, 196, 768, 768, 4, 768, 768, 0, IM2COL_R): ("err", -4),
    # the images' bytes against 2^31 (R = 1024: 6 MiB an image): 341 whole images pass, one row of a 342nd is -2 (the gather's own guard
    # counts that image whole), 342 whole images are -4 (M * 768 * 2: the tile kernel does not take the shape)
    (8, 341 * 4096, 128, 768, 4, 128, 128, 0, 1024): ("v5", 256, "pingpong", "", "nt", ""),
    (6, 341 * 4096, 128, 768, 4, 128, 128, 0, 1024): ("v5", 256, "double", "", "nt", ""),
    (8, 341 * 4096 + 1, 128, 768, 4, 128, 128, 0, 1024): ("err", -2),
    (8, 342 * 4096, 128, 768, 4, 128, 128, 0, 1024): ("err", -4),
    (108, 8200, 3072, 768, 7, 3072, 3072, 0, 0): ("v5", 256, "pingpong", "", "nt", "g4"),   # DESIGN.md's <7, 8, 2576>
}


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import build, runtime
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    return runtime.load_library()


_OUT = (ctypes.c_int * len(FIELDS))()


def lib_plan(lib, variant, M, N, K, epi, ldc, ldres, stats, im2col):
    assert lib.ovmr_debug_gemm_route(variant, M, N, K, epi, ldc, ldres, stats, im2col, _OUT) == 0
    return dict(zip(FIELDS, _OUT))


def as_route(p, N):
    """A library plan in gemm_exact.route's form, and whether QuickGELU runs in the one-rounding form."""
    gelu = p["gelu_mode"] != 0
    if p["kernel"] == 0:
        return ("err", p["rc"]), gelu
    if p["kernel"] == 1:
        return ("t128",), gelu
    if p["kernel"] == 2:
        return ("s64", p["depth"], p["groups"]), gelu
    assert p["kernel"] == 3, p
    tn = (N + 255) // 256
    assert p["n_group"] in (4, tn), p
    return ("v5", p["tile_rows"], LOOPS[p["loop"]], "a_nt" if p["a_nt"] else "", "nt" if p["nt_store"] else "", "g4" if p["n_group"] != tn else ""), gelu


def case_launches():
    """Every fp16 case of the exact-value tests under every variant, and under + 100."""
    for c in G.CASES:
        if c.kind != "f32":
            ldc = c.ldc or c.N
            for v in VARIANTS:
                for variant in (v, v + 100):
                    yield variant, c.M, c.N, c.K, c.epi, ldc, c.ldres or ldc, int(c.kind == "stats"), 0


def grid_launches():
    for variant in GRID_VARIANTS:
        for M in GRID_M:
            for N in GRID_N:
                for K in GRID_K:
                    for epi in range(9):
                        yield variant, M, N, K, epi, N, N, 0, 0
                    for epi in (G.EPI_BIAS, G.EPI_BIAS_RES):
                        yield variant, M, N, K, epi, N, N, 1, 0


def all_launches():
    yield from case_launches()
    yield from grid_launches()
    yield from SPOT


def _differences(lib, launches):
    n, bad = 0, []
    for key in launches:
        variant, M, N, K, epi, ldc, ldres, stats, im2col = key
        want = G.route(variant, M, N, K, epi, ldc, ldres, bool(stats), im2col), G.one_rounding_gelu(variant, epi)
        got = as_route(lib_plan(lib, *key), N)
        n += 1
        if got != want:
            bad.append((key, got, want))
    return n, bad


def test_restated_route_gives_the_spot_values():
    for key, plan in SPOT.items():
        variant, M, N, K, epi, ldc, ldres, stats, im2col = key
        assert G.route(variant, M, N, K, epi, ldc, ldres, bool(stats), im2col) == plan, f"route{key}, the launchers ran {plan}"
    for c in G.CASES:                               # + 100 changes the QuickGELU form, never the kernel
        for v in VARIANTS:
            assert G.route(v + 100, c.M, c.N, c.K, c.epi, c.ldc, c.ldres, c.kind == "stats") == G.route(v, c.M, c.N, c.K, c.epi, c.ldc, c.ldres, c.kind == "stats")


def test_library_route_equals_the_restated_route_on_the_cases(lib):
    n, bad = _differences(lib, list(case_launches()) + list(SPOT))
    assert not bad, f"{len(bad)} of {n} launches differ; (key, library, restated): {bad[:6]}"


def test_library_route_equals_the_restated_route_on_the_grid(lib):
    n, bad = _differences(lib, grid_launches())
    assert n > 200000
    assert not bad, f"{len(bad)} of {n} launches differ; (key, library, restated): {bad[:6]}"


def test_the_plans_are_the_tile_kernel_table(lib):
    cap = 256
    buf = (ctypes.c_int * (3 * cap))()
    n = lib.ovmr_debug_gemm_tile_kernels(buf, cap)
    assert 0 < n <= cap
    table = [tuple(buf[3 * i:3 * i + 3]) for i in range(n)]
    assert len(set(table)) == n, "an instantiation is listed twice"
    planned = set()
    for key in all_launches():
        variant, M, N, K, epi, ldc, ldres, stats, im2col = key
        r = G.route(variant, M, N, K, epi, ldc, ldres, bool(stats), im2col)
        if r[0] == "v5":
            opt = OPT_BITS.get(r[2], 0) | (OPT_BITS["a_nt"] if r[3] else 0) | (OPT_BITS["nt"] if r[4] else 0)
            planned.add((epi, r[1] // 32, opt | (OPT_BITS["gelu"] if G.one_rounding_gelu(variant, epi) else 0)))
    assert planned == set(table), f"planned, not in the table: {sorted(planned - set(table))}; in the table, never planned: {sorted(set(table) - planned)}"
    for epi, mt, opt in table:                      # what the table must not hold, whatever the route says
        assert mt in (4, 8) and (mt == 8 or not opt & OPT_BITS["pingpong"]), "the ping-pong loop exists for 256-row tiles only"
        assert not (opt & OPT_BITS["pingpong"] and opt & OPT_BITS["boundary"])
        assert not opt & OPT_BITS["a_nt"] or epi == G.EPI_BIAS_RES
        assert not opt & OPT_BITS["boundary"] or epi in (G.EPI_BIAS_RES, G.EPI_LN_BIAS, G.EPI_LN_BIAS_QGELU)
        assert not opt & OPT_BITS["gelu"] or epi in (G.EPI_BIAS_QGELU, G.EPI_LN_BIAS_QGELU)
        assert not opt & OPT_BITS["nt"] or epi not in (G.EPI_BIAS_RES, G.EPI_SCALE_ARGMAX)
