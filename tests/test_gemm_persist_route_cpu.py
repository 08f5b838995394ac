"""The tile loop of the LayerNorm-folding ping-pong GEMMs (gemm_f16_v5.hip "Tile loop"), the parts that need no GPU:

  * gemm_f16_route plans it (GemmPlan::persist, the eleventh field of ovmr_debug_gemm_plan) exactly where the caller's "gemm_persist"
    option is on, the epilogue is a LayerNorm-folding one, the launch runs 256-row tiles with the ping-pong K loop and has more tiles
    than the 256 CUs -- and the option changes no other field of any plan;
  * a grid of `grid` workgroups, workgroup w taking the dispatch slots w, w + grid, ..., visits every tile exactly once, and visits
    them in the order in which one workgroup per tile is dispatched today: slot -> tile is the XCD-aware map of the block id,
    restated here (ovmr_debug_gemm_tile_walk against tile_of), over grids of 1 .. 600 x 1 .. 12 tiles and 1 .. 256 workgroups.

Both entry points are test hooks without a row in runtime.SIGNATURES: their signatures are bound here.  No launch, no GPU."""
import ctypes
import os
import random

import pytest

import gemm_exact as G
from test_gemm_route_cpu import FIELDS, GRID_K, GRID_M, GRID_N, IM2COL_R

c_i = ctypes.c_int
PLAN = FIELDS + ("persist",)
LOOP_PINGPONG = 2


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import build, runtime
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    lib = runtime.load_library()
    lib.ovmr_debug_gemm_plan.restype = c_i
    lib.ovmr_debug_gemm_plan.argtypes = [c_i] * 10 + [ctypes.POINTER(c_i)]
    lib.ovmr_debug_gemm_tile_walk.restype = c_i
    lib.ovmr_debug_gemm_tile_walk.argtypes = [c_i, c_i, c_i, c_i, ctypes.POINTER(c_i), c_i]
    return lib


_OUT = (c_i * len(PLAN))()


def plan(lib, variant, M, N, K, epi, persist, im2col=0):
    assert lib.ovmr_debug_gemm_plan(variant, M, N, K, epi, N, N, 0, im2col, persist, _OUT) == 0
    return dict(zip(PLAN, _OUT))


def test_persist_is_planned_for_the_stated_launches_only(lib):
    n = planned = 0
    rows = GRID_M + (196 * 256, 197 * 775, 65280, 65281, 65536, 65537)          # 255 / 256 / 257 row tiles of 256 rows, the batch shapes
    for variant in (0, 6, 7, 8, 9, 108):
        for M in rows:
            for N in GRID_N + (2304,):
                for K in GRID_K:
                    for epi in range(9):
                        off, on = plan(lib, variant, M, N, K, epi, 0), plan(lib, variant, M, N, K, epi, 1)
                        assert off["persist"] == 0
                        assert {k: v for k, v in on.items() if k != "persist"} == {k: v for k, v in off.items() if k != "persist"}
                        tiles = ((M + 255) // 256) * ((N + 255) // 256)
                        want = int(on["kernel"] == 3 and epi in (G.EPI_LN_BIAS, G.EPI_LN_BIAS_QGELU) and on["tile_rows"] == 256 and
                                   on["loop"] == LOOP_PINGPONG and tiles > 256)
                        assert on["persist"] == want, (variant, M, N, K, epi, on)
                        n += 1
                        planned += want
    assert planned > 100 and n > 50000
    # the launches the loop was written for: in_proj and c_fc at 775 and 256 images
    for M, N, epi in ((197 * 775, 2304, G.EPI_LN_BIAS), (197 * 775, 3072, G.EPI_LN_BIAS_QGELU), (197 * 256, 2304, G.EPI_LN_BIAS), (197 * 256, 3072, G.EPI_LN_BIAS_QGELU)):
        assert plan(lib, 108, M, N, 768, epi, 1)["persist"] == 1
    assert plan(lib, 8, 197 * 775, 768, 768, G.EPI_BIAS_RES, 1)["persist"] == 0                      # the residual projections stay as they are
    assert plan(lib, 8, 64 * 196, 768, 768, G.EPI_PATCH, 1, IM2COL_R)["persist"] == 0
    assert plan(lib, 6, 197 * 775, 2304, 768, G.EPI_LN_BIAS, 1)["persist"] == 0                      # the boundary loop
    assert plan(lib, 8, 256 * 64, 1024, 768, G.EPI_LN_BIAS, 1)["persist"] == 0                       # 256 tiles: one per CU already


def tile_of(bid, tiles_m, tiles_n, n_group):
    """The block id -> (tm, tn) map of the tile kernel as it stood before there was a tile loop."""
    nwg = tiles_m * tiles_n
    xcd, idx, q, r = bid & 7, bid >> 3, nwg >> 3, nwg & 7
    bid = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
    g = n_group if n_group > 0 else tiles_n
    full, per = tiles_n // g, tiles_m * g
    grp = bid // per
    if grp < full:
        r = bid - grp * per
        return r // g, grp * g + r % g
    gl, r = tiles_n - full * g, bid - full * per
    return r // gl, full * g + r % gl


def walk_cases():
    rnd = random.Random(5)
    edge_m, edge_g = (1, 2, 7, 8, 9, 21, 28, 63, 64, 65, 591, 592, 600), (1, 2, 7, 8, 9, 255, 256)
    for tm in edge_m:
        for tn in range(1, 13):
            for grid in edge_g:
                yield tm, tn, grid
    for _ in range(600):
        yield rnd.randint(1, 600), rnd.randint(1, 12), rnd.randint(1, 256)


def test_the_walk_visits_every_tile_once_in_dispatch_order(lib):
    cap = 600 * 12
    buf = (c_i * (3 * cap))()
    n_cases = 0
    for tiles_m, tiles_n, grid in walk_cases():
        tiles = tiles_m * tiles_n
        for n_group in {tiles_n, 4 if tiles_n >= 8 else tiles_n, 0}:
            assert lib.ovmr_debug_gemm_tile_walk(tiles_m, tiles_n, n_group, grid, buf, cap) == tiles
            got = [tuple(buf[3 * i:3 * i + 3]) for i in range(tiles)]
            want = [(w,) + tile_of(slot, tiles_m, tiles_n, n_group) for w in range(min(grid, tiles)) for slot in range(w, tiles, grid)]
            assert got == want, (tiles_m, tiles_n, n_group, grid)
            assert sorted(t[1:] for t in got) == [(m, n) for m in range(tiles_m) for n in range(tiles_n)], (tiles_m, tiles_n, n_group, grid)
            n_cases += 1
    # one workgroup per tile: the walk is today's dispatch
    assert lib.ovmr_debug_gemm_tile_walk(21, 12, 4, 21 * 12, buf, cap) == 252
    assert [tuple(buf[3 * i + 1:3 * i + 3]) for i in range(252)] == [tile_of(b, 21, 12, 4) for b in range(252)]
    assert n_cases > 1500
