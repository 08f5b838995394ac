"""Which attention kernel a launch runs.  Every fp16 kernel computes the same values, so a routing mistake changes no output, only the
time: the exact-value tests cannot see it.  Here the library's routing function (route() in csrc/attention.hip, exported as
ovmr_debug_attention_route) is held to attn_exact.route -- the shape tests the launchers used to make themselves, restated in Python --
on a grid around every threshold, and the case tables of test_hip_attn_exact.py are checked to reach every kernel.
Loads the library as test_abi_cpu.py does: no launch, no GPU."""
import os

import pytest

import attn_exact as A

VARIANTS = (0, 1, 2, 3, 4, 5, 7)            # the option values with a meaning, and two without one
LENGTHS = A.SHORT_L + A.MID_L + A.SINGLE_L + A.LONG_L
KERNELS = {A.V0, A.V1, A.SHORT, A.V3, A.V5}

# (variant, L, Lq, causal) -> kernel, read from the launchers' own shape tests before there was a routing function
SPOT = {
    (3, 197, 197, 0): A.V3, (3, 197, 1, 0): A.V1, (3, 257, 257, 0): A.V5, (3, 257, 16, 0): A.V1, (3, 257, 33, 0): A.V5,
    (3, 209, 209, 0): A.V1, (3, 192, 192, 0): A.V1, (3, 77, 77, 1): A.V0, (3, 32, 32, 1): A.SHORT, (3, 33, 33, 1): A.V0,
    (0, 32, 32, 1): A.V0, (5, 577, 577, 1): A.V1, (1, 128, 128, 0): A.V1, (1, 127, 127, 0): A.V0, (4, 197, 197, 0): A.V3,
}


def _grid():
    for variant in VARIANTS:
        for L in LENGTHS:
            for Lq in sorted({lq for lq in (1, 16, 31, 32, 33, L) if lq <= L}):
                for causal in (0, 1):
                    yield variant, L, Lq, causal


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import build, runtime
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    return runtime.load_library()


def test_restated_route_gives_the_spot_values():
    grid = set(_grid())
    for key, kernel in SPOT.items():
        assert A.route(*key) == kernel, f"route{key} = {A.route(*key)}, the launchers ran {kernel}"
        assert key in grid, f"{key} is not on the grid"


def test_library_route_equals_the_restated_route(lib):
    got = {key: lib.ovmr_debug_attention_route(*key) for key in _grid()}
    bad = [(key, kernel, A.route(*key)) for key, kernel in got.items() if kernel != A.route(*key)]
    assert not bad, f"{len(bad)} of {len(got)} (variant, L, Lq, causal) differ; (key, library, restated): {bad[:8]}"
    assert {A.route(*key) for key in _grid()} == KERNELS


def _launches():
    """(variant, L, Lq, causal) of every fp16 launch of test_attention_exact and test_attention_q_exact."""
    for c in A.CASES:
        for variant in c.variants:
            yield variant, c.L, c.L, c.causal
    for L in A.Q_L:
        for Lq in A.Q_LQ:
            for variant in A.ATTN_VARIANTS:
                yield variant, L, Lq, 0


def _v5_waves(Lq):
    """Waves per workgroup of variant 5's launch: 3 where that leaves fewer idle wave slots than 4 (attention_v5.hip)."""
    nT = (Lq + 31) // 32
    return 3 if (nT + 2) // 3 * 3 < (nT + 3) // 4 * 4 else 4


def test_case_tables_reach_every_kernel():
    ran = {}
    for key in _launches():
        ran.setdefault(A.route(*key), []).append(key)
    assert set(ran) == KERNELS, f"no case runs kernel(s) {sorted(KERNELS - set(ran))}"
    v5 = {(Lq, _v5_waves(Lq)) for _, _, Lq, _ in ran[A.V5]}
    assert (257, 3) in v5 and _v5_waves(257) == 3 and (257 + 31) // 32 == 9, "variant 5's 3-wave launch (9 tiles at Lq = 257)"
    assert (577, 4) in v5, "variant 5's 4-wave launch (Lq = 577)"
