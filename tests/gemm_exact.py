"""Exact-operand cases, the reference and the comparator for the GEMM family (ovmr_amd/csrc/gemm_f16.hip, gemm_f16_small.hip,
gemm_f16_v5.hip, gemm_f32.hip behind ovmr_debug_gemm / ovmr_debug_gemm_strided).  Plain torch, no library: shared by
test_hip_gemm_exact.py (GPU) and test_gemm_exact_cpu.py (which proves that the comparator rejects the defects it is there for).

The method (head_exact.py carried over).  A and W are dense, without zeros, entries +-k/16 with 1 <= k <= 15; bias entries are
non-zero multiples of 2^-8 in [-2, 2], residual and positional entries non-zero multiples of 2^-7 in (-16, 16): all fp16 values.
Every product is a multiple of 2^-8 and sum_k |a||w| < K <= 4096 < 2^16, so every partial sum of every dot product, in any order and
grouping, is exact in fp32 and in the MFMA's fp32 accumulator, and so is acc + bias.  The fp16 output of an epilogue is then ONE bit
pattern whatever the kernel's K order: the comparison is bit equality, with no tolerance.  What the epilogues round, and where
(common.h, test_hip_kernels._ref_gemm_f16):

    NONE h(acc)     BIAS h(acc + b)     BIAS_RES h(h(acc + b) + res)     SCALE h(h(acc) * s), s = 100     PATCH h(h(acc) + pos)

QuickGELU alone keeps an inexact tail (the device's exp and reciprocal): the function and the reference's fp16 form are evaluated on
the exact x = acc + b and compared under the bounds test_gemm_quickgelu_one_rounding and test_gemm_f16 use.  The fp32 kernel's
output is the exact sum acc + b + res itself (every term a multiple of 2^-8 below 2^16).

The statistics operands (the second operand set of a "stats" case, operands(c, integer=True)): A = +-1/2, W = +-1, so acc is an integer with |acc| <= K/2; bias and residual are integers in
[-2, 2] and [-8, 8].  The stored rows are integers with |x| <= 64 (asserted), so both per-slot sums -- at most 256 * 64^2 = 2^20 --
are exact in fp32 in any order and are compared bit for bit.
"""
import functools
import math
from typing import NamedTuple

import torch

EPI_NONE, EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RES, EPI_PATCH, EPI_SCALE = range(6)
EPI_NAMES = ("none", "bias", "qgelu", "res", "patch", "scale")
SCALE = 100.0
GEMM_VARIANTS = (0, 6, 8, 9)
SENTINEL = 0x5A5A                       # fp16 203.25 (test_hip_strided.py): compared as bits
SENTINEL32 = 0x5A5A5A5A
PAD_ROWS = 64
CHEAP_FP64 = 1 << 32                    # M * N * K up to which the fp64 product is computed beside the fp32 one
STATS_MAX = 64.0


# ---- which kernel instantiation a launch runs: the dispatcher as it stood BEFORE the library had a routing function -- launch_gemm_f16
# ---- trying the split-K launcher, the tile kernel's launcher and the 128 x 128 kernel in turn, each with its own shape test, and the
# ---- tile launcher's chain of tile height, K loop and hints -- restated branch by branch, in that order.  The library's gemm_f16_route
# ---- (csrc/gemm_f16.hip) is held to this by test_gemm_route_cpu.py; nothing here calls the library. ----

EPI_LN_BIAS, EPI_LN_BIAS_QGELU, EPI_SCALE_ARGMAX = 6, 7, 8


def is_small(M, N):
    return ((M + 63) // 64) * ((N + 63) // 64) <= 256


def _err(rc):
    return ("err", rc)


def _route_v5(loop, M, N, K, epi, ldc, ldres, stats=False, im2col=0):
    """gemm_f16_v5.hip: None where the tile kernel's launcher did not take the shape and handed on (operand pointers are 16-byte aligned, lda = K and the operands of
    the LayerNorm fold and the argmax are present here), ("err", rc) where it returned an error, else
    ("v5", tile rows, K loop, "a_nt" | "", "nt" | "", "g4" | "")."""
    far = M * K * 2 >= 0x7fffffff or N * K * 2 >= 0x7fffffff
    if epi == EPI_SCALE_ARGMAX:                                           # stores no C: no test of N & 7, ldc
        if M < 256 or N < 128 or far:
            return None
    elif M < 256 or N < 128 or (N & 7) or (ldc & 7) or (epi == EPI_BIAS_RES and (ldres & 7)) or far:
        return None
    if im2col:                                                            # rows_in = (R / 16)^2 here
        rows_in = (im2col >> 4) ** 2
        if epi != EPI_PATCH or K != 768 or (im2col & 15) or (M + rows_in - 1) // rows_in * 3 * im2col * im2col * 2 >= 0x7fffffff:
            return _err(-2)
    lnf = epi in (EPI_LN_BIAS, EPI_LN_BIAS_QGELU)
    if lnf and (N & 63):
        return _err(-2)
    if stats and (epi != EPI_BIAS_RES or (N & 255)):
        return _err(-2)
    if loop not in (6, 8):
        return _err(-5)
    if not 0 <= epi <= 8:
        return _err(-3)
    pp = loop == 8 and K % 128 == 0                                       # the ping-pong loop is asked for: two K-tiles per iteration
    tn = (N + 255) // 256
    t256, t128 = ((M + 255) // 256) * tn, ((M + 127) // 128) * tn
    if pp:                                                                # tile height
        big = math.ceil(t256 / 256.0) <= 0.74 * math.ceil(t128 / 256.0)
    else:
        eff = lambda t: t / (math.ceil(t / 256.0) * 256.0)
        big = t256 >= 64 and eff(t256) + 0.08 >= eff(t128)
    bm = 256 if big else 128
    tm = (M + bm - 1) // bm
    pp8 = pp and big                                                      # the kernel: the ping-pong loop is for 256-row tiles
    # the store hint: for every epilogue but BIAS_RES by size; the argmax epilogue stores nothing (its kernels with the bit
    # and without were the same instructions): no hint
    nt = epi not in (EPI_BIAS_RES, EPI_SCALE_ARGMAX) and M * N * 2 >= (48 << 20)
    a_nt = epi == EPI_BIAS_RES and tn <= 4 and tm * tn >= 512
    ov = not pp8 and (lnf or (epi == EPI_BIAS_RES and K >= 2048))         # the boundary loop: LayerNorm fold, or BIAS_RES at K >= 2048
    return ("v5", bm, "pingpong" if pp8 else "boundary" if ov else "double", "a_nt" if a_nt else "", "nt" if nt else "",
            "g4" if pp8 and tn >= 8 else "")


def route(variant, M, N, K, epi, ldc=0, ldres=0, stats=False, im2col=0):
    """The kernel a launch under `variant` runs: ("t128",), ("s64", prefetch depth D, K groups per wave) or _route_v5's tuple; ("err", rc)
    where the launch returns rc without one (0: empty shape).  variant + 100 runs the same kernel (one_rounding_gelu).  im2col: the
    image side R of a patch-gathering launch."""
    ldc = ldc or N
    ldres = ldres or ldc
    if variant >= 100:
        variant %= 100
    if M <= 0 or N <= 0:
        return _err(0)
    if K <= 0 or K % 64:
        return _err(-2)
    loop = 8 if variant in (0, 7, 9) else variant
    if im2col or stats or epi in (EPI_LN_BIAS, EPI_LN_BIAS_QGELU, EPI_SCALE_ARGMAX):   # what only the tile kernel does
        r = _route_v5(loop, M, N, K, epi, ldc, ldres, stats, im2col)
        return _err(-4) if r is None else r
    if (variant == 9 or (variant == 8 and is_small(M, N))) and K >= 128 and K % 128 == 0 and epi in (EPI_NONE, EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RES, EPI_SCALE):
        steps, tiles = K >> 7, ((M + 63) >> 6) * ((N + 63) >> 6)
        D = 4 if steps % 4 == 0 and tiles <= 256 else 3 if steps % 3 == 0 else 2 if steps % 2 == 0 else 1
        return ("s64", D, steps // D)
    if variant >= 1:
        r = _route_v5(loop, M, N, K, epi, ldc, ldres)
        if r is not None:
            return r
    return ("t128",) if 0 <= epi <= EPI_SCALE else _err(-3)


def one_rounding_gelu(variant, epi):
    """variant + 100: the QuickGELU epilogues in the one-rounding form (the tile kernel: template bit 2048)."""
    return variant >= 100 and epi in (EPI_BIAS_QGELU, EPI_LN_BIAS_QGELU)


# ---- the cases -------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    kind: str                   # "f16": ovmr_debug_gemm(0, ...); "strided": ovmr_debug_gemm_strided; "stats": f16 with stats_out; "f32"
    M: int
    N: int
    K: int
    epi: int
    want: dict                  # variant -> the branch this case is in the list for (route()'s tuple): asserted by the CPU test
    rows: tuple = (0, 0)        # EPI_PATCH: (rows_in, rows_out)
    ldc: int = 0                # 0: N
    ldres: int = 0              # 0: in place (res == C, ldres = ldc), as the engine runs its residual projections

    @property
    def id(self):
        s = f"{self.kind}-{self.M}x{self.N}x{self.K}-{EPI_NAMES[self.epi]}"
        return s + (f"-ldc{self.ldc}" if self.ldc else "") + (f"-ldres{self.ldres}" if self.ldres else "")

    @property
    def out_rows(self):
        return self.M // self.rows[0] * self.rows[1] if self.epi == EPI_PATCH else self.M

    @property
    def inplace(self):
        return self.epi == EPI_BIAS_RES and not self.ldres


T128 = ("t128",)
N_, B_, Q_, R_, P_, S_ = EPI_NONE, EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RES, EPI_PATCH, EPI_SCALE


def _v5(bm, loop, a_nt="", nt="", g4=""):
    return ("v5", bm, loop, a_nt, nt, g4)


def _f16(M, N, K, epi, want, **kw):
    return Case("f16", M, N, K, epi, want, **kw)


_PP_M = 17 * 256 - 19           # 4333 rows: 17 row tiles of 256 (the last one part full), 34 of 128
CASES = [
    # -- the 128 x 128 register-staged kernel: variant 0 always; 6 / 8 / 9 wherever the tile kernels refuse (M < 256, N < 128, N & 7)
    #    and the split-K kernel refuses (K < 128 or K % 128).  One K-tile (K = 64), 3 and 48 K-tiles; M around one tile.
    _f16(1, 6, 64, N_, {0: T128, 6: T128, 8: T128, 9: T128}),
    _f16(127, 1003, 192, B_, {0: T128, 6: T128, 8: T128, 9: T128}),
    _f16(128, 136, 3072, R_, {0: T128, 6: T128}),
    _f16(129, 1003, 3072, S_, {0: T128, 6: T128}),                         # N & 7: scalar stores; 6 falls through (M < 256)
    _f16(300, 6, 192, R_, {0: T128, 6: T128, 8: T128, 9: T128}),             # N < 128: 6 / 8 / 9 fall through; ldres = 6: scalar residual loads
    _f16(300, 1003, 64, B_, {0: T128, 6: T128, 8: T128, 9: T128}),           # N & 7 at M >= 256
    _f16(300, 1003, 3072, R_, {0: T128, 6: T128}),                         # N & 7, odd ldc = ldres
    _f16(6 * 49, 136, 128, P_, {0: T128}, rows=(49, 50)),                  # EPI_PATCH, rows_in -> rows_out = 49 -> 50
    _f16(4 * 196, 264, 192, P_, {0: T128, 6: _v5(128, "double"), 8: _v5(128, "double"), 9: _v5(128, "double")}, rows=(196, 197)),
    # -- the split-K 64 x 64 kernel: variant 9 always, variant 8 when is_small.  Depth 4 if steps % 4 == 0 and at most
    #    256 tiles, else 3 / 2 / 1 by divisibility; steps = K / 128 = 1, 2, 3, 5, 16, 24, 32; ragged M and N.
    _f16(63, 72, 128, N_, {8: ("s64", 1, 1), 9: ("s64", 1, 1)}),
    _f16(65, 130, 256, B_, {8: ("s64", 2, 1), 9: ("s64", 2, 1)}),
    _f16(63, 72, 384, R_, {8: ("s64", 3, 1), 9: ("s64", 3, 1)}),
    _f16(65, 130, 640, S_, {8: ("s64", 1, 5), 9: ("s64", 1, 5)}),
    _f16(300, 136, 2048, R_, {8: ("s64", 4, 4), 9: ("s64", 4, 4)}),
    _f16(128, 136, 3072, B_, {8: ("s64", 4, 6), 9: ("s64", 4, 6)}),
    _f16(64, 64, 4096, N_, {8: ("s64", 4, 8), 9: ("s64", 4, 8)}),
    _f16(65, 130, 192, B_, {8: T128, 9: T128}),                            # K % 128 != 0: the split-K kernel hands on (M < 256: to t128)
    _f16(300, 136, 320, R_, {8: _v5(128, "double"), 9: _v5(128, "double")}),  # ... and to the tile kernel
    # -- more than 256 tiles of 64 x 64: variant 8 is past is_small (18 x 16 = 288 tiles), variant 9 runs depth 2 / 3 there.
    #    t256 = 20 < 64: 128-row tiles under 6; under 8 ceil(20/256) = 1 > 0.74 * ceil(36/256): 128-row tiles, double-buffered loop.
    _f16(1100, 1024, 128, R_, {6: _v5(128, "double"), 8: _v5(128, "double"), 9: ("s64", 1, 1)}),          # BIAS_RES: neither a_nt nor ov
    _f16(1100, 1024, 2048, R_, {6: _v5(128, "boundary"), 8: _v5(128, "boundary"), 9: ("s64", 2, 8)}),     # ov alone (K >= 2048, 128-row tiles)
    _f16(1100, 1000, 3072, B_, {9: ("s64", 3, 8), 8: _v5(128, "double")}),
    # -- variant 6 and variant 8 off the ping-pong loop (K % 128 != 0): the small-tile rule t256 >= 64 && eff(256) + 0.08 >= eff(128)
    _f16(300, 256, 64, B_, {6: _v5(128, "double"), 8: _v5(128, "double")}),                               # t256 = 2 < 64; ONE K-tile
    _f16(300, 256, 192, S_, {6: _v5(128, "double"), 8: _v5(128, "double")}),
    _f16(22 * 256 - 19, 768, 320, R_, {6: _v5(128, "double"), 8: _v5(128, "double")}),                    # t256 = 66 >= 64, eff .26 + .08 < .52
    _f16(_PP_M, 2048, 64, N_, {6: _v5(256, "double"), 8: _v5(256, "double")}),                            # t256 = 136, eff .53 = eff(128): 256-row tiles; ONE K-tile
    _f16(_PP_M, 2048, 192, B_, {6: _v5(256, "double"), 8: _v5(256, "double")}),                           # variant 8, K = 192: ping-pong refused
    _f16(_PP_M, 2048, 320, R_, {6: _v5(256, "double"), 8: _v5(256, "double")}),                           # variant 8, K = 320
    # -- 256-row tiles with the ping-pong loop: variant 8, K % 128 == 0, not small, ceil(t256/256) <= 0.74 * ceil(t128/256)
    #    (t256 = 136 -> 1, t128 = 272 -> 2).  n_group = 4 from 8 N tiles on (N = 2048), all N tiles below (N = 768: t256 = 132, t128 = 264).
    _f16(_PP_M, 2048, 128, N_, {8: _v5(256, "pingpong", g4="g4"), 6: _v5(256, "double")}),                # K = 128: one iteration
    _f16(_PP_M, 2048, 256, B_, {8: _v5(256, "pingpong", g4="g4")}),
    _f16(_PP_M, 2048, 4096, B_, {8: _v5(256, "pingpong", g4="g4")}),
    _f16(17 * 256 + 1, 2048, 128, S_, {8: _v5(256, "pingpong", g4="g4")}),                                # M one past a tile
    _f16(44 * 256 - 19, 768, 384, B_, {8: _v5(256, "pingpong")}),                                         # tiles_n = 3; three iterations
    _f16(88 * 49, 2048, 128, P_, {8: _v5(256, "pingpong", g4="g4"), 6: _v5(256, "double")}, rows=(49, 50)),  # EPI_PATCH on 256-row tiles
    _f16(_PP_M, 2048, 128, R_, {8: _v5(256, "pingpong", g4="g4"), 6: _v5(256, "double")}),                # BIAS_RES in place, neither a_nt nor ov
    _f16(_PP_M, 2048, 2048, R_, {6: _v5(256, "boundary"), 8: _v5(256, "pingpong", g4="g4")}),             # ov alone on 256-row tiles (variant 6: no ping-pong loop)
    # -- BIAS_RES in place with the nontemporal A stream: tiles_n <= 4 and at least 512 tiles.
    #    130 900 x 128: 512 tiles of 256 rows (eff 1.0 under 6; 2 <= 0.74 * 4 under 8): a_nt alone, OPT 1 and OPT 16 | 1.
    _f16(130900, 128, 128, R_, {6: _v5(256, "double", "a_nt"), 8: _v5(256, "pingpong", "a_nt")}),
    #    43 600 x 520: t256 = 513 -> 3 rounds, t128 = 1023 -> 4: 3 > 0.74 * 4, the one window where variant 8 prefers 128-row tiles at
    #    512 tiles or more (the engine's batch 221 of 197-token images); under 6 eff .67 + .08 < 1.0 as well.
    _f16(43600, 520, 128, R_, {6: _v5(128, "double", "a_nt"), 8: _v5(128, "double", "a_nt")}),            # a_nt alone (OPT 1)
    _f16(43600, 520, 2048, R_, {6: _v5(128, "boundary", "a_nt"), 8: _v5(128, "boundary", "a_nt")}),       # a_nt and ov (OPT 5)
    #    32 700 x 1000: 128 x 4 = 512 tiles of 256 rows; under variant 6 ov holds on 256-row tiles too: OPT 5 with MT = 8
    _f16(32700, 1000, 2048, R_, {6: _v5(256, "boundary", "a_nt"), 8: _v5(256, "pingpong", "a_nt")}),
    # -- nontemporal stores: M * N * 2 >= 48 MiB, every epilogue but BIAS_RES / PATCH; K = 128.
    #    8200 x 3072: 256-row tiles (396 -> 2 <= 0.74 * 4; eff .77 + .08 >= .76); 10 800 x 3072: 128-row tiles (516 -> 3 > 0.74 * 4; .67 + .08 < 1.0)
    _f16(8200, 3072, 128, N_, {6: _v5(256, "double", nt="nt"), 8: _v5(256, "pingpong", nt="nt", g4="g4")}),
    _f16(8200, 3072, 128, B_, {6: _v5(256, "double", nt="nt"), 8: _v5(256, "pingpong", nt="nt", g4="g4")}),
    _f16(8200, 3072, 128, Q_, {6: _v5(256, "double", nt="nt"), 8: _v5(256, "pingpong", nt="nt", g4="g4")}),
    _f16(8200, 3072, 128, S_, {6: _v5(256, "double", nt="nt"), 8: _v5(256, "pingpong", nt="nt", g4="g4")}),
    _f16(10800, 3072, 128, N_, {6: _v5(128, "double", nt="nt"), 8: _v5(128, "double", nt="nt")}),
    _f16(10800, 3072, 128, B_, {6: _v5(128, "double", nt="nt"), 8: _v5(128, "double", nt="nt")}),
    _f16(10800, 3072, 128, Q_, {6: _v5(128, "double", nt="nt"), 8: _v5(128, "double", nt="nt")}),
    _f16(10800, 3072, 128, S_, {6: _v5(128, "double", nt="nt"), 8: _v5(128, "double", nt="nt")}),
    # -- QuickGELU below the nontemporal threshold: t128, split-K and both tile heights
    _f16(300, 264, 256, Q_, {0: T128, 6: _v5(128, "double"), 8: ("s64", 2, 1)}),
    _f16(_PP_M, 2048, 256, Q_, {6: _v5(256, "double"), 8: _v5(256, "pingpong", g4="g4")}),
    # -- stats_out (BIAS_RES, N % 256 == 0, M >= 256): every variant runs the tile kernel (0 / 9 with the loop of 8)
    Case("stats", 300, 256, 128, R_, {0: _v5(128, "double"), 6: _v5(128, "double"), 8: _v5(128, "double"), 9: _v5(128, "double")}),
    Case("stats", 300, 768, 256, R_, {6: _v5(128, "double"), 8: _v5(128, "double")}),
    Case("stats", 44 * 256 - 19, 768, 128, R_, {8: _v5(256, "pingpong"), 6: _v5(256, "double")}),           # three slots per row, 256-row tiles (132 of them)
    # -- through ovmr_debug_gemm_strided: BIAS_RES with the residual in a buffer of its own stride, and C rows longer than N
    Case("strided", 300, 256, 128, R_, {0: T128, 6: _v5(128, "double"), 8: ("s64", 1, 1)}, ldres=264),     # ldres != ldc
    Case("strided", 129, 136, 128, R_, {0: T128, 9: ("s64", 1, 1)}, ldres=137),                             # odd ldres: scalar residual loads
    Case("strided", 300, 256, 256, R_, {0: T128, 6: _v5(128, "double"), 8: ("s64", 2, 1)}, ldc=272),       # ldc > N, in place
    Case("strided", 1100, 1000, 256, R_, {0: T128, 6: _v5(128, "double"), 8: _v5(128, "double"), 9: ("s64", 2, 1)}, ldc=1024),   # ... ragged N tile
    Case("strided", _PP_M, 2040, 128, B_, {6: _v5(256, "double"), 8: _v5(256, "pingpong", g4="g4")}, ldc=2048),   # ... on 256-row tiles, ragged last N tile
] + [
    # -- fp32 (ovmr_debug_gemm(1, ...)): 64 x 64 tiles, K-tiles of 32; the exact sum is the expected fp32 value
    Case("f32", M, N, K, epi, {})
    for M, N, K, epi in [(1, 4, 32, N_), (63, 100, 96, B_), (64, 128, 512, R_), (65, 130, 2048, N_), (300, 130, 96, R_), (300, 100, 2048, B_),
                         (65, 4, 512, R_), (1, 128, 2048, B_), (63, 130, 32, R_), (64, 100, 512, N_), (300, 128, 32, N_), (300, 4, 96, B_),
                         (300, 130, 512, Q_)]
]

# every ("v5", ...) instantiation class and split-K depth the dispatcher can reach that the list must hold (assert_coverage)
REQUIRED = (
    [T128] + [("s64", d) for d in (1, 2, 3, 4)]
    + [_v5(bm, "double") for bm in (128, 256)] + [_v5(256, "pingpong"), _v5(256, "pingpong", g4="g4")]
    + [_v5(128, "double", nt="nt"), _v5(256, "double", nt="nt"), _v5(256, "pingpong", nt="nt", g4="g4")]
    + [_v5(bm, loop, a) for bm in (128, 256) for loop in ("double", "boundary") for a in ("", "a_nt")] + [_v5(256, "pingpong", "a_nt")]
)


def reached(cases=None):
    """{(epi, branch)} over every case and variant, the split-K kernel by its depth alone."""
    out = set()
    for c in (CASES if cases is None else cases):
        if c.kind == "f32":
            continue
        for v in GEMM_VARIANTS:
            r = route(v, c.M, c.N, c.K, c.epi, c.ldc, c.ldres, c.kind == "stats")
            out.add((c.epi, r[:2] if r[0] == "s64" else r))
    return out


def assert_coverage(cases=None):
    got = reached(cases)
    res = {b for e, b in got if e == EPI_BIAS_RES}
    anyepi = {b for e, b in got}
    missing = [b for b in REQUIRED if b not in (res if (b[0] == "v5" and (b[3] or b[2] == "boundary")) else anyepi)]
    for epi in (EPI_NONE, EPI_BIAS, EPI_BIAS_QGELU, EPI_SCALE):             # nontemporal stores, each epilogue, both tile heights
        missing += [(EPI_NAMES[epi], b) for b in REQUIRED if b[0] == "v5" and b[4] and (epi, b) not in got]
    for epi in range(6):                                                  # every epilogue on every kernel that takes it
        missing += [(EPI_NAMES[epi], k) for k in ("t128", "s64", "v5") if not (k == "s64" and epi == EPI_PATCH)
                    and not any(e == epi and b[0] == k for e, b in got)]
    missing += [(EPI_NAMES[epi], 256, "pingpong") for epi in range(6) if not any(e == epi and b[:3] == ("v5", 256, "pingpong") for e, b in got)]
    assert not missing, f"the case list does not reach: {missing}"


# ---- operands ---------------------------------------------------------------------------------------------------------------

def _signed(g, shape, kmax, dtype=torch.int16):
    """Integers in [-kmax, kmax] without 0, uniform."""
    r = torch.randint(0, 2 * kmax, shape, generator=g, dtype=dtype)
    return r - kmax + (r >= kmax).to(dtype)


@functools.lru_cache(maxsize=2)
def _aw(M, N, K, stats):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    if stats:
        return _signed(g, (M, K), 1, torch.int8).half() / 2, _signed(g, (N, K), 1, torch.int8).half()
    return _signed(g, (M, K), 15, torch.int8).half() / 16, _signed(g, (N, K), 15, torch.int8).half() / 16


def operands(c, integer=False):
    """(A [M, K], W [N, K], bias [N], res [out_rows, N], pos [rows_out, N] or None): fp16, fp32 for an "f32" case.  A and W depend on
    (M, N, K) alone and are shared by the cases of one shape.  integer: the statistics operands (module docstring) of a "stats" case,
    whose output is compared on the standard set as well."""
    stats = integer
    assert not integer or c.kind == "stats"
    A, W = _aw(c.M, c.N, c.K, stats)
    g = torch.Generator().manual_seed(c.M + 5 * c.N + 11 * c.K + 1)
    if stats:
        bias, res, pos = _signed(g, (c.N,), 2).half(), _signed(g, (c.out_rows, c.N), 8).half(), None
    else:
        bias = _signed(g, (c.N,), 512).half() / 256
        res = _signed(g, (c.out_rows, c.N), 2047).half() / 128
        pos = _signed(g, (c.rows[1], c.N), 2047).half() / 128 if c.epi == EPI_PATCH else None
    if c.kind == "f32":
        A, W, bias, res = A.float(), W.float(), bias.float(), res.float()
    return A, W, bias, res, pos


def lowbit_exponent(x, chunk=1 << 24):
    """Smallest p >= 0 such that every element of x (fp16 / fp32, |x| < 2^8, at most 16 fractional bits) is a multiple of 2^-p; no zeros."""
    low = 1 << 16
    flat = x.reshape(-1)
    for i in range(0, flat.numel(), chunk):
        v = flat[i:i + chunk].float().abs() * 65536.0
        vi = v.to(torch.int32)
        assert bool((vi.float() == v).all()) and bool((vi > 0).all()), "an operand that is zero or has more than 16 fractional bits"
        low = min(low, int((vi & -vi).min()))
    return 16 - (low.bit_length() - 1)


def assert_exact(a, b, what):
    """The exactness condition for the products a[i,k] * b[j,k] (head_exact.assert_exact): with p = p_a + p_b every product is a
    multiple of 2^-p, and sum_k |a[i,k] b[j,k]| <= max_i sum_k |a[i,k]| * max |b| < 2^(24 - p).  Sufficient for every partial sum to
    be exact in fp32, in any order."""
    p = lowbit_exponent(a) + lowbit_exponent(b)
    bound = float(a.float().abs().sum(1).max()) * float(b.float().abs().max())      # (the row sums are exact: multiples of 2^-4 below 2^12)
    assert bound < 2.0 ** (24 - p), f"{what}: sum of |products| up to {bound} with p = {p}: not exact in fp32"
    return p, bound


def assert_case_exact(c, ops=None):
    """assert_exact for the product, and the conditions on what the epilogue adds: acc + bias (+ res for fp32) stays a multiple of
    2^-8 below 2^16.  Returns (p, bound)."""
    A, W, bias, res, pos = ops or operands(c)
    p, bound = assert_exact(A, W, c.id)
    assert p <= 8 and bound < c.K <= 4096
    assert lowbit_exponent(bias) <= 8 and float(bias.abs().max()) <= 2
    for t in (res, pos):
        assert t is None or (lowbit_exponent(t) <= 7 and float(t.abs().max()) < 16)
    assert all(t is None or t.dtype == (torch.float32 if c.kind == "f32" else torch.float16) for t in (A, W, bias, res, pos))
    return p, bound


# ---- the reference ----------------------------------------------------------------------------------------------------------

def _h(x):
    return x.half().float()


def product(A, W, check64=None):
    """The exact product as fp32: torch's fp32 matmul on the CPU (exact under assert_exact in whatever order it sums), equal to the
    fp64 product -- asserted where fp64 is cheap."""
    acc = A.float() @ W.float().t()
    if check64 is None:
        check64 = A.shape[0] * W.shape[0] * A.shape[1] <= CHEAP_FP64
    if check64:
        assert torch.equal(acc.double(), A.double() @ W.double().t()), "the fp32 product differs from the fp64 product"
    return acc


def epilogue(c, acc, bias, res, pos, one_rounding=False):
    """The epilogue's rounding points on the exact fp32 product (a row range of it with the matching rows of res).  fp16 tensor; fp32
    for an "f32" case; None for QuickGELU (gelu_forms).  one_rounding: the defect h(acc + b + res) instead of h(h(acc + b) + res)."""
    if c.kind == "f32":
        return {EPI_NONE: acc, EPI_BIAS: acc + bias, EPI_BIAS_RES: acc + bias + res}[c.epi] if c.epi != EPI_BIAS_QGELU else None
    if c.epi == EPI_NONE:
        return acc.half()
    if c.epi == EPI_BIAS:
        return (acc + bias.float()).half()
    if c.epi == EPI_BIAS_RES:
        if one_rounding:
            return (acc + bias.float() + res.float()).half()
        return (_h(acc + bias.float()) + res.float()).half()
    if c.epi == EPI_SCALE:
        return (_h(acc) * SCALE).half()
    if c.epi == EPI_PATCH:                                    # (whole images only: acc holds B * rows_in rows)
        rin, rout = c.rows
        B = acc.shape[0] // rin
        out = torch.zeros((B, rout, c.N), dtype=torch.float16)
        out[:, 1:] = (_h(acc).view(B, rin, c.N) + pos.float()[1:1 + rin]).half()
        return out.view(B * rout, c.N)
    return None


def gelu_forms(acc, bias):
    """(the function x * sigmoid(1.702 x) in fp64, the reference's fp16 form as fp32) on the exact x = acc + bias."""
    return gelu_forms_of((acc + bias.float()).double())


def gelu_forms_of(x):
    """gelu_forms on a given fp64 x (gemm_ln_exact.py: the output of the LayerNorm fold)."""
    u = _h(x.float())
    return x * torch.sigmoid(1.702 * x), _h(u * _h(torch.sigmoid(_h(1.702 * u))))


def expected(c, ops=None):
    """The reference output of a case ([out_rows, N]; for EPI_PATCH the CLS rows are zero and not compared) and the exact product."""
    A, W, bias, res, pos = ops or operands(c)
    acc = product(A, W)
    return epilogue(c, acc, bias, res, pos), acc


def compared_rows(c):
    """Row mask of the output that the comparison covers: all rows but, for EPI_PATCH, the CLS rows (another kernel writes them)."""
    keep = torch.ones(c.out_rows, dtype=torch.bool)
    if c.epi == EPI_PATCH:
        keep[::c.rows[1]] = False
    return keep


def expected_stats(want16):
    """[M, N/256, 2] fp32: (sum, sum of squares) of the stored fp16 row per 256-column slot -- integers below 2^24 (asserted): exact."""
    x = want16.double()
    assert bool((x == x.round()).all()) and float(x.abs().max()) <= STATS_MAX, f"stored rows are not integers within {STATS_MAX}: max |x| = {float(x.abs().max())}"
    x = x.view(x.shape[0], -1, 256)
    st = torch.stack([x.sum(-1), (x * x).sum(-1)], -1)
    assert float(st.abs().max()) < 2 ** 24
    return st.float()


# ---- the comparator ---------------------------------------------------------------------------------------------------------

def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def bits_mismatch(got, want):
    """None if the tensors (fp16 or fp32, same shape) are bit-equal, else: how many elements differ, the first (row, column), its row
    and column modulo 256 and 64 (the tile, the wave and the lane group a defect sits in), and both values with their bit patterns."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    g, w = bits(got), bits(want)
    if torch.equal(g, w):
        return None
    bad = g != w
    r, c = (int(i) for i in bad.nonzero()[0])
    rows = bad.any(1).nonzero().flatten()
    cols = bad.any(0).nonzero().flatten()
    mask, width = (0xffffffff, 8) if got.dtype == torch.float32 else (0xffff, 4)
    return (f"{int(bad.sum())} of {bad.numel()} elements differ, in rows {int(rows[0])}..{int(rows[-1])} and columns {int(cols[0])}..{int(cols[-1])}; "
            f"first at ({r}, {c}) = row {r % 256} of its 256-row tile ({r % 64} mod 64), column {c % 256} of its 256-column tile ({c % 64} mod 64): "
            f"got {float(got[r, c])} (0x{int(g[r, c]) & mask:0{width}x}), want {float(want[r, c])} (0x{int(w[r, c]) & mask:0{width}x})")


def share_differing(got, want):
    return float((bits(got) != bits(want)).float().mean())


def sentinel_buffer(rows, cols, dtype=torch.float16, device="cpu"):
    t = torch.empty((rows, cols), dtype=dtype, device=device)
    bits(t).fill_(SENTINEL32 if dtype == torch.float32 else SENTINEL)
    return t


def outside_untouched(buf, rows, N):
    """buf [rows + PAD_ROWS, ldc]: None if the rows behind `rows` and the columns from N on still hold the sentinel, else what was written."""
    s = SENTINEL32 if buf.dtype == torch.float32 else SENTINEL
    b = bits(buf)
    if not bool((b[rows:] == s).all()):
        r, c = (int(i) for i in (b[rows:] != s).nonzero()[0])
        return f"wrote behind the last row: ({rows + r}, {c})"
    if buf.shape[1] > N and not bool((b[:rows, N:] == s).all()):
        r, c = (int(i) for i in (b[:rows, N:] != s).nonzero()[0])
        return f"wrote into the padding columns: ({r}, {N + c})"
    return None


# ---- a torch emulation of the kernel on a row range, with the defects the comparator must reject ----------------------------------------

def k_tile(c):
    return 32 if c.kind == "f32" else 64


def emulate(c, ops, rows, defect=None, band=None):
    """The output rows `rows` (a slice; whole images for EPI_PATCH) as a kernel computes them -- K-tiles of 64 (fp32 kernel: 32)
    accumulated in fp32 in order, then the epilogue -- optionally with ONE defect:
      "lost_product": one k's contribution missing in the rows of `band` (a slice within the range);
      "tile_twice":   K-tile 0 of A and W read in place of K-tile 1 (two K-tiles at least);
      "one_rounding": h(acc + b + res);        "bias_column": bias from the neighbouring column;
      "res_row":      the residual (positional) row of the neighbouring row."""
    A, W, bias, res, pos = ops
    a, w = A[rows].float(), W.float()
    acc = torch.zeros((a.shape[0], c.N))
    bk = k_tile(c)
    for kt in range(c.K // bk):
        src = 0 if (defect == "tile_twice" and kt == 1) else kt
        acc += a[:, src * bk:src * bk + bk] @ w[:, src * bk:src * bk + bk].t()
    if defect == "lost_product":
        k0 = c.K // 2 + 1
        acc[band] -= a[band, k0, None] * w[None, :, k0]
    if defect == "bias_column":
        bias = bias.roll(1)
    out_rows = slice(rows.start // c.rows[0] * c.rows[1], rows.stop // c.rows[0] * c.rows[1]) if c.epi == EPI_PATCH else rows
    r = res[out_rows]
    if defect == "res_row":
        r, pos = r.roll(1, 0), (pos.roll(1, 0) if pos is not None else None)
    return epilogue(c, acc, bias, r, pos, one_rounding=defect == "one_rounding")
