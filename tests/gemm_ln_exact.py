"""Cases, operands, reference, error budget and comparator for the LayerNorm-folding GEMM epilogues EPI_LN_BIAS / EPI_LN_BIAS_QGELU
(ovmr_amd/csrc/gemm_f16_v5.hip; "the fold") and for the kernels that produce their operands (row_stats_kernel and fold_ln_kernel in
layernorm.hip, the stats_out epilogue).  Plain torch, no library: shared by test_hip_gemm_ln_exact.py (GPU) and
test_gemm_ln_exact_cpu.py (which proves that the comparator accepts honest fp32 evaluations and rejects the defects it is there for).

The method: decided bits under a derived error budget.  rstd = 1 / sqrt(var + 1e-5) cannot be made exact, so the output of the fold is
not ONE bit pattern as gemm_exact's are.  Everything else is exact: the dot product acc (gemm_exact's operands), the per-slot sums
(su, sq) of the statistics (integers far below 2^24), ln_g[n] and ln_b[n] (small dyadic rationals).  The reference is the epilogue's
formula in fp64 on these exact inputs,

    mean = su / K      var = max(sq / K - mean^2, 0)      rstd = 1 / sqrt(var + 1e-5)      x = rstd * (acc - mean * ln_g[n]) + ln_b[n]

and an honest fp32 evaluation differs from x by at most a budget E per element.  With lo = h(x - E) and hi = h(x + E) (h: fp64 ->
fp16, round to nearest even, ONE rounding: h64 below) an element is DECIDED when lo and hi are the same fp16 value, and then the output
must equal it bit for bit; an undecided element must lie in [lo, hi] (with lo and hi neighbours, as they are wherever E is below an
fp16 step, that is "equals lo or hi"; near zero, where an fp16 step is 2^-24, E can span several values and an honest output may be any
of them).  At most 5 % of a case's elements on ordinary rows may be undecided (MAX_UNDECIDED): a condition on the operands, asserted on
the CPU for every case, the same for every variant.

The budget, from the kernel's operation sequence (u = 2^-24, one fp32 rounding; the build runs without contraction and with correctly
rounded division and square root, but nothing below depends on whether sq * inv_k - mean * mean is contracted).  a = 0 where K is a
power of two -- then inv_k, su * inv_k and sq * inv_k are exact -- and a = 1 otherwise:

    inv_k = fl(1 / K)             rel. a u
    mean^ = fl(su * inv_k)        rel. 2a u                                                     (su = sum of the slots: exact)
    msq^  = fl(sq * inv_k)        rel. 2a u
    var^  = fl(msq^ - fl(mean^ * mean^))       |var^ - var| <= dvar = u * (2a msq + (4a + 1) mean^2 + |msq - mean^2|)
    v^    = fl(max(var^, 0) + fl(1e-5))        rel. dv = dvar / (var + 1e-5) + 2u     (the clamp only moves var^ towards var >= 0)
    rstd^ = fl(1 / fl(sqrt(v^)))               rel. rho = (1 - dv)^(-1/2) * (1 + u)^2 - 1       (~ dv / 2 + 2u while dv << 1)
    t^    = fl(-rstd^ * mean^) = -rstd * mean * (1 + rho') (1 + 3u')
    t2^   = fma(t^, ln_g, ln_b)                one rounding of b - rstd * mean * ln_g
    x^    = fma(rstd^, acc, t2^)               one rounding of x

dvar / (var + 1e-5) is the cancellation in the variance: at most (4a + 1) kappa u with kappa = (msq + mean^2) / (var + 1e-5), which the
messages print.  rstd^ * acc + t^ * ln_g = (1 + rho') * ((x - ln_b) - 3u' * rstd * mean * ln_g): the error of rstd is common to both
terms and scales their DIFFERENCE x - ln_b, not each of them.  Hence the bound

    B = (1 + 2^-10) * [ rho * |x - ln_b| + (1 + rho) * u * ( 3 |rstd mean ln_g| + |ln_b - rstd mean ln_g| + |x| ) ]        E = 2 B

((1 + 2^-10): the second-order terms left out).  B holds for the kernel's sequence, and the emulation of that sequence comes to 0.92 B (below);
the test is to hold any honest fp32 evaluation of the formula -- another order of the same operations, a contracted variance, a
reciprocal square root good to an ulp -- so the budget is 2 B, and the honest evaluations are asserted to stay below E / 2 = B.  The
form that was proposed with the test, 2u * [(2 + kappa) |x - ln_b| + 3 |rstd mean ln_g| + |ln_b - rstd mean ln_g| + |x|], has the same
last three terms; its rstd term is 2 (2 + kappa) u against 2 rho ~ dv + 4u here, which is smaller for K a power of two and large
kappa (dv ~ kappa u / 2), larger for kappa near 1 (7u against 6u) and at K = 768 (up to 3.5 kappa u).  E is never tuned against the
device's output.  Three statements keep it honest, all asserted by test_gemm_ln_exact_cpu.py on every case: two honest fp32
emulations -- the kernel's order with two fused multiply-adds, and rstd * (acc - mean * g) + b with every operation rounded -- stay
below E / 2 on every element; the 5 % cap holds; each planted defect is rejected (epsilon 1e-6 for 1e-5 changes 200 .. 370 DECIDED
elements of the 300 x 192 cases).

Degenerate rows, in every case: rows whose statistics say variance exactly 0, and one row whose statistics say a NEGATIVE variance
(sq / K - mean^2 = -1/16: impossible for real data, but it is what the kernel's fmaxf is for -- without it the row is NaN; the
reference clamps as the kernel does).  At K = 768, whose 1 / K is inexact, two rows state var = -1 / K^2 = -1.7e-6 (row_sums: with
dyadic means and variance exactly 0 the fp32 sequence never goes negative, su * fl(1 / K) rounds back to the mean), and the fp32
sequence sees that sign (asserted on the CPU): above -1e-5, so that without the clamp they stay finite, but 9 % off.  On degenerate
rows rstd is about 316, kappa up to 8e5 and almost nothing is decided: they are left out of the 5 % count and compared with
|got - x| <= E + half an fp16 step, and must be finite.

Operands of the epilogue-alone cases (kind "epi": ovmr_debug_gemm with epilogue 6 / 7, operands handed in).  A, W: gemm_exact._aw
(+-k/16, dense, no zeros).  Statistics per row, NOT derived from A, so that every row has its own moments and a misread row shows:
mean_m a multiple of 1/8 in [-2, 2], var_m out of VARS = 1/16 .. 16, assigned from the row index so that rows m and m +- 1, 8, 16,
64, 128 differ (asserted); (K mean, K (var + mean^2)) split unevenly over the K / 256 slots with one all-zero slot and one slot whose
sum is negative -- the pattern row_stats_kernel writes is (everything, 0, 0, ...) -- all multiples of 2^-8 below 2^16, so every order
of adding them is exact; the buffer carries PAD_ROWS rows of NaN behind row M.  ln_g[n] a non-zero multiple of 1/16 in [-4, 4], ln_b[n] a non-zero
multiple of 2^-8 in [-2, 2], neighbouring columns distinct by construction (asserted).

The chains (statistics and folded operands now computed in fp64 from what the device was given):
  "rows"    ovmr_debug_lnfold with A1 == NULL: row_stats_kernel -> fold_ln_kernel -> GEMM.  x1 rows of multiples of 1/4 in [-8, 8], each
            row with its own offset and spread, constant rows among them; gamma in +-{1/2, 1, 2} (h(gamma W) is exact), beta multiples
            of 1/4 in [-1, 1]: row sums, column sums and the folded bias are exact in fp32 in any order (assert_sums_exact);
  "stats"   ovmr_debug_lnfold with A1: the stats_out epilogue -> fold_ln_kernel -> GEMM.  gemm_exact's integer operand set for the first
            GEMM: x1 is integers within 64, compared bit for bit; the expected statistics are those of the expected x1;
  "stride"  ovmr_debug_gemm_strided with epilogue 6 and row_step 1 / 5 / 50 (ln_stride): the rows between the strided ones carry other
            moments, and the result is also bit-equal to the launch on the gathered rows.

Measured (test_gemm_ln_exact_cpu.py and test_hip_gemm_ln_exact.py print them; the emulations on the first 300 rows and the degenerate rows):
    case                               branch under 0/8/9 | under 6, store hint; undecided share; worst err / E of the two evaluations (kernel
    order, separate roundings); MI355X: worst error over E that the device's fp16 output shows on ordinary rows (observed(), all variants)
    epi-300x192x256-ln                 128 boundary | 128 boundary -   undecided  2.88%   err / E 0.300 0.288   MI355X 0.255
    epi-300x192x768-ln                 128 boundary | 128 boundary -   undecided  4.78%   err / E 0.277 0.252   MI355X 0.225
    epi-300x192x1024-ln                128 boundary | 128 boundary -   undecided  4.24%   err / E 0.295 0.280   MI355X 0.255
    epi-300x320x256-ln                 128 boundary | 128 boundary -   undecided  2.80%   err / E 0.341 0.282   MI355X 0.263
    epi-300x320x768-ln                 128 boundary | 128 boundary -   undecided  4.73%   err / E 0.296 0.243   MI355X 0.237
    epi-4333x2048x256-ln               256 pingpong | 256 boundary -   undecided  2.98%   err / E 0.412 0.285   MI355X 0.288
    epi-4333x2048x768-ln               256 pingpong | 256 boundary -   undecided  4.60%   err / E 0.308 0.261   MI355X 0.254
    epi-11245x768x1024-ln              256 pingpong | 256 boundary -   undecided  4.24%   err / E 0.334 0.284   MI355X 0.303
    epi-8200x3072x256-ln               256 pingpong | 256 boundary nt  undecided  2.94%   err / E 0.371 0.286   MI355X 0.307
    epi-10800x3072x256-ln              128 boundary | 128 boundary nt  undecided  2.99%   err / E 0.390 0.288   MI355X 0.299
    rows-300x192x256-ln                128 boundary | 128 boundary -   undecided  1.01%   err / E 0.370 0.282   MI355X 0.109
    rows-300x192x768-ln                128 boundary | 128 boundary -   undecided  1.45%   err / E 0.370 0.302   MI355X 0.147
    rows-300x192x1024-ln               128 boundary | 128 boundary -   undecided  0.97%   err / E 0.408 0.357   MI355X 0.173
    rows-4333x2048x256-ln              256 pingpong | 256 boundary -   undecided  1.00%   err / E 0.438 0.324   MI355X 0.242
    stats-300x192x256-ln-k1_128        128 boundary | 128 boundary -   undecided  0.47%   err / E 0.382 0.320   MI355X 0.146
    stats-300x192x768-ln-k1_128        128 boundary | 128 boundary -   undecided  0.44%   err / E 0.364 0.305   MI355X 0.164
    stats-4333x2048x256-ln-k1_128      256 pingpong | 256 boundary -   undecided  0.44%   err / E 0.460 0.331   MI355X 0.291
    stride-300x192x768-ln-step1        128 boundary | 128 boundary -   undecided  1.45%   err / E 0.370 0.302   MI355X 0.147
    stride-300x192x768-ln-step5        128 boundary | 128 boundary -   undecided  1.33%   err / E 0.353 0.301   MI355X 0.160
    stride-300x192x256-ln-step50       128 boundary | 128 boundary -   undecided  0.97%   err / E 0.370 0.285   MI355X 0.144
    stride-4333x2048x256-ln-step5      256 pingpong | 256 boundary -   undecided  0.99%   err / E 0.423 0.335   MI355X 0.259
(the epilogue-7 cases share operands, reference and shares with the epilogue-6 case of their shape).
"""
import functools
from typing import NamedTuple

import torch

import gemm_exact as G
from gemm_exact import EPI_LN_BIAS, EPI_LN_BIAS_QGELU, PAD_ROWS, _PP_M, _v5

U = 2.0 ** -24
EPS = 1e-5
MAX_UNDECIDED = 0.05
VARS = (1 / 16, 1 / 4, 1.0, 4.0, 16.0)
STEPS = (1, 8, 16, 64, 128)             # row distances at which the moments must differ
PLAIN, ONE_ROUNDING = (0, 6, 8, 9), (100, 106, 108)
PRODUCERS = {"rows": "row_stats_kernel and fold_ln_kernel (layernorm.hip)",
             "stats": "the stats_out epilogue of the first GEMM (gemm_f16_v5.hip) and fold_ln_kernel (layernorm.hip)",
             "stride": "row_stats_kernel and fold_ln_kernel (layernorm.hip), the statistics read with ln_stride = row_step * K / 256"}


# ---- the cases --------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    kind: str                   # "epi" | "rows" | "stats" | "stride" (module docstring)
    M: int                      # rows of the folding GEMM (stride: the strided rows)
    N: int
    K: int                      # = the LayerNorm width D
    epi: int
    want: dict                  # variant -> the branch of the folding GEMM this case is in the list for (gemm_exact.route's tuple)
    step: int = 1               # "stride": row_step
    K1: int = 0                 # "stats": K of the first GEMM

    @property
    def id(self):
        s = f"{self.kind}-{self.M}x{self.N}x{self.K}-{'ln' if self.epi == EPI_LN_BIAS else 'lnqgelu'}"
        return s + (f"-step{self.step}" if self.kind == "stride" else "") + (f"-k1_{self.K1}" if self.K1 else "")

    @property
    def variants(self):
        return tuple(self.want)


def _want(r6, r8, epi=EPI_LN_BIAS):
    """Variants 0 and 9 run the K loop of 8; variants + 100: the same kernels with the one-rounding QuickGELU."""
    w = {0: r8, 6: r6, 8: r8, 9: r8}
    if epi == EPI_LN_BIAS_QGELU:
        w.update({100: r8, 106: r6, 108: r8})
    return w


_B128, _B256 = _v5(128, "boundary"), _v5(256, "boundary")
_SHAPES = {     # (M, N) -> (branch under 6, under 8)
    (300, 192): (_B128, _B128),                                            # one ragged N tile (192 of 256 columns), ragged last row tile
    (300, 320): (_B128, _B128),                                            # two N tiles, the last with 64 columns
    (_PP_M, 2048): (_B256, _v5(256, "pingpong", g4="g4")),
    (44 * 256 - 19, 768): (_B256, _v5(256, "pingpong")),                   # three N tiles: no g4
    (8200, 3072): (_v5(256, "boundary", nt="nt"), _v5(256, "pingpong", nt="nt", g4="g4")),      # the store hint, 256-row tiles
    (10800, 3072): (_v5(128, "boundary", nt="nt"), _v5(128, "boundary", nt="nt")),              # ... and 128-row tiles
}


def _case(kind, M, N, K, epi=EPI_LN_BIAS, **kw):
    return Case(kind, M, N, K, epi, _want(*_SHAPES[(M, N)], epi=epi), **kw)


CASES = [
    # -- 1. the epilogue alone, epilogue 6: 128-row tiles with the boundary loop at all three K (1, 3 and 4 slots)
    _case("epi", 300, 192, 256), _case("epi", 300, 192, 768), _case("epi", 300, 192, 1024),
    _case("epi", 300, 320, 256), _case("epi", 300, 320, 768),
    #    256-row tiles: the boundary loop under 6, the ping-pong loop (its own copy of the prologue) under 0 / 8 / 9
    _case("epi", _PP_M, 2048, 256), _case("epi", _PP_M, 2048, 768),
    _case("epi", 44 * 256 - 19, 768, 1024),
    #    the store hint at both tile heights
    _case("epi", 8200, 3072, 256), _case("epi", 10800, 3072, 256),
    # -- 2. epilogue 7, one shape per class; variants + 100: the one-rounding form
    _case("epi", 300, 192, 768, EPI_LN_BIAS_QGELU), _case("epi", _PP_M, 2048, 256, EPI_LN_BIAS_QGELU),
    _case("epi", 8200, 3072, 256, EPI_LN_BIAS_QGELU), _case("epi", 10800, 3072, 256, EPI_LN_BIAS_QGELU),
    # -- 3. the producing kernels, chained
    _case("rows", 300, 192, 256), _case("rows", 300, 192, 768), _case("rows", 300, 192, 1024), _case("rows", _PP_M, 2048, 256),
    _case("stats", 300, 192, 256, K1=128), _case("stats", 300, 192, 768, K1=128), _case("stats", _PP_M, 2048, 256, K1=128),
    _case("stride", 300, 192, 768, step=1), _case("stride", 300, 192, 768, step=5), _case("stride", 300, 192, 256, step=50),
    _case("stride", _PP_M, 2048, 256, step=5),                             # ln_stride in the ping-pong prologue's copy
]

# every (epilogue, one-rounding QuickGELU, tile rows, K loop, store hint) class the tile kernel's table holds for the LN epilogues:
# V5_STORES(V5_BOUNDARY_PP, ...) three times = 18 instantiations
REQUIRED = [(epi, fast, bm, loop, nt) for epi, fast in ((EPI_LN_BIAS, False), (EPI_LN_BIAS_QGELU, False), (EPI_LN_BIAS_QGELU, True))
            for bm, loop in ((128, "boundary"), (256, "boundary"), (256, "pingpong")) for nt in ("", "nt")]


def reached(cases=None, kinds=("epi",)):
    out = set()
    for c in (CASES if cases is None else cases):
        if c.kind in kinds:
            for v in c.variants:
                r = G.route(v, c.M, c.N, c.K, c.epi)
                out.add((c.epi, G.one_rounding_gelu(v, c.epi), r[1], r[2], r[4]) if r[0] == "v5" else r)
    return out


def assert_coverage(cases=None):
    """The epilogue-alone cases reach every instantiation class of REQUIRED; both n_group arms of the ping-pong loop; every chain
    runs on 128-row tiles, on the 256-row boundary loop and on the ping-pong loop."""
    got = reached(cases)
    missing = [r for r in REQUIRED if r not in got]
    cs = CASES if cases is None else cases
    g4 = {G.route(v, c.M, c.N, c.K, c.epi)[5] for c in cs if c.kind == "epi" for v in c.variants if G.route(v, c.M, c.N, c.K, c.epi)[2:3] == ("pingpong",)}
    missing += [("n_group", x) for x in ("", "g4") if x not in g4]
    for kind in PRODUCERS:
        loops = {r[2:4] for r in reached(cases, (kind,))}
        missing += [(kind, bm, loop) for bm, loop in ((128, "boundary"), (256, "boundary"), (256, "pingpong")) if (bm, loop) not in loops]
    assert not missing, f"the case list does not reach: {missing}"


# ---- rounding fp64 -> fp16 once ------------------------------------------------------------------------------------------------

def h64(y):
    """fp64 -> fp16, round to nearest even, ONE rounding.  Through fp32 rounded TO ODD (truncate, then set the last bit if anything was
    cut off), after which the second rounding cannot go wrong: fp32 carries more than two bits beyond fp16's (test_gemm_ln_exact_cpu.py
    holds this against numpy's direct conversion on ties and their fp64 neighbours)."""
    f = y.float()
    back = f.double()
    t = torch.where(back.abs() > y.abs(), torch.nextafter(f, torch.zeros_like(f)), f)
    odd = t.view(torch.int32) | (back != y).to(torch.int32)
    return odd.view(torch.float32).half()


def half_step(v):
    """Half the fp16 spacing at magnitude v (fp64)."""
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 11)


# ---- operands ------------------------------------------------------------------------------------------------------------------

def _kernel_var32(su, sq, K):
    """sq * inv_k - mean * mean as the kernel's fp32 sequence gives it (before the clamp)."""
    inv_k = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(K), dtype=torch.float32)
    mean = su.float() * inv_k
    return sq.float() * inv_k - mean * mean


def degenerate_rows(M):
    """Row -> kind.  No two of them 1, 8, 16, 64 or 128 apart; one in the last row tile."""
    return {3: "zero", 70: "tiny", 141: "zero", 200: "stated", 259: "tiny", M - 2: "zero"}


def row_sums(M, K):
    """(su [M], sq [M], degenerate [M] bool, mean [M], var [M]), fp64; var is what the statistics STATE.  Ordinary rows: mean a
    multiple of 1/8, var out of VARS.  "zero": var = 0.  "stated": var = -1/16.  "tiny", where 1 / K is inexact (K = 768; elsewhere
    as "zero"): su = K mean + 1 and sq = (su^2 - 1) / K, a multiple of 1/4 -- the statistics state var = -1 / K^2 = -1.7e-6, which
    the fp32 sequence must see as negative too (with dyadic means and variance exactly 0 it never does: su * fl(1 / K) rounds back
    to the mean)."""
    m = torch.arange(M)
    mean = ((m * 5) % 33 - 16).double() / 8
    var = torch.tensor(VARS, dtype=torch.float64)[(m // 2 + m // 16) % 5]
    deg = torch.zeros(M, dtype=torch.bool)
    kinds = degenerate_rows(M)
    for r, kind in kinds.items():
        deg[r] = True
        var[r] = -1 / 16 if kind == "stated" else 0.0
    mean[3] = 0.0                                                        # (0, 0): rstd = 1 / sqrt(1e-5) with nothing to cancel
    su, sq = K * mean, K * (var + mean * mean)
    if K & (K - 1):
        for r in (r for r, kind in kinds.items() if kind == "tiny"):
            su[r] += 1
            sq[r] = (su[r] * su[r] - 1) / K
            assert float(sq[r] * 4) == round(float(sq[r] * 4)) and float(sq[r]) * K == float(su[r]) ** 2 - 1
    return su, sq, deg, su / K, sq / K - (su / K) ** 2


def assert_rows_distinct(mean, var):
    for d in STEPS:
        if d < mean.numel():
            assert bool(((mean[d:] != mean[:-d]) | (var[d:] != var[:-d])).all()), f"rows {d} apart share their moments"


def slot_split(su, sq, K):
    """[M, K/256, 2] fp32: (su, sq) split unevenly over the slots -- slot 1 all zero, the last slot with a negative sum (both only
    where there is more than one slot); multiples of 2^-8 below 2^16, so that adding them in any order is exact (asserted)."""
    M, S = su.numel(), K // 256
    m = torch.arange(M)
    st = torch.zeros((M, S, 2), dtype=torch.float64)
    if S > 1:
        st[:, S - 1, 0] = -64.0 * (1 + m % 3)
        st[:, S - 1, 1] = 16.0 * (1 + m % 5)
    if S > 3:
        st[:, 2, 0] = 32.0 * (1 + m % 7)
        st[:, 2, 1] = 8.0 * (1 + m % 11)
    st[:, 0, 0] = su - st[:, 1:, 0].sum(1)
    st[:, 0, 1] = sq - st[:, 1:, 1].sum(1)
    assert bool((st * 256 == (st * 256).round()).all()) and float(st.abs().sum(1).max()) < 2 ** 16, "statistics partials are not exact in fp32"
    assert torch.equal(st.sum(1), torch.stack([su, sq], 1))
    if S > 1:
        assert bool((st[:, 1] == 0).all()) and bool((st[:, S - 1, 0] < 0).all()) and bool((st[:, 0] != 0).any(1).all())
    return st.float()


def columns(N, seed):
    """(ln_g [N], ln_b [N]) fp32: non-zero multiples of 1/16 in [-4, 4] and of 2^-8 in [-2, 2]; a walk with non-zero steps, so that
    neighbouring columns differ in both."""
    gen = torch.Generator().manual_seed(seed)

    def walk(kmax):
        k = torch.randint(1, 2 * kmax, (N,), generator=gen).cumsum(0) % (2 * kmax)      # 0 .. 2 kmax - 1, neighbours distinct
        return (k - kmax + (k >= kmax).long()).float()                                  # -kmax .. -1, 1 .. kmax
    g, b = walk(64) / 16, walk(512) / 256
    assert bool((g != 0).all()) and bool((b != 0).all()) and float(g.abs().max()) <= 4 and float(b.abs().max()) <= 2
    assert bool((g[1:] != g[:-1]).all()) and bool((b[1:] != b[:-1]).all())
    return g, b


def lowbit(x):
    """Smallest p >= 0 with every element of x a multiple of 2^-p (zeros allowed, unlike gemm_exact.lowbit_exponent; |x| < 2^15)."""
    v = x.double().abs() * 65536.0
    vi = v.to(torch.int64)
    assert bool((vi.double() == v).all()), "more than 16 fractional bits"
    vi = vi[vi > 0]
    low = int((vi & -vi).min()) if vi.numel() else 1 << 16
    return max(0, 16 - (low.bit_length() - 1))


def assert_sums_exact(t, what, other=1.0, p_other=0):
    """Every partial sum of a row of t (times a factor below `other`, a multiple of 2^-p_other) is exact in fp32, in any order."""
    p = lowbit(t) + p_other
    bound = float(t.double().abs().sum(-1).max()) * other
    assert bound < 2.0 ** (24 - p), f"{what}: sums of magnitudes up to {bound} in units of 2^-{p}: not exact in fp32"


class Operands(NamedTuple):
    A: torch.Tensor             # fp16 [rows, K]: the folding GEMM's A ("stride": the dense buffer it strides over)
    W: torch.Tensor             # fp16 [N, K]: the weight the GEMM multiplies by (chains: h(gamma W), computed here in fp64)
    g: torch.Tensor             # fp32 [N] ln_g
    b: torch.Tensor             # fp32 [N] ln_b
    stats: torch.Tensor         # fp32 [M, K/256, 2] of the GEMM's rows: what the producer must write (epi: what is handed in)
    su: torch.Tensor            # fp64 [M]
    sq: torch.Tensor            # fp64 [M]
    deg: torch.Tensor           # bool [M]
    raw: dict                   # chains: what the device is given (W2, gamma, beta, b2; stats: the first GEMM's case and operands, x1)


def _seed(c):
    return c.M * 13 + c.N * 5 + c.K * 3 + 7


def ln_rows(R, D, seed, constant=()):
    """fp16 [R, D]: multiples of 1/4 in [-8, 8], row m = offset_m + spread_m * {-3 .. 3}; the rows `constant` hold their offset alone."""
    gen = torch.Generator().manual_seed(seed)
    m = torch.arange(R)
    offset = ((m * 3) % 17 - 8).double() / 4
    spread = torch.tensor([0.25, 0.5, 1.0, 2.0], dtype=torch.float64)[(m // 3 + m // 17) % 4]
    r = torch.randint(-3, 4, (R, D), generator=gen, dtype=torch.int8).double()
    r[list(constant)] = 0
    x = offset[:, None] + spread[:, None] * r
    return x.half()


@functools.lru_cache(maxsize=2)
def _operands(c):
    if c.kind == "epi":
        A, W = G._aw(c.M, c.N, c.K, False)
        G.assert_exact(A, W, c.id)
        g, b = columns(c.N, _seed(c))
        su, sq, deg, mean, var = row_sums(c.M, c.K)
        assert_rows_distinct(mean, var)
        return Operands(A, W, g, b, slot_split(su, sq, c.K), su, sq, deg, {})
    gen = torch.Generator().manual_seed(_seed(c))
    D = c.K
    W2 = G._aw(c.M, c.N, D, False)[1]
    gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (D,), generator=gen)] * (torch.randint(0, 2, (D,), generator=gen) * 2 - 1).float()
    beta = torch.randint(-4, 5, (D,), generator=gen).float() / 4
    b2 = G._signed(gen, (c.N,), 512).half() / 256
    raw = {"W2": W2, "gamma": gamma, "beta": beta, "b2": b2}
    if c.kind == "stats":
        c1 = G.Case("stats", c.M, D, c.K1, G.EPI_BIAS_RES, {})
        ops1 = G.operands(c1, integer=True)
        G.assert_exact(ops1[0], ops1[1], c.id + " (first GEMM)")
        x1 = G.expected(c1, ops1)[0]
        dense, rows = x1, x1
        raw.update(c1=c1, ops1=ops1, x1=x1, stats1=G.expected_stats(x1))
    else:
        R = (c.M - 1) * c.step + 1
        dense = ln_rows(R, D, _seed(c) + 1, constant=[r * c.step for r in degenerate_rows(c.M)])
        rows = dense[::c.step]
        assert rows.shape[0] == c.M
        if c.step > 1:                                                   # the rows in between carry other moments
            nxt = dense[1::c.step][:c.M - 1].double()
            mine = rows[:c.M - 1].double()
            assert bool(((nxt.sum(1) != mine.sum(1)) | ((nxt * nxt).sum(1) != (mine * mine).sum(1))).all())
    # the folded operands, in fp64 from what the device is given; every one of them exact in fp32 in any order
    wf64 = gamma.double()[None] * W2.double()
    wf = wf64.half()
    assert torch.equal(wf.double(), wf64), "h(gamma W) is not exact"
    assert_sums_exact(wf, c.id + ": column sums of the folded weight")
    bw = beta.double()[None] * W2.double()
    assert_sums_exact(bw, c.id + ": beta W")
    g64, b64 = wf64.sum(1), b2.double() + bw.sum(1)
    assert lowbit(b64) <= 8 and float(b64.abs().max()) < 2 ** 15 and torch.equal(g64.float().double(), g64) and torch.equal(b64.float().double(), b64)
    x = rows.double()
    assert_sums_exact(x, c.id + ": row sums")
    assert_sums_exact(x * x, c.id + ": row sums of squares")
    assert_sums_exact(x, c.id + ": the dot products", other=float(wf64.abs().max()), p_other=lowbit(wf))
    su, sq = x.sum(1), (x * x).sum(1)
    deg = sq * D == su * su                                              # variance exactly 0: the constant rows
    S = D // 256
    if c.kind == "stats":
        stats = raw["stats1"]
    else:                                                                # row_stats_kernel: slot 0 holds everything
        stats = torch.zeros((c.M, S, 2), dtype=torch.float32)
        stats[:, 0, 0], stats[:, 0, 1] = su.float(), sq.float()
    assert torch.equal(stats.double().sum(1), torch.stack([su, sq], 1))
    return Operands(dense, wf, g64.float(), b64.float(), stats, su, sq, deg, raw)


def operands(c):
    """The operands of a case; the two epilogues of one shape share them."""
    return _operands(c._replace(epi=EPI_LN_BIAS, want=None))


def gemm_rows(c, ops):
    """The rows the folding GEMM reads: fp16 [M, K]."""
    return ops.A[::c.step] if c.kind == "stride" else ops.A


def stats_buffer(ops):
    """The statistics as ovmr_debug_gemm takes them: [M + PAD_ROWS, K/256, 2] fp32, NaN behind row M."""
    M, S, _ = ops.stats.shape
    buf = torch.full((M + PAD_ROWS, S, 2), float("nan"), dtype=torch.float32)
    buf[:M] = ops.stats
    return buf


# ---- the reference and its budget --------------------------------------------------------------------------------------------

class Reference(NamedTuple):
    x: torch.Tensor             # fp64 [M, N]: the epilogue's formula on the exact inputs
    E: torch.Tensor             # fp64 [M, N]: the budget
    lo: torch.Tensor            # fp16: h(x - E)
    hi: torch.Tensor            # fp16: h(x + E)
    deg: torch.Tensor           # bool [M]: degenerate rows
    kappa: torch.Tensor         # fp64 [M]

    def to(self, device):
        return Reference(*(t.to(device) for t in self))

    def rows(self, idx):
        return Reference(*(t[idx] for t in self))


def row_terms(su, sq, K):
    """(mean, rstd, rho, kappa) per row, fp64 (module docstring)."""
    mean, msq = su / K, sq / K
    var = (msq - mean * mean).clamp_min(0.0)
    v = var + EPS
    kappa = (msq.abs() + mean * mean) / v
    a = 0 if K & (K - 1) == 0 else 1                                     # 1 / K, and with it su / K and sq / K, exact or not
    dv = U * ((2 * a * msq.abs() + (4 * a + 1) * mean * mean + (msq - mean * mean).abs()) / v + 2)
    assert float(dv.max()) < 0.5, f"kappa up to {float(kappa.max())}: the variance is lost in its own rounding"
    rho = (1 - dv) ** -0.5 * (1 + U) ** 2 - 1
    return mean, 1 / v.sqrt(), rho, kappa


def reference(acc, su, sq, g, b, K, deg):
    """acc: the exact product (fp32 or fp64, [M, N]); su, sq fp64 [M]; g, b [N]."""
    mean, rstd, rho, kappa = row_terms(su, sq, K)
    g, b = g.double()[None], b.double()[None]
    acc = acc.double()
    x = rstd[:, None] * (acc - mean[:, None] * g) + b
    rmg = (rstd * mean)[:, None] * g
    E = rho[:, None] * (x - b).abs()
    E += ((1 + rho) * U)[:, None] * (3 * rmg.abs() + (b - rmg).abs() + x.abs())
    E *= 2 * (1 + 2.0 ** -10)
    del rmg
    assert bool(torch.isfinite(x).all()) and float((x.abs() + E).max()) < 60000, "the reference leaves the fp16 range"
    return Reference(x, E, h64(x - E), h64(x + E), deg, kappa)


@functools.lru_cache(maxsize=1)
def _expected(c):
    ops = operands(c)
    acc = G.product(gemm_rows(c, ops), ops.W)
    return reference(acc, ops.su, ops.sq, ops.g, ops.b, c.K, ops.deg), acc


def expected(c):
    """(Reference, the exact product) of a case; cases of one shape and kind share neither operands nor reference (the epilogues do)."""
    return _expected(c._replace(epi=EPI_LN_BIAS, want=None))


def undecided_share(ref):
    """Share of the elements on ordinary rows whose fp16 value the budget does not decide."""
    und = G.bits(ref.lo) != G.bits(ref.hi)
    return float(und[~ref.deg].float().mean())


# ---- the comparator ---------------------------------------------------------------------------------------------------------

def _ok(got, ref):
    gf = got.double()
    decided = G.bits(ref.lo) == G.bits(ref.hi)
    ordinary = torch.where(decided, G.bits(got) == G.bits(ref.lo), (gf >= ref.lo.double()) & (gf <= ref.hi.double()))
    degenerate = torch.isfinite(gf) & ((gf - ref.x).abs() <= ref.E + half_step(ref.x.abs() + ref.E))
    return torch.where(ref.deg[:, None], degenerate, ordinary), decided


def ln_mismatch(got, ref, producers=None, sums=None):
    """None if the fp16 output `got` passes (module docstring: decided elements bit-equal, undecided ones within [lo, hi], degenerate
    rows finite and within E + half an fp16 step), else, after gemm_exact.bits_mismatch: how many elements fail, the first (row,
    column), both modulo 256 and 64, got / want / E and whether the element was decided.  producers: for a chain, the kernels in
    front of the GEMM, named in the message with the row's expected (su, sq) = sums[row]."""
    assert got.shape == ref.x.shape and got.dtype == torch.float16, f"{tuple(got.shape)} {got.dtype} against {tuple(ref.x.shape)}"
    ok, decided = _ok(got, ref)
    if bool(ok.all()):
        return None
    bad = ~ok
    r, c = (int(i) for i in bad.nonzero()[0])
    rows, cols = bad.any(1).nonzero().flatten(), bad.any(0).nonzero().flatten()
    state = "a degenerate row: within E + half an fp16 step" if bool(ref.deg[r]) else \
        "decided: bit equality" if bool(decided[r, c]) else "undecided: within [lo, hi]"
    msg = (f"{int(bad.sum())} of {bad.numel()} elements fail ({int((bad & decided & ~ref.deg[:, None]).sum())} of them decided), in rows {int(rows[0])}..{int(rows[-1])} "
           f"and columns {int(cols[0])}..{int(cols[-1])}; first at ({r}, {c}) = row {r % 256} of its 256-row tile ({r % 64} mod 64), column {c % 256} of its "
           f"256-column tile ({c % 64} mod 64): got {float(got[r, c])} (0x{int(G.bits(got)[r, c]) & 0xffff:04x}), want x = {float(ref.x[r, c]):.9g}, "
           f"lo {float(ref.lo[r, c])} (0x{int(G.bits(ref.lo)[r, c]) & 0xffff:04x}), hi {float(ref.hi[r, c])} (0x{int(G.bits(ref.hi)[r, c]) & 0xffff:04x}), "
           f"E = {float(ref.E[r, c]):.3e}, kappa {float(ref.kappa[r]):.3g}; {state}")
    if producers:
        msg += (f".  The epilogue-alone cases hold the GEMM's own prologue and epilogue on handed-in operands: if they pass, look at {producers}; "
                f"row {r} expects (su, sq) = ({float(sums[0][r])}, {float(sums[1][r])})")
    return msg


def _toward(got, direction):
    """The fp16 neighbour of got in `direction` (-1, 0, 1 per element), as fp64."""
    b = G.bits(got).int()
    o = torch.where(b < 0, -(b & 0x7fff), b) + direction
    mag = o.abs().to(torch.int16).view(torch.float16).double()
    return torch.where(o < 0, -mag, mag)


def observed(got, ref):
    """What the fp16 output shows of the fp32 error, over E, per element: the distance from x to the interval of reals that round to
    got (0 where got = h(x)).  A lower bound of |x^ - x| / E, and all that can be seen behind the output's rounding."""
    gf = got.double()
    s = torch.sign(ref.x - gf).int()
    tie = (gf + _toward(got, s)) / 2
    return ((ref.x - tie) * s).clamp_min(0.0) / ref.E


def worst_observed(got, ref):
    o = observed(got, ref)
    return float(o[~ref.deg].max()), float(o[ref.deg].max()) if bool(ref.deg.any()) else 0.0


# ---- honest fp32 evaluations, and the defects the comparator must reject --------------------------------------------------------------

DEFECTS = ("stats_row+1", "stats_row-1", "stats_row+16", "stats_row-16", "g_col+1", "g_col-1", "b_col+1", "b_col-1", "drop_last_slot",
           "zero_slot_copy", "eps_1e-6", "plus_mean", "no_clamp", "no_mean_in_var", "inv_n")


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emulate(c, ops, acc, rows, order="fma", defect=None):
    """The fp32 value in front of the fp16 conversion for the rows `rows` (an index tensor), every operation rounded to fp32:
    order "fma": the kernel's sequence -- slots added in order, mean = su * inv_k, t = -rstd * mean, two fused multiply-adds;
    order "separate": rstd * (acc - mean * g) + b.  defect: one of DEFECTS (the statistics of another row, ln_g / ln_b of another
    column, a dropped last slot, the zero slot a copy of slot 0, epsilon 1e-6, +rstd * mean, no clamp at zero, the mean forgotten in
    the variance, 1/N for 1/K)."""
    f = torch.float32
    st = ops.stats.clone()
    g, b = ops.g.clone(), ops.b.clone()
    if defect and defect.startswith("stats_row"):
        st = st.roll(-int(defect[9:]), 0)
    if defect and defect[1:5] == "_col":
        g, b = (g.roll(-int(defect[5:])), b) if defect[0] == "g" else (g, b.roll(-int(defect[5:])))
    if defect == "drop_last_slot":
        st[:, -1] = 0
    if defect == "zero_slot_copy":
        assert st.shape[1] > 1
        st[:, 1] = st[:, 0]
    st = st[rows]
    su, sq = torch.zeros(st.shape[0], dtype=f), torch.zeros(st.shape[0], dtype=f)
    for s in range(st.shape[1]):
        su, sq = su + st[:, s, 0], sq + st[:, s, 1]
    inv_k = torch.tensor(1.0, dtype=f) / torch.tensor(float(c.N if defect == "inv_n" else c.K), dtype=f)
    mean = su * inv_k
    var = sq * inv_k if defect == "no_mean_in_var" else sq * inv_k - mean * mean
    if defect != "no_clamp":
        var = torch.maximum(var, torch.zeros((), dtype=f))
    rstd = 1.0 / torch.sqrt(var + torch.tensor(1e-6 if defect == "eps_1e-6" else 1e-5, dtype=f))
    a = acc[rows].float()
    sign = 1.0 if defect == "plus_mean" else -1.0
    if order == "fma":
        t = sign * (rstd * mean)
        return _fma32(rstd[:, None], a, _fma32(t[:, None], g[None], b[None]))
    return rstd[:, None] * (a + sign * (mean[:, None] * g[None])) + b[None]


def emulation_rows(c, ops):
    """The rows the emulations run on: the first 300 and every degenerate row."""
    idx = set(range(min(c.M, 300))) | set(ops.deg.nonzero().flatten().tolist())
    return torch.tensor(sorted(idx))
