"""Cases, operands, fp64 references, budgets and comparators for the row kernels that sit between the GEMMs: layernorm_rows
(ovmr_amd/csrc/layernorm.hip), l2norm_f16_kernel and the text front (text_embed_ids_kernel, argmax_ids_kernel, text_add_pos_kernel,
gather_rows_kernel, embed_gather_kernel, assemble_prompts_kernel: rowops.hip) and the prompt ensemble (text_ensemble.hip).  Plain torch,
no library: shared by test_hip_rowops_exact.py (GPU) and test_rowops_exact_cpu.py (which proves that the comparators accept honest
evaluations and reject the defects they are there for).  Nothing here is compared at a tolerance.

Three methods, in the order of how much of the kernel's arithmetic can be made exact.

1. ONE bit pattern (the text front, embed_tokens, assemble_prompts; the "exact" operand set of the L2 norm; everything in the ensemble
   but its last norm).  Every element is a copy or takes the stated single roundings of exact quantities: h(tok) (fp32 -> fp16), the
   sum of two fp16 values (exact in fp64, rounded to fp32 and then to fp16 as the kernels do), a quotient or a square root (the build
   has correctly rounded fp32 division and square root, and 53 >= 2 * 24 + 2, so the fp64 operation rounded to fp32 IS the fp32
   operation: h32 below).  Tables carry their own row and column in their values (tok_table, pos_table, prompt_table: rows v and v + k,
   columns c and c + k differ for every k below 2039 resp. 1021), ids tie at their maximum (the first one wins, as in torch.argmax),
   and the gather gets indices outside [0, Lseq), which it clamps.

2. At most TWO whole rows (the L2 norm of arbitrary fp16 values -- the "model-like" set, what a second application sees, and the
   ensemble's last norm).  The squares of fp16 values are exact in fp32; their sum, in ANY order, carries at most
   gamma = (D - 1) u / (1 - (D - 1) u) relative error (u = 2^-24), the square root halves it, and fp16 values are 2^-11 .. 2^-10
   apart: n = h(sqrt(ss^)) is one of the fp16 values between h(sqrt(ss (1 - gamma))) and h(sqrt(ss (1 + gamma))), at most two
   (asserted for every row of every case: l2_apply).  The output row must be bit-equal, AS A WHOLE ROW, to h(x / n) for one of them;
   two applications give at most four rows.  Nothing is left out.  On the "exact" set (multiples of 1/16 in [-2, 2]: the sum of
   squares is a multiple of 2^-8 below 2^13, exact in fp32 in any order) gamma is 0 and there is one row.  Pinned rows in every case:
   an all-zero row (the kernel's 1e-12 clamp keeps it zero where torch gives NaN) and a row whose norm overflows fp16 (+-40000: the
   quotients are signed zeros; bits are compared).

3. Decided bits under a derived budget (LayerNorm, fp16 and fp32), after gemm_ln_exact.py.  Operands: x multiples of 1/8, row m =
   offset_m + spread_m * {-2 .. 2} with offset a multiple of 1/8 in [-2, 2] and spread in {1/4, 1/2, 1, 2} (row sums exact in fp32 in
   any order, asserted; rows m and m + 1 differ; five levels, not seven: their standard deviation is sqrt(2) spread, not 2 spread, which
   in a wide row puts rstd within 1e-5 of a power of two and every d gamma + beta, a dyadic number, on an fp16 tie); gamma non-zero multiples of 1/16 in [-4, 4]; beta multiples of 1/16 in [-2, 2];
   neighbouring columns distinct in both.  In every case: CONSTANT rows (variance exactly 0, the deviations are exactly 0: the output must be
   beta bit for bit) and LOW-VARIANCE rows (offset + {0, 1/8}: variance about 2^-8, where epsilon is 0.3 % of the denominator).  A
   one-row case runs three times, its row ordinary, constant and low-variance (ln_row0s).  The reference is the formula in fp64,

       mean = sum / D     d = x - mean     var = sum d^2 / D     rstd = 1 / sqrt(var + 1e-5)     y = d rstd gamma     out = y + beta

   and the budget follows the kernel's operation sequence (no contraction: the build sets -ffp-contract=off):

       mean^ = fl(sum / D)                    rel. u (the sum is exact)
       d^    = fl(x - mean^)                  |d^ - d| <= u (|mean| + |d|): a shift common to the row, and one rounding
       q^    = sum fl(d^ d^)                  a lane adds its 4 MAXIT squares in turn, six butterfly steps add the lanes: every path
                                              holds one product and at most k - 1 additions, k = 4 MAXIT + 6 = 22 (D <= 1024) or 38;
                                              the common shift cancels in sum d (= 0 exactly) and is left as u^2 mean^2
       v^    = fl(fl(q^ / D) + fl(1e-5))      rel. dv = (k + 4) u + u^2 kappa,  kappa = mean^2 / (var + 1e-5)
       rstd^ = rsqrtf(v^)                     rel. rho = (1 - dv)^(-1/2) (1 + 2u) - 1: rsqrtf budgeted as good to an ulp, 2u -- as
                                              gemm_ln_exact.py budgets its reciprocal square root; the ROCm tree here carries no
                                              document that states a bound for it
       out^  = fl(fl(fl(d^ rstd^) gamma) + beta)

       B = (1 + 2^-10) [ |y| (rho + 3u) + u |mean| rstd |gamma| + u |out| ]          E = 2 B

   ((1 + 2^-10): second-order terms).  E is never tuned against the device.  Two honest fp32 evaluations are asserted to stay below
   E / 2 on every element of every case (ln_emulate): the kernel's order with a correctly rounded reciprocal square root, and torch's
   own summation order with 1 / sqrt.  fp16 output: lo = h(out - E), hi = h(out + E) (h64: one rounding); a decided element (lo == hi) must
   match bit for bit, an undecided one lies in [lo, hi]; at most 5 % of the elements on ordinary (non-constant) rows may be undecided,
   asserted for every case.  fp32 output: |got - out| <= E on every element; constant rows equal beta bit for bit in both types.

Measured (test_rowops_exact_cpu.py and test_hip_rowops_exact.py print them).  LayerNorm, per D and type, for rows = 1 / 5 / 301:
undecided share of the ordinary rows; worst err / E of the two CPU evaluations (kernel order, torch order); MI355X: the worst error
over E that the device's output shows (fp16: observed(), what can be seen behind the output's rounding; fp32: |got - out| / E), over the
four launch modes (out of place, in place, in_stride = D + 4, in_stride = 2 D):
    D     type   undecided (rows 1 / 5 / 301)   err / E kernel order      err / E torch order       MI355X
    4     f16    0.00% / 0.00% / 0.84%        0.029 / 0.051 / 0.075   0.029 / 0.051 / 0.068   0.000 / 0.000 / 0.012
    64    f16    3.12% / 1.17% / 1.44%        0.115 / 0.228 / 0.409   0.115 / 0.228 / 0.409   0.000 / 0.000 / 0.020
    128   f16    1.56% / 0.59% / 1.48%        0.112 / 0.174 / 0.440   0.112 / 0.174 / 0.440   0.000 / 0.000 / 0.032
    252   f16    1.98% / 1.19% / 1.38%        0.160 / 0.358 / 0.472   0.160 / 0.358 / 0.472   0.000 / 0.010 / 0.141
    256   f16    2.54% / 1.56% / 1.40%        0.157 / 0.296 / 0.440   0.157 / 0.296 / 0.440   0.000 / 0.000 / 0.079
    260   f16    1.92% / 1.63% / 1.39%        0.206 / 0.220 / 0.436   0.206 / 0.220 / 0.436   0.000 / 0.013 / 0.358
    768   f16    2.47% / 1.30% / 1.38%        0.339 / 0.336 / 0.484   0.339 / 0.336 / 0.484   0.154 / 0.065 / 0.222
    1024  f16    2.78% / 2.10% / 1.38%        0.283 / 0.412 / 0.461   0.283 / 0.412 / 0.461   0.000 / 0.000 / 0.085
    1028  f16    2.97% / 1.97% / 1.81%        0.136 / 0.367 / 0.450   0.136 / 0.367 / 0.450   0.000 / 0.035 / 0.348
    2048  f16    1.88% / 2.11% / 1.78%        0.288 / 0.381 / 0.475   0.288 / 0.381 / 0.475   0.027 / 0.059 / 0.103
    4     f32            (as fp16)            0.029 / 0.051 / 0.075   0.029 / 0.051 / 0.068   0.029 / 0.051 / 0.065
    64    f32            (as fp16)            0.115 / 0.228 / 0.409   0.115 / 0.228 / 0.409   0.115 / 0.228 / 0.409
    128   f32            (as fp16)            0.112 / 0.174 / 0.440   0.112 / 0.174 / 0.440   0.112 / 0.174 / 0.440
    252   f32            (as fp16)            0.160 / 0.358 / 0.472   0.160 / 0.358 / 0.472   0.160 / 0.358 / 0.472
    256   f32            (as fp16)            0.157 / 0.296 / 0.440   0.157 / 0.296 / 0.440   0.157 / 0.296 / 0.440
    260   f32            (as fp16)            0.206 / 0.220 / 0.436   0.206 / 0.220 / 0.436   0.206 / 0.220 / 0.436
    768   f32            (as fp16)            0.339 / 0.336 / 0.484   0.339 / 0.336 / 0.484   0.339 / 0.336 / 0.484
    1024  f32            (as fp16)            0.283 / 0.412 / 0.461   0.283 / 0.412 / 0.461   0.283 / 0.412 / 0.461
    1028  f32            (as fp16)            0.136 / 0.367 / 0.450   0.136 / 0.367 / 0.450   0.136 / 0.367 / 0.450
    2048  f32            (as fp16)            0.288 / 0.381 / 0.475   0.288 / 0.381 / 0.475   0.288 / 0.381 / 0.475
(fp32: the device's worst element shows the same figure as the kernel-order evaluation.  The figures near 0.5 are elements with d close to 0,
where the rounding of the last addition, up to u |out|, is nearly all of B.)
L2 norm, model-like set: share of the rows of a case (rows = 131) with two different candidate rows after one or two applications, by D:
    4: 0.00%   64: 0.76%   128: 0.76%   252: 2.29%   256: 4.58%   260: 3.05%   512: 7.63%   768: 9.16%   1024: 12.98%
"""
import functools
from typing import NamedTuple

import numpy as np
import torch

import gemm_exact as G
import gemm_ln_exact as L
from gemm_ln_exact import U, h64

EPS = 1e-5
MAX_UNDECIDED = 0.05
GUARD = 8                               # guard rows in front of and behind every output


def h32(y):
    """fp64 -> fp32 -> fp16: the kernels' two roundings of an exact sum, product, quotient or square root (module docstring, 1.)."""
    return y.float().half()


def sqrt32(t):
    """fp32 square root, correctly rounded (numpy's; torch's vectorised fp32 sqrt on the CPU is not, test_rowops_exact_cpu.py shows it)."""
    return torch.from_numpy(np.sqrt(t.contiguous().numpy()))


def guarded(rows, cols, dtype=torch.float16, device="cpu"):
    """(buffer [GUARD + rows + GUARD, cols] filled with the sentinel, its middle `rows` rows as a view)."""
    buf = G.sentinel_buffer(rows + 2 * GUARD, cols, dtype, device)
    return buf, buf[GUARD:GUARD + rows]


def guards_untouched(buf, rows):
    s = G.SENTINEL32 if buf.dtype == torch.float32 else G.SENTINEL
    b = G.bits(buf)
    for name, part, first in (("in front of the first", b[:GUARD], 0), ("behind the last", b[GUARD + rows:], GUARD + rows)):
        if not bool((part == s).all()):
            r, c = (int(i) for i in (part != s).nonzero()[0])
            return f"wrote {name} row: guard element ({first + r - GUARD}, {c}) relative to the output"
    return None


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------

LN_ROWS = (1, 5, 301)                   # 301: the last block has one live wave
LN_D = (4, 64, 128, 252, 256, 260, 768, 1024, 1028, 2048)
LN_MODES = ("out_of_place", "in_place", "stride_d+4", "stride_2d")


class LnCase(NamedTuple):
    rows: int
    D: int
    f32: bool

    @property
    def id(self):
        return f"ln-{self.rows}x{self.D}-{'f32' if self.f32 else 'f16'}"


LN_CASES = [LnCase(r, d, f) for f in (False, True) for d in LN_D for r in LN_ROWS]


def ln_maxit(D):
    return 4 if D <= 1024 else 8        # launch_layernorm's choice of instantiation


def ln_row0s(rows):
    """The kinds row 0 takes, one launch each: a one-row case cannot hold the three kinds at once."""
    return ("ordinary", "constant", "lowvar") if rows == 1 else ("ordinary",)


def ln_kinds(rows, row0="ordinary"):
    kinds = {} if row0 == "ordinary" else {0: row0}
    if rows >= 5:
        kinds.update({1: "constant", 3: "lowvar"})
    if rows >= 301:
        kinds.update({70: "lowvar", 141: "constant", rows - 2: "lowvar", rows - 1: "constant"})
    return kinds


class LnOperands(NamedTuple):
    x: torch.Tensor             # [rows, D] fp16 or fp32
    g: torch.Tensor             # fp32 [D]
    b: torch.Tensor             # fp32 [D]
    const: torch.Tensor         # bool [rows]: constant rows


def ln_columns(D, seed):
    gen = torch.Generator().manual_seed(seed)
    k = torch.randint(1, 128, (D,), generator=gen).cumsum(0) % 128
    g = (k - 64 + (k >= 64).long()).float() / 16                          # -4 .. -1/16, 1/16 .. 4
    kb = torch.randint(1, 65, (D,), generator=gen).cumsum(0) % 65
    b = (kb - 32).float() / 16                                            # -2 .. 2, zero among them
    assert bool((g != 0).all()) and float(g.abs().max()) <= 4 and float(b.abs().max()) <= 2
    assert bool((g[1:] != g[:-1]).all()) and bool((b[1:] != b[:-1]).all())
    return g, b


@functools.lru_cache(maxsize=8)
def ln_operands(c, row0="ordinary"):
    rows, D = c.rows, c.D
    gen = torch.Generator().manual_seed(rows * 7919 + D * 31 + 3)
    m = torch.arange(rows)
    offset = ((m * 5) % 33 - 16).double() / 8
    spread = torch.tensor([0.25, 0.5, 1.0, 2.0], dtype=torch.float64)[(m // 2 + m // 7) % 4]
    r = torch.randint(-2, 3, (rows, D), generator=gen).double()
    r[:, 0], r[:, 1] = (-2 + m % 2).double(), (2 - m % 2).double()        # no row is constant by chance
    x = offset[:, None] + spread[:, None] * r
    const = torch.zeros(rows, dtype=torch.bool)
    for row, kind in ln_kinds(rows, row0).items():
        low = ((row * 3) % 9 - 4) / 8
        if kind == "constant":
            x[row] = offset[row]
            const[row] = True
        else:
            bern = torch.randint(0, 2, (D,), generator=gen).double()
            bern[0], bern[1] = 0.0, 1.0
            x[row] = low + bern / 8
    assert torch.equal(x.half().double(), x) and torch.equal(x * 8, (x * 8).round()), "x is not a multiple of 1/8 within fp16"
    L.assert_sums_exact(x, c.id + ": row sums")
    if rows > 1:
        assert bool((x[1:] != x[:-1]).any(1).all()), "neighbouring rows are equal"
    assert bool(((x == x[:, :1]).all(1) == const).all())
    g, b = ln_columns(D, D * 17 + 1)
    return LnOperands(x.float() if c.f32 else x.half(), g, b, const)


class LnReference(NamedTuple):
    x: torch.Tensor             # fp64 [rows, D]: the formula
    E: torch.Tensor             # fp64: the budget
    lo: torch.Tensor            # fp16 h(x - E)
    hi: torch.Tensor            # fp16 h(x + E)
    const: torch.Tensor         # bool [rows]
    beta: torch.Tensor          # fp32 [D]

    def to(self, device):
        return LnReference(*(t.to(device) for t in self))


def ln_reference(ops):
    x = ops.x.double()
    D = x.shape[1]
    g, b = ops.g.double()[None], ops.b.double()[None]
    mean = x.sum(1, keepdim=True) / D
    d = x - mean
    var = (d * d).sum(1, keepdim=True) / D
    v = var + EPS
    rstd = 1 / v.sqrt()
    y = d * rstd * g
    out = y + b
    k = 4 * ln_maxit(D) + 6
    kappa = mean * mean / v
    dv = (k + 4) * U + U * U * kappa
    assert float(dv.max()) < 2.0 ** -10
    rho = (1 - dv) ** -0.5 * (1 + 2 * U) - 1
    B = (1 + 2.0 ** -10) * (y.abs() * (rho + 3 * U) + U * mean.abs() * rstd * g.abs() + U * out.abs())
    E = 2 * B
    assert bool(torch.isfinite(out).all()) and float((out.abs() + E).max()) < 60000
    return LnReference(out, E, h64(out - E), h64(out + E), ops.const, ops.b)


def ln_undecided_share(ref):
    und = G.bits(ref.lo) != G.bits(ref.hi)
    return float(und[~ref.const].float().mean()) if bool((~ref.const).any()) else 0.0


def ln_mismatch(got, ref):
    """None if `got` ([rows, D] fp16 or fp32) passes: constant rows equal beta bit for bit; fp16: decided elements bit-equal, undecided
    ones within [lo, hi]; fp32: |got - x| <= E.  Else how many elements fail, how many of them decided, and the first."""
    assert got.shape == ref.x.shape, f"{tuple(got.shape)} against {tuple(ref.x.shape)}"
    gf = got.double()
    decided = G.bits(ref.lo) == G.bits(ref.hi)
    if got.dtype == torch.float16:
        ordinary = torch.where(decided, G.bits(got) == G.bits(ref.lo), (gf >= ref.lo.double()) & (gf <= ref.hi.double()))
    else:
        ordinary = (gf - ref.x).abs() <= ref.E
        decided = torch.ones_like(decided)
    beta = ref.beta.to(got.dtype)[None].expand_as(got)
    ok = torch.where(ref.const[:, None], G.bits(got) == G.bits(beta.contiguous()), ordinary)
    if bool(ok.all()):
        return None
    bad = ~ok
    r, c = (int(i) for i in bad.nonzero()[0])
    state = "a constant row: beta bit for bit" if bool(ref.const[r]) else "decided" if bool(decided[r, c]) else "undecided: within [lo, hi]"
    return (f"{int(bad.sum())} of {bad.numel()} elements fail ({int((bad & decided).sum())} of them decided), in rows {int(bad.any(1).nonzero()[0])}.."
            f"{int(bad.any(1).nonzero()[-1])}; first at ({r}, {c}) = lane {(c // 4) % 64}, step {c // 256}: got {float(got[r, c])!r}, want "
            f"{float(ref.x[r, c]):.9g} (lo {float(ref.lo[r, c])}, hi {float(ref.hi[r, c])}, E {float(ref.E[r, c]):.3e}, beta {float(ref.beta[c])}); {state}")


def over_E(err, E):
    """err / E per element, 0 where both are 0 (d = 0, beta = 0 and mean = 0: the element is exactly 0 and E is 0)."""
    return torch.where(err == 0, torch.zeros_like(err), err / E)


def ln_observed(got, ref):
    """The worst error over E the output shows on ordinary rows: fp32 |got - x| / E; fp16 gemm_ln_exact.observed."""
    keep = ~ref.const
    if not bool(keep.any()):
        return 0.0
    if got.dtype == torch.float32:
        return float(over_E((got.double() - ref.x).abs(), ref.E)[keep].max())
    return float(torch.nan_to_num(L.observed(got, ref), nan=0.0)[keep].max())


LN_DEFECTS = ("eps_1e-6", "var_over_d-1", "g_col+1", "b_col+1", "row+1", "stats_drop_last4")


def _lane_sum(t, maxit):
    """[rows, maxit * 256] fp32 -> [rows]: the kernel's order -- lane l adds columns (64 it + l) * 4 + k in turn, then the butterfly."""
    rows = t.shape[0]
    v = t.view(rows, maxit, 64, 4)
    s = torch.zeros((rows, 64), dtype=torch.float32)
    for it in range(maxit):
        for k in range(4):
            s = s + v[:, it, :, k]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def ln_emulate(ops, order="kernel", defect=None):
    """An honest fp32 evaluation of the formula, every operation rounded, as fp32 [rows, D] in front of the output conversion.  order
    "kernel": the kernel's summation order and a correctly rounded reciprocal square root; "torch": torch's own order and 1 / sqrt.
    defect: one of LN_DEFECTS."""
    f = torch.float32
    x = ops.x.float()
    rows, D = x.shape
    g, b = ops.g, ops.b
    if defect == "row+1":
        x = x.roll(-1, 0)
    if defect == "g_col+1":
        g = g.roll(-1)
    if defect == "b_col+1":
        b = b.roll(-1)
    n_stat = D - 4 if defect == "stats_drop_last4" else D
    live = (torch.arange(D) < n_stat).to(f)[None]
    maxit = ln_maxit(D)

    def total(t):
        if order == "kernel":
            pad = torch.zeros((rows, maxit * 256), dtype=f)
            pad[:, :D] = t
            return _lane_sum(pad, maxit)
        return t.sum(1)
    mean = total(x * live) / torch.tensor(float(D), dtype=f)
    d = x - mean[:, None]
    q = total(d * d * live) / torch.tensor(float(D - 1 if defect == "var_over_d-1" else D), dtype=f)
    v = q + torch.tensor(1e-6 if defect == "eps_1e-6" else 1e-5, dtype=f)
    rstd = (1 / v.double().sqrt()).float() if order == "kernel" else 1.0 / sqrt32(v)
    return d * rstd[:, None] * g[None] + b[None]


# ---- L2 norm -----------------------------------------------------------------------------------------------------------------------

L2_ROWS = (1, 4, 5, 131)
L2_D = (4, 64, 128, 252, 256, 260, 512, 768, 1024)
L2_SETS = ("exact", "model")


def l2_row0s(rows):
    return ("ordinary", "zero", "overflow") if rows == 1 else ("ordinary",)


def l2_pins(rows, row0="ordinary"):
    pins = {} if row0 == "ordinary" else {0: row0}
    if rows >= 4:
        pins.update({1: "zero", 2: "overflow"})
    if rows >= 131:
        pins.update({rows - 2: "zero", rows - 1: "overflow"})
    return pins


def exact_rows(shape, gen):
    """fp16 multiples of 1/16 in [-2, 2]: the sum of squares of a row is a multiple of 2^-8 below 2^13, exact in fp32 in any order."""
    x = torch.randint(-32, 33, shape, generator=gen).double() / 16
    assert float((x * x).sum(-1).max()) < 2.0 ** 13 and torch.equal(x.half().double(), x)
    return x.half()


def is_exact_set(X):
    x = X.double()
    return bool((x.abs() <= 2).all()) and torch.equal(x * 16, (x * 16).round()) and X.shape[-1] <= 2048


@functools.lru_cache(maxsize=8)
def l2_operands(rows, D, kind, row0="ordinary"):
    gen = torch.Generator().manual_seed(rows * 131 + D * 7 + len(kind))
    if kind == "exact":
        X = exact_rows((rows, D), gen)
    else:
        scale = torch.tensor([0.02, 0.3, 1.0, 7.0, 40.0])[torch.arange(rows) % 5]
        X = (torch.randn((rows, D), generator=gen) * scale[:, None]).half()
    pinned = torch.zeros(rows, dtype=torch.bool)
    for row, pin in l2_pins(rows, row0).items():
        sign = (torch.randint(0, 2, (D,), generator=gen) * 2 - 1).half()
        X[row] = 0.0 if pin == "zero" else 40000.0 * sign
        pinned[row] = True
    return X, pinned


def _next_f16(n):
    """The fp16 value above a non-negative fp16 value (inf stays inf)."""
    b = G.bits(n).int()
    return torch.where(b >= 0x7c00, b, b + 1).to(torch.int16).view(torch.float16)


def l2_apply(X, exact=False):
    """One application of the kernel to the fp16 rows X [R, D]: the two candidate results, fp16 [R, D] each, bit-equal wherever the norm
    is decided (module docstring, 2.).  exact: True, or a bool mask of the rows for which the caller states that the sum of squares is
    exact in fp32 (checked: is_exact_set) -- their gamma is 0 and their two candidates are one.  Asserts that no row has more than two
    candidate norms."""
    x = X.double()
    R_, D = x.shape
    mask = exact if isinstance(exact, torch.Tensor) else torch.full((R_,), bool(exact))
    assert is_exact_set(X[mask])
    ss = (x * x).sum(1)                                                   # fp64: 22-bit squares, at most 2^-42 off
    gamma = torch.where(mask, torch.zeros((), dtype=torch.float64), torch.tensor((D - 1) * U / (1 - (D - 1) * U) + 2.0 ** -40, dtype=torch.float64))
    n_lo, n_hi = h32((ss * (1 - gamma)).sqrt()), h32((ss * (1 + gamma)).sqrt())
    assert bool(((G.bits(n_hi) == G.bits(n_lo)) | (G.bits(n_hi) == G.bits(_next_f16(n_lo)))).all()), "more than two candidate fp16 norms"
    assert torch.equal(G.bits(n_lo[mask]), G.bits(n_hi[mask]))
    out = []
    for n in (n_lo, n_hi):
        nd = n.double()
        nd = torch.where(nd == 0, torch.full_like(nd, float(torch.tensor(1e-12, dtype=torch.float32))), nd)      # fmaxf(n, 1e-12f)
        out.append(h32(x / nd[:, None]))
    return out


def l2_candidates(X, times, exact=False):
    """The candidate results of `times` applications: 2^times tensors (equal where the norms are decided).  exact: as in l2_apply,
    for the FIRST application; what a later one sees is arbitrary fp16."""
    cands = l2_apply(X, exact)
    for _ in range(times - 1):
        cands = [o for cnd in cands for o in l2_apply(cnd)]
    return cands


def two_norm_share(cands):
    """Share of the rows whose candidates differ."""
    differ = torch.zeros(cands[0].shape[0], dtype=torch.bool)
    for cnd in cands[1:]:
        differ |= (G.bits(cnd) != G.bits(cands[0])).any(1)
    return float(differ.float().mean())


def rows_mismatch(got, cands, what="candidate"):
    """None if every row of `got` is bit-equal, as a whole row, to the same row of one of `cands`; else which rows are not, and for the
    first of them how many elements differ from its nearest candidate and the first such element."""
    assert all(got.shape == cnd.shape and got.dtype == cnd.dtype for cnd in cands), f"{tuple(got.shape)} {got.dtype}"
    gb = G.bits(got)
    diff = torch.stack([(gb != G.bits(cnd)).sum(1) for cnd in cands])     # [n_cand, rows]
    best, which = diff.min(0)
    if not bool(best.any()):
        return None
    bad = best.nonzero().flatten()
    r = int(bad[0])
    want = cands[int(which[r])]
    c = int((gb[r] != G.bits(want)[r]).nonzero()[0])
    n_c = len({tuple(G.bits(cnd)[r].tolist()) for cnd in cands})
    return (f"{bad.numel()} of {got.shape[0]} rows equal no {what} row, rows {r}..{int(bad[-1])}; row {r} differs from the nearest of its {n_c} "
            f"in {int(best[r])} of {got.shape[1]} elements, first at column {c} (lane {(c // 4) % 64}): got {float(got[r, c])!r} "
            f"(0x{int(gb[r, c]) & 0xffff:04x}), want {float(want[r, c])!r} (0x{int(G.bits(want)[r, c]) & 0xffff:04x})")


def l2_emulate(X, times=1, defect=None):
    """An honest fp32 evaluation in torch's own summation order.  defect "norm_not_rounded": the norm kept in fp32."""
    x = X
    for _ in range(times):
        xf = x.float()
        n = sqrt32((xf * xf).sum(1))
        if defect != "norm_not_rounded":
            n = n.half().float()
        x = (xf / n.clamp_min(1e-12)[:, None]).half()
    return x


# ---- prompt ensemble ---------------------------------------------------------------------------------------------------------------

ENS_T = (1, 2, 7, 13)
ENS_ROWS = (1, 5, 131)
ENS_E_V8 = (8, 64, 128, 512, 520, 768, 1024)      # 16-byte paths: v8<1> up to 512, v8<2> up to 1024
ENS_E_ANY = (1, 36, 100, 1100)                    # E % 8 != 0 or E > 1024: the element-wise kernel


@functools.lru_cache(maxsize=4)
def ens_operands(T, rows, E):
    gen = torch.Generator().manual_seed(T * 1009 + rows * 13 + E)
    feats = exact_rows((T, rows, E), gen)
    if T >= 2:
        feats[T - 1, rows - 1] = 0.0                                      # one template's row all zero: u_t = 0 through the clamp
    return feats


def ens_reference(feats, defect=None):
    """feats [T, rows, E] fp16 from the exact set -> (the candidate output rows, m): n_t, u_t, acc and m have ONE bit pattern
    (text_ensemble.hip lists the rounding points), the last norm the two-candidate rule.  defect "mean_div": m = h(acc / T), a
    mean taken in fp16 steps, h(acc * h(1 / T)), for h(acc * fl(1 / T)).  (The quotient itself, h(acc / T), is no defect: an 11-bit acc over
    T <= 13 never comes within 2^-24 of an fp16 tie, so it equals h(acc * fl(1 / T)) -- "mean_quotient", asserted equal on the CPU.)"""
    T = feats.shape[0]
    acc = None
    for t in range(T):
        u = l2_apply(feats[t], exact=True)[0]
        acc = u if acc is None else h32(acc.double() + u.double())
    inv_T = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(T), dtype=torch.float32)
    m = _mean(acc, T, inv_T, defect)
    return l2_apply(m), m


def _mean(acc, T, inv_T, defect):
    if defect == "mean_div":
        return h32(acc.double() * inv_T.half().double())
    if defect == "mean_quotient":
        return h64(acc.double() / T)
    return h32(acc.double() * inv_T.double())


def ens_emulate(feats, defect=None):
    """The same sequence in fp32 torch arithmetic, torch's own summation order."""
    T = feats.shape[0]
    acc = None
    for t in range(T):
        u = l2_emulate(feats[t])
        acc = u if acc is None else (acc.float() + u.float()).half()
    inv_T = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(T), dtype=torch.float32)
    m = _mean(acc, T, inv_T, defect) if defect else (acc.float() * inv_T).half()
    return l2_emulate(m)


# ---- text front --------------------------------------------------------------------------------------------------------------------

VOCAB = 512
LCTX = 77
TEXT_N = (1, 5)
TEXT_LSEQ = (1, 9, 77)
TEXT_D = (64, 128, 768)
TEXT_STRIDES = (77, 80)
PAD_ID = 10 ** 6                        # behind column LCTX of an ids row: wins the argmax if it is read


def _grid(rows, D):
    return torch.arange(rows, dtype=torch.int64)[:, None], torch.arange(D, dtype=torch.int64)[None]


@functools.lru_cache(maxsize=4)
def tok_table(D, vocab=VOCAB):
    """fp32 [vocab, D]: ((131 v + 7 c) mod 2039 - 1019) / 256 + ((5 v + 3 c) mod 15 - 7) 2^-13 -- a wrong row or column shows in nearly
    every element (2039 is prime), and five values in six are no fp16 values: h(tok) rounds, and leaves eighths of the sum's fp16 step behind."""
    v, c = _grid(vocab, D)
    t = ((v * 131 + c * 7) % 2039 - 1019).double() / 256 + ((v * 5 + c * 3) % 15 - 7).double() * 2.0 ** -13
    assert torch.equal(t.float().double(), t)
    return t.float()


@functools.lru_cache(maxsize=4)
def pos_table(D, rows=LCTX + 1):
    """fp16 [rows, D]: ((89 l + 3 c) mod 1021 - 510) / 128; one row more than the context, for the planted "row l + 1"."""
    l, c = _grid(rows, D)
    t = ((l * 89 + c * 3) % 1021 - 510).double() / 128
    assert torch.equal(t.half().double(), t)
    return t.half()


@functools.lru_cache(maxsize=4)
def prompt_table(N, D, Lctx=LCTX):
    """fp16 [N, Lctx, D]: h(((131 (n Lctx + l) + 7 c) mod 2039 - 1019) / 256)."""
    r, c = _grid(N * Lctx, D)
    return (((r * 131 + c * 7) % 2039 - 1019).double() / 256).half().view(N, Lctx, D)


_MAXIMA = ((7, 30), (76, 76), (0, 50), (3, 4), (40, 41))


@functools.lru_cache(maxsize=4)
def ids_table(N, stride, vocab=VOCAB):
    """int64 [N, stride]: ids below vocab - 1, the maximum vocab - 1 at the two columns of _MAXIMA (row 1: the last column alone, row
    2: column 0 first); behind column LCTX, PAD_ID."""
    gen = torch.Generator().manual_seed(N * 5 + stride)
    ids = torch.randint(0, vocab - 1, (N, stride), generator=gen)
    for n in range(N):
        for p in _MAXIMA[n % len(_MAXIMA)]:
            ids[n, p] = vocab - 1
    ids[:, LCTX:] = PAD_ID
    return ids


TEXT_DEFECTS = ("pos_row+1", "sum_before_rounding", "double_rounding")


def _round12(y):
    """fp64 -> 12 significant bits, to nearest (Veltkamp): the intermediate of a planted double rounding."""
    c = y * (2.0 ** 41 + 1)
    return c - (c - y)


def embed_ids_reference(ids, tok, pos, Lseq, defect=None):
    """(x fp16 [N * Lseq, D] = h(h(tok[ids]) + pos[l]), index int32 [N] = the first maximum of ids[n, :LCTX]).  defect: one of
    TEXT_DEFECTS (the position row l + 1; the embedding added before it is rounded to fp16; the sum rounded to 12 bits first)."""
    N, D = ids.shape[0], tok.shape[1]
    e = tok[ids[:, :Lseq]]
    p = pos[1:Lseq + 1] if defect == "pos_row+1" else pos[:Lseq]
    e = e.double() if defect == "sum_before_rounding" else e.half().double()
    s = e + p.double()[None]
    x = _round12(s).half() if defect == "double_rounding" else h32(s)
    return x.reshape(N * Lseq, D), torch.argmax(ids[:, :LCTX], dim=1).to(torch.int32)


def add_pos_reference(prompts, pos, Lseq, defect=None):
    N, _, D = prompts.shape
    p = pos[1:Lseq + 1] if defect == "pos_row+1" else pos[:Lseq]
    return h32(prompts[:, :Lseq].double() + p.double()[None]).reshape(N * Lseq, D)


def gather_reference(x, index, Lseq):
    """x fp16 [N * Lseq, D], index int32 [N] (any value: clamped to [0, Lseq)) -> [N, D]."""
    N = index.numel()
    return x.view(N, Lseq, -1)[torch.arange(N), index.long().clamp(0, Lseq - 1)]


def gather_indices(N, Lseq):
    """int32 [N]: inside, on both edges, and outside [0, Lseq) on both sides."""
    vals = [Lseq - 1, -3, Lseq, 0, 2 ** 31 - 1, -2 ** 31, Lseq + 5]
    return torch.tensor([vals[n % len(vals)] for n in range(N)], dtype=torch.int32)


def embed_tokens_reference(ids, tok):
    return tok[ids].half()


def assemble_reference(base, labels, tokens, n_ctx):
    """base fp16 [*, Lctx, D], labels int64 [Cb] or None (row 0), tokens fp32 [Cb, n_ctx, D] -> fp16 [Cb, Lctx, D]."""
    Cb = tokens.shape[0]
    rows = base[labels] if labels is not None else base[:1].expand(Cb, -1, -1)
    return torch.cat([rows[:, :2], tokens.half(), rows[:, 2:rows.shape[1] - n_ctx]], dim=1)
