"""CPU companion of test_hip_gemm_ln_exact.py (gemm_ln_exact.py: the method and the derivation of the budget E).  Pure torch: no library,
no GPU.  For every case of gemm_ln_exact.CASES:

  * the exactness promises hold (products, slot sums, folded operands: asserted while the operands are built), rows 1, 8, 16, 64, 128
    apart and neighbouring columns differ, the degenerate rows are what they are said to be, the reference stays inside fp16;
  * at most 5 % of the elements on ordinary rows are undecided;
  * the case takes the branch it is listed for under every variant, and the list reaches every instantiation class the tile kernel's
    table holds for the LN epilogues;
  * two honest fp32 evaluations -- the kernel's order with two fused multiply-adds, and rstd * (acc - mean * g) + b with every
    operation rounded -- stay below E / 2 on every element and pass the comparator;
and on the small shapes the comparator REJECTS each planted defect (gemm_ln_exact.DEFECTS).
"""
import numpy as np
import pytest
import torch

import gemm_exact as G
import gemm_ln_exact as L
from conftest import usable_threads

_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(usable_threads())


def _ids(c):
    return c.id


def test_h64_rounds_once():
    """h64 against numpy's direct fp64 -> fp16 conversion: random values over the fp16 range, every kind of tie, and the fp64 values
    next to a tie -- where rounding through fp32 to nearest would round twice and go wrong."""
    gen = torch.Generator().manual_seed(1)
    y = torch.randn(200000, generator=gen, dtype=torch.float64) * torch.logspace(-8, 3.5, 200000, dtype=torch.float64)
    h = torch.arange(0, 0x7bff, dtype=torch.int32).to(torch.int16).view(torch.float16).double()
    ties = (h[1:] + h[:-1]) / 2
    near = torch.cat([ties, torch.nextafter(ties, ties + 1), torch.nextafter(ties, ties - 1), ties * (1 + 2.0 ** -30), ties * (1 - 2.0 ** -30)])
    y = torch.cat([y, near, -near, h, torch.zeros(1, dtype=torch.float64)])
    want = torch.from_numpy(y.numpy().astype(np.float16))
    assert torch.equal(G.bits(L.h64(y)), G.bits(want))
    twice = y.float().half()                                              # the conversion h64 is there to avoid
    assert not torch.equal(G.bits(twice), G.bits(want))


def test_every_case_takes_the_branch_it_is_listed_for():
    for c in L.CASES:
        assert c.want and set(L.PLAIN) <= set(c.want), c.id
        assert (c.epi == G.EPI_LN_BIAS_QGELU) == (set(L.ONE_ROUNDING) <= set(c.want)), c.id
        for v, want in c.want.items():
            got = G.route(v, c.M, c.N, c.K, c.epi)
            assert got == want, f"{c.id}, variant {v}: listed for {want}, the dispatcher takes {got}"
        if c.kind == "stats":                                             # the first GEMM: the tile kernel with the statistics epilogue
            assert all(G.route(v, c.M, c.K, c.K1, G.EPI_BIAS_RES, stats=True)[0] == "v5" for v in c.variants)
    L.assert_coverage()
    assert len(L.REQUIRED) == 18
    for drop in ((8200, 3072), (10800, 3072), (L._PP_M, 2048)):          # without the store-hint shapes, or the g4 shape, the list is short
        with pytest.raises(AssertionError):
            L.assert_coverage([c for c in L.CASES if (c.M, c.N) != drop])
    with pytest.raises(AssertionError):
        L.assert_coverage([c for c in L.CASES if c.epi == G.EPI_LN_BIAS])
    # gemm_exact's own list holds no case of these epilogues
    assert not [c for c in G.CASES if c.epi in (G.EPI_LN_BIAS, G.EPI_LN_BIAS_QGELU)]


@pytest.mark.parametrize("c", [c for c in L.CASES if c.epi == G.EPI_LN_BIAS], ids=_ids)
def test_case_conditions_and_honest_evaluations(c):
    ops = L.operands(c)
    ref, acc = L.expected(c)
    S = c.K // 256
    assert ops.stats.shape == (c.M, S, 2) and ops.g.shape == (c.N,) and ops.b.shape == (c.N,) and acc.shape == (c.M, c.N)
    assert L.gemm_rows(c, ops).shape == (c.M, c.K) and ops.W.shape == (c.N, c.K)
    buf = L.stats_buffer(ops)
    assert bool(torch.isnan(buf[c.M:]).all()) and buf.shape[0] == c.M + G.PAD_ROWS and torch.equal(buf[:c.M], ops.stats)
    # degenerate rows
    var32 = L._kernel_var32(ops.su, ops.sq, c.K)
    stated = ops.sq / c.K - (ops.su / c.K) ** 2
    assert bool((stated[ops.deg] <= 0).all()) and bool((stated[~ops.deg] >= 1 / 16).all())
    assert int(ops.deg.sum()) >= (3 if c.kind != "stats" else 0)
    if c.kind == "epi":
        assert int((stated == 0).sum()) >= 3 and int((stated == -1 / 16).sum()) == 1
        assert bool((var32[stated == -1 / 16] < -1e-5).all())            # without the clamp: NaN
        tiny = (stated < 0) & (stated > -1e-5)                           # K = 768: the fp32 sequence sees the sign, and stays above -1e-5
        assert int(tiny.sum()) == (2 if c.K == 768 else 0) and bool((var32[tiny] < 0).all()) and bool((var32[tiny] > -1e-5).all())
        assert bool((var32[stated == 0] == 0).all())
        if S > 1:
            assert bool((ops.stats[:, 1] == 0).all()) and bool((ops.stats[:, S - 1, 0] < 0).all())
    elif c.kind != "stats":
        assert bool((L.gemm_rows(c, ops)[ops.deg] == L.gemm_rows(c, ops)[ops.deg][:, :1]).all())      # constant rows
    assert float(ref.kappa[ops.deg].min() if bool(ops.deg.any()) else 0.0) >= 0 and bool((ref.lo.double() <= ref.hi.double()).all())
    # the 5 % cap
    share = L.undecided_share(ref)
    assert 0 < share <= L.MAX_UNDECIDED, f"{c.id}: {share:.2%} of the elements are undecided"
    # honest evaluations: below E / 2, and accepted
    rows = L.emulation_rows(c, ops)
    rr = ref.rows(rows)
    worst = {}
    for order in ("fma", "separate"):
        x = L.emulate(c, ops, acc, rows, order)
        ratio = (x.double() - rr.x).abs() / rr.E
        worst[order] = float(ratio.max())
        assert worst[order] < 0.5, f"{c.id}: the {order} evaluation is {worst[order]:.3f} E off"
        msg = L.ln_mismatch(x.half(), rr)
        assert msg is None, f"{c.id}, {order}: {msg}"
        assert max(L.worst_observed(x.half(), rr)) <= worst[order] + 1e-9  # what the output shows never exceeds the fp32 error
    _FIGURES[c.id] = (G.route(8, c.M, c.N, c.K, c.epi), G.route(6, c.M, c.N, c.K, c.epi), share, worst["fma"], worst["separate"])
    print(f"\n{c.id}: undecided {share:.2%}; worst err / E: kernel order {worst['fma']:.3f}, separate roundings {worst['separate']:.3f}")


SMALL = [c for c in L.CASES if c.kind == "epi" and c.epi == G.EPI_LN_BIAS and c.M == 300 and c.N == 192]


# (one slot at K = 256: there is no zero slot to overwrite)
PLANTED = [(c, d) for c in SMALL for d in L.DEFECTS if not (d == "zero_slot_copy" and c.K == 256)]


@pytest.mark.parametrize("c,defect", PLANTED, ids=lambda v: v.id if isinstance(v, L.Case) else v)
def test_comparator_rejects_planted_defects(c, defect):
    ops = L.operands(c)
    ref, acc = L.expected(c)
    rows = torch.arange(c.M)
    good = L.emulate(c, ops, acc, rows).half()
    assert L.ln_mismatch(good, ref) is None
    for order in ("fma", "separate"):
        bad = L.emulate(c, ops, acc, rows, order, defect).half()
        msg = L.ln_mismatch(bad, ref)
        assert msg is not None, f"{c.id}, {order}: {defect} went unnoticed"
        failing = int(msg.split(" of ")[0])
        if defect == "no_clamp":        # NaN on the row whose statistics state variance -1/16; at K = 768 the two rows of variance -1 / K^2 are 9 % off
            assert failing == c.N * (3 if c.K == 768 else 1) and "in rows 70..259" in msg or "in rows 200..200" in msg
            assert not bool(torch.isfinite(bad[200]).any())
        elif defect == "eps_1e-6":                                        # 1e-6 for 1e-5 moves rstd by a few 1e-6: decided elements change
            assert int(msg.split("(")[1].split(" of them decided")[0]) >= 100, msg
        else:
            assert failing >= 0.9 * c.M * c.N, f"{c.id}, {order}, {defect}: {msg}"


def test_the_message_places_the_defect():
    c = SMALL[1]
    ops = L.operands(c)
    ref, acc = L.expected(c)
    good = L.emulate(c, ops, acc, torch.arange(c.M)).half()
    und = (G.bits(ref.lo) != G.bits(ref.hi)) & ~ref.deg[:, None]
    for want_state, pick in (("decided: bit equality", ~und & ~ref.deg[:, None]), ("undecided: within [lo, hi]", und)):
        r, col = (int(i) for i in pick.nonzero()[-1])
        moved = good.clone()
        if und[r, col]:
            moved[r, col] = ref.hi[r, col].float() + 3 * (ref.hi[r, col].float() - ref.lo[r, col].float()) + 0.01
        else:
            G.bits(moved)[r, col] ^= 1
        msg = L.ln_mismatch(moved, ref, L.PRODUCERS["rows"], (ops.su, ops.sq))
        assert msg is not None and msg.startswith(f"1 of {good.numel()} elements") and f"first at ({r}, {col})" in msg and want_state in msg
        assert f"row {r % 256} of its 256-row tile ({r % 64} mod 64), column {col % 256} of its 256-column tile ({col % 64} mod 64)" in msg
        assert "row_stats_kernel" in msg and f"row {r} expects (su, sq) = ({float(ops.su[r])}, {float(ops.sq[r])})" in msg
    # an undecided element may take lo or hi, nothing else; a degenerate row takes E + half a step, not more
    r, col = (int(i) for i in und.nonzero()[0])
    for v in (ref.lo[r, col], ref.hi[r, col]):
        ok = good.clone()
        ok[r, col] = v
        assert L.ln_mismatch(ok, ref) is None
    d = int(ref.deg.nonzero()[0])
    off = good.clone().double()
    off[d] = ref.x[d] + 1.5 * ref.E[d] + 2 * L.half_step(ref.x[d].abs() + ref.E[d])
    assert L.ln_mismatch(off.half(), ref) is not None


def test_report_figures():
    """Prints the table of the module docstring of gemm_ln_exact.py for the cases run in this session."""
    for cid, (r8, r6, share, fma, sep) in _FIGURES.items():
        print(f"\n    {cid:34s} {r8[1]} {r8[2]:8s} | {r6[1]} {r6[2]:8s} {r8[4] or '-':2s}  undecided {share:6.2%}   err / E {fma:.3f} {sep:.3f}")
