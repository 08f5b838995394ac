"""CPU companion of test_hip_rowops_exact.py (rowops_exact.py: the three methods and the derivation of the LayerNorm budget E).  Pure
torch: no library, no GPU.

  * LayerNorm, every case and every kind of first row: the operand promises hold (asserted while they are built), at most 5 % of the
    elements on ordinary rows are undecided, two honest fp32 evaluations -- the kernel's order with a correctly rounded reciprocal
    square root, torch's order with 1 / sqrt -- stay below E / 2 on every element, pass the comparator and give beta bit for bit on
    constant rows; each planted defect (rowops_exact.LN_DEFECTS) is rejected on decided elements;
  * L2 norm and ensemble, every case: no row has more than two candidate norms per application (asserted inside l2_apply), the exact
    set has one, an honest fp32 evaluation in torch's summation order equals a candidate row, the pinned rows are what they are said to
    be; a norm that is not rounded to fp16 and a mean taken in fp16 steps are rejected;
  * text front: the tables tell rows and columns apart, h(tok) rounds in most places, the first maximum wins, the gather clamps; a position
    row l + 1, an embedding added before it is rounded and a sum rounded twice are rejected.
"""
import pytest
import torch

import gemm_exact as G
import rowops_exact as R
from conftest import usable_threads

_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(usable_threads())


def _decided_failures(msg):
    return int(msg.split("(")[1].split(" of them decided")[0])


def test_fp64_operations_rounded_to_fp32_are_the_fp32_operations():
    """53 >= 2 * 24 + 2: division and square root in fp64, rounded to fp32, are the correctly rounded fp32 operations (what h32 relies on)."""
    gen = torch.Generator().manual_seed(2)
    a = torch.randn(200000, generator=gen) * torch.logspace(-6, 6, 200000)
    b = torch.randn(200000, generator=gen).abs() + 2.0 ** -10
    assert torch.equal(G.bits((a.double() / b.double()).float()), G.bits(a / b))
    assert torch.equal(G.bits(a.abs().double().sqrt().float()), G.bits(R.sqrt32(a.abs())))
    print(f"\ntorch's own fp32 sqrt differs from the correctly rounded one in {int((a.abs().sqrt() != R.sqrt32(a.abs())).sum())} of {a.numel()} values")
    h = torch.randn(200000, generator=gen).half()
    k = torch.randn(200000, generator=gen).half()
    assert torch.equal(G.bits(R.h32(h.double() + k.double())), G.bits((h.float() + k.float()).half()))


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.LN_CASES, ids=lambda c: c.id)
def test_ln_case_conditions_and_honest_evaluations(c):
    und_n = und_d = 0
    worst = {"kernel": 0.0, "torch": 0.0}
    for row0 in R.ln_row0s(c.rows):
        ops = R.ln_operands(c, row0)
        ref = R.ln_reference(ops)
        assert ops.x.dtype == (torch.float32 if c.f32 else torch.float16) and ops.x.shape == (c.rows, c.D)
        kinds = R.ln_kinds(c.rows, row0)
        assert int(ops.const.sum()) == sum(k == "constant" for k in kinds.values())
        if c.rows > 1:
            assert "constant" in kinds.values() and "lowvar" in kinds.values()
        xd = ops.x.double()
        var = xd.var(1, unbiased=False)
        for row, kind in kinds.items():
            if kind == "lowvar":                                          # epsilon is a visible share of the denominator
                assert 2.0 ** -10 < float(var[row]) <= 2.0 ** -8, f"{c.id}: row {row} has variance {float(var[row])}"
        assert bool((ref.lo.double() <= ref.hi.double()).all())
        ordinary = ~ops.const
        if bool(ordinary.any()):
            und = (G.bits(ref.lo) != G.bits(ref.hi))[ordinary]
            und_n, und_d = und_n + int(und.sum()), und_d + und.numel()
            assert R.ln_undecided_share(ref) <= R.MAX_UNDECIDED, f"{c.id}, row 0 {row0}: {R.ln_undecided_share(ref):.2%} of the elements are undecided"
        for order in ("kernel", "torch"):
            x = R.ln_emulate(ops, order)
            if bool(ordinary.any()):
                ratio = float(R.over_E((x.double() - ref.x).abs(), ref.E)[ordinary].max())
                worst[order] = max(worst[order], ratio)
                assert ratio < 0.5, f"{c.id}, row 0 {row0}: the {order} evaluation is {ratio:.3f} E off"
            assert torch.equal(G.bits(x[ops.const]), G.bits(ops.b[None].expand(int(ops.const.sum()), -1).contiguous()))
            got = x if c.f32 else x.half()
            msg = R.ln_mismatch(got, ref)
            assert msg is None, f"{c.id}, row 0 {row0}, {order}: {msg}"
            assert R.ln_observed(got, ref) <= worst[order] + 1e-9
    share = und_n / max(und_d, 1)
    assert share <= R.MAX_UNDECIDED
    _FIGURES[c.id] = (share, worst["kernel"], worst["torch"])
    print(f"\n{c.id}: undecided {share:.2%}; worst err / E: kernel order {worst['kernel']:.3f}, torch order {worst['torch']:.3f}")


LN_PLANTED = [R.LnCase(rows, D, f32) for f32 in (False, True) for rows, D in ((5, 4), (5, 260), (301, 768), (301, 1028))]


@pytest.mark.parametrize("defect", R.LN_DEFECTS)
@pytest.mark.parametrize("c", LN_PLANTED, ids=lambda c: c.id)
def test_ln_comparator_rejects_planted_defects(c, defect):
    ops = R.ln_operands(c)
    ref = R.ln_reference(ops)
    for order in ("kernel", "torch"):
        bad = R.ln_emulate(ops, order, defect)
        msg = R.ln_mismatch(bad if c.f32 else bad.half(), ref)
        assert msg is not None, f"{c.id}, {order}: {defect} went unnoticed"
        decided = _decided_failures(msg)
        print(f"\n{c.id}, {order}, {defect}: {msg.split(';')[0]}")
        if c.rows == 301 and defect in ("eps_1e-6", "var_over_d-1"):      # the two a tolerance of 2e-3 lets through
            assert decided >= 1000, msg
        elif defect in ("eps_1e-6", "var_over_d-1"):
            assert decided >= 1, msg
        else:
            ordinary = int((~ops.const).sum()) * c.D
            assert decided >= 0.5 * ordinary, msg


def test_ln_comparator_places_a_defect():
    c = R.LnCase(5, 260, False)
    ops = R.ln_operands(c)
    ref = R.ln_reference(ops)
    good = R.ln_emulate(ops).half()
    assert R.ln_mismatch(good, ref) is None
    und = (G.bits(ref.lo) != G.bits(ref.hi)) & ~ref.const[:, None]
    dec = ~und & ~ref.const[:, None]
    r, col = (int(i) for i in dec.nonzero()[-1])
    moved = good.clone()
    G.bits(moved)[r, col] ^= 1
    msg = R.ln_mismatch(moved, ref)
    assert msg is not None and msg.startswith(f"1 of {good.numel()} elements fail (1 of them decided)") and f"first at ({r}, {col})" in msg
    if bool(und.any()):
        r, col = (int(i) for i in und.nonzero()[0])
        for v in (ref.lo[r, col], ref.hi[r, col]):
            ok = good.clone()
            ok[r, col] = v
            assert R.ln_mismatch(ok, ref) is None
        far = good.clone()
        far[r, col] = ref.hi[r, col].float() * 1.01 + 0.01
        assert R.ln_mismatch(far, ref) is not None
    row = int(ref.const.nonzero()[0])                                     # a constant row takes beta and nothing else
    off = good.clone()
    G.bits(off)[row, 7] ^= 1
    assert "a constant row" in R.ln_mismatch(off, ref)
    g32 = R.ln_emulate(R.ln_operands(c._replace(f32=True)))
    ref32 = R.ln_reference(R.ln_operands(c._replace(f32=True)))
    assert R.ln_mismatch(g32, ref32) is None
    g32 = g32.clone()
    g32[0, 3] += 4 * float(ref32.E[0, 3]) + 1e-6
    assert R.ln_mismatch(g32, ref32) is not None


def test_guards():
    buf, mid = R.guarded(5, 12)
    assert mid.shape == (5, 12) and mid.data_ptr() == buf.data_ptr() + R.GUARD * 12 * 2
    mid.zero_()
    assert R.guards_untouched(buf, 5) is None
    for r in (R.GUARD - 1, R.GUARD + 5):
        b2 = buf.clone()
        b2[r, 3] = 1.0
        assert R.guards_untouched(b2, 5) is not None


# ---- L2 norm -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", R.L2_D)
@pytest.mark.parametrize("rows", R.L2_ROWS)
def test_l2_candidates_and_honest_evaluation(rows, D):
    for kind in R.L2_SETS:
        for row0 in R.l2_row0s(rows):
            X, pinned = R.l2_operands(rows, D, kind, row0)
            pins = R.l2_pins(rows, row0)
            assert int(pinned.sum()) == len(pins)
            if rows > 1:
                assert {"zero", "overflow"} <= set(pins.values())
            if kind == "exact":
                assert R.is_exact_set(X[~pinned])
            exact = ~pinned if kind == "exact" else False
            for times in (1, 2):
                cands = R.l2_candidates(X, times, exact)                  # asserts: at most two norms per application, one on the exact set
                assert len(cands) == 2 ** times
                if kind == "exact" and times == 1:                        # ONE bit pattern, and the general rule contains it
                    assert torch.equal(G.bits(cands[0]), G.bits(cands[1]))
                    assert R.rows_mismatch(cands[0], R.l2_candidates(X, 1)) is None
                for row, pin in pins.items():                             # zeros stay zeros, an overflowing norm gives signed zeros
                    want = X[row].clone() if pin == "zero" else torch.copysign(torch.zeros(D), X[row].float()).half()
                    for cnd in cands:
                        assert torch.equal(G.bits(cnd[row]), G.bits(want)), f"{pin} row {row}"
                got = R.l2_emulate(X, times)
                msg = R.rows_mismatch(got, cands)
                assert msg is None, f"l2-{rows}x{D}-{kind}-x{times}, row 0 {row0}: {msg}"
                norm = got[~pinned].double().norm(dim=1)
                assert bool(((norm - 1).abs() < 2e-3).all())


@pytest.mark.parametrize("kind", R.L2_SETS)
def test_l2_rejects_a_norm_that_is_not_rounded_to_fp16(kind):
    for rows, D in ((131, 768), (131, 260), (5, 64)):
        X, pinned = R.l2_operands(rows, D, kind)
        for times in (1, 2):
            cands = R.l2_candidates(X, times, ~pinned if kind == "exact" else False)
            assert R.rows_mismatch(R.l2_emulate(X, times), cands) is None
            msg = R.rows_mismatch(R.l2_emulate(X, times, "norm_not_rounded"), cands)
            assert msg is not None, f"{kind} {rows}x{D} x{times}: an fp32 norm went unnoticed"
            assert int(msg.split(" of ")[0]) >= 0.5 * (rows - 2), msg


def test_rows_mismatch_is_a_whole_row_rule():
    X, _ = R.l2_operands(131, 768, "model")
    cands = R.l2_candidates(X, 1, exact=False)
    differ = (G.bits(cands[0]) != G.bits(cands[1])).any(1)
    assert bool(differ.any()), "no row of the model-like set has two candidate norms: the rule is not exercised"
    r = int(differ.nonzero()[0])
    cols = (G.bits(cands[0][r]) != G.bits(cands[1][r])).nonzero().flatten()
    assert cols.numel() >= 2
    mixed = cands[0].clone()
    mixed[r, cols[0]] = cands[1][r, cols[0]]                              # one element from the other candidate: no candidate's row
    msg = R.rows_mismatch(mixed, cands)
    assert msg is not None and msg.startswith("1 of 131 rows") and f"row {r} differs" in msg
    assert R.rows_mismatch(cands[1], cands) is None


# ---- ensemble ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", R.ENS_E_V8 + R.ENS_E_ANY)
@pytest.mark.parametrize("T", R.ENS_T)
def test_ensemble_candidates_and_honest_evaluation(T, E):
    for rows in R.ENS_ROWS:
        feats = R.ens_operands(T, rows, E)
        assert feats.shape == (T, rows, E) and R.is_exact_set(feats)
        cands, m = R.ens_reference(feats)                                 # asserts: one norm per template, at most two at the end
        msg = R.rows_mismatch(R.ens_emulate(feats), cands)
        assert msg is None, f"ens-T{T}-{rows}x{E}: {msg}"
        assert torch.equal(G.bits(m), G.bits(R.ens_reference(feats, "mean_quotient")[1]))       # h(acc / T) is the same value
        if T == 1:                                                        # m = h(u_0 * 1)
            assert torch.equal(G.bits(m), G.bits(R.l2_apply(feats[0], exact=True)[0]))


@pytest.mark.parametrize("T", (7, 13))
def test_ensemble_rejects_a_mean_taken_in_fp16_steps(T):
    feats = R.ens_operands(T, 131, 512)
    cands, m = R.ens_reference(feats)
    m_div = R.ens_reference(feats, "mean_div")[1]
    assert not torch.equal(G.bits(m), G.bits(m_div))
    for bad in (R.ens_emulate(feats, "mean_div"), R.ens_reference(feats, "mean_div")[0][0]):
        msg = R.rows_mismatch(bad, cands)
        assert msg is not None, f"T = {T}: h(acc * h(1 / T)) went unnoticed"
        print(f"\nT = {T}: {msg}")


# ---- text front --------------------------------------------------------------------------------------------------------------------

def test_text_tables_tell_rows_and_columns_apart():
    for D in R.TEXT_D:
        tok, pos, prm = R.tok_table(D), R.pos_table(D), R.prompt_table(5, D)
        assert tok.shape == (R.VOCAB, D) and pos.shape == (R.LCTX + 1, D) and prm.shape == (5, R.LCTX, D)
        assert float((tok.half().float() != tok).float().mean()) > 0.75, "h(tok) rarely rounds"
        t16 = tok.half()
        for t in (t16, pos, prm.view(-1, D)):
            for k in (1, 2, 3, 4, 8, 64):
                assert float((t[k:] != t[:-k]).float().mean()) > 0.98, f"rows {k} apart look alike"
            for k in (1, 4, 8, 32):
                assert float((t[:, k:] != t[:, :-k]).float().mean()) > 0.98, f"columns {k} apart look alike"


def test_ids_tie_at_their_maximum_and_the_first_wins():
    for N in R.TEXT_N:
        for stride in R.TEXT_STRIDES:
            ids = R.ids_table(N, stride)
            assert ids.shape == (N, stride) and bool((ids[:, R.LCTX:] == R.PAD_ID).all()) and int(ids[:, :R.LCTX].max()) == R.VOCAB - 1
            index = R.embed_ids_reference(ids, R.tok_table(64), R.pos_table(64), 9)[1]
            for n in range(N):
                p1, p2 = R._MAXIMA[n % len(R._MAXIMA)]
                assert int(index[n]) == p1 and int(ids[n, p2]) == R.VOCAB - 1
                assert [int(v) for v in (ids[n, :R.LCTX] == R.VOCAB - 1).nonzero().flatten()] == sorted({p1, p2})


def test_text_references_against_loops():
    D, N, Lseq = 64, 5, 9
    ids, tok, pos, prm = R.ids_table(N, 80), R.tok_table(D), R.pos_table(D), R.prompt_table(N, D)
    x, index = R.embed_ids_reference(ids, tok, pos, Lseq)
    y = R.add_pos_reference(prm, pos, Lseq)
    for n in range(N):
        for l in range(Lseq):
            want = (tok[ids[n, l]].half().float() + pos[l].float()).half()
            assert torch.equal(G.bits(x[n * Lseq + l]), G.bits(want))
            assert torch.equal(G.bits(y[n * Lseq + l]), G.bits((prm[n, l].float() + pos[l].float()).half()))
    idx = R.gather_indices(7, Lseq)
    x7 = R.prompt_table(7, D)[:, :Lseq].reshape(7 * Lseq, D)
    got = R.gather_reference(x7, idx, Lseq)
    for n in range(7):
        assert torch.equal(got[n], x7[n * Lseq + min(max(int(idx[n]), 0), Lseq - 1)])
    assert int(idx.min()) < 0 and int(idx.max()) >= Lseq
    base, tokens, labels = R.prompt_table(6, D), R.tok_table(D)[:10].view(5, 2, D), torch.tensor([3, 0, 5, 5, 1])
    for lab in (labels, None):
        out = R.assemble_reference(base, lab, tokens, 2)
        assert out.shape == (5, R.LCTX, D)
        for c in range(5):
            src = base[int(lab[c]) if lab is not None else 0]
            assert torch.equal(out[c, :2], src[:2]) and torch.equal(out[c, 2:4], tokens[c].half()) and torch.equal(out[c, 4:], src[2:R.LCTX - 2])


@pytest.mark.parametrize("defect", R.TEXT_DEFECTS)
def test_text_rejects_planted_defects(defect):
    for D in (64, 768):
        ids, tok, pos = R.ids_table(5, 80), R.tok_table(D), R.pos_table(D)
        want = R.embed_ids_reference(ids, tok, pos, R.LCTX)[0]
        msg = G.bits_mismatch(R.embed_ids_reference(ids, tok, pos, R.LCTX, defect)[0], want)
        assert msg is not None, f"{defect} went unnoticed in the embedding add"
        print(f"\nembed, D = {D}, {defect}: {msg.split(';')[0]}")
        if defect == "pos_row+1":
            prm = R.prompt_table(5, D)
            assert G.bits_mismatch(R.add_pos_reference(prm, pos, 9, defect), R.add_pos_reference(prm, pos, 9)) is not None


def test_report_figures():
    """Prints the LayerNorm table of the module docstring of rowops_exact.py for the cases run in this session."""
    for cid, (share, k, t) in _FIGURES.items():
        print(f"\n    {cid:22s} undecided {share:6.2%}   err / E {k:.3f} {t:.3f}")
