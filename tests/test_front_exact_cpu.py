"""CPU companion of test_hip_front_exact.py: the reference of front_exact.py is conv1 (not our reading of the index order), fold is its
inverse, the fused cases reach every branch they are listed for, and every case -- fused and im2col -- rejects every named index mistake
(front_exact.MUTANTS): the mistake changes the very bits the GPU test compares.  Pure torch: no library, no GPU."""
import pytest
import torch

import front_exact as F
import gemm_exact as G


@pytest.mark.parametrize("P", [14, 16, 32])
def test_unfold_is_conv1(P):
    """unfold(img) @ W.T == conv2d(img, W.view(N, 3, P, P), stride = P) in float64, on integer operands (both sides exact), with and without padding."""
    g = torch.Generator().manual_seed(P)
    B, R, N, K = 3, 3 * P, 5, 3 * P * P
    img = torch.randint(-8, 9, (B, 3, R, R), generator=g).double()
    W = torch.randint(-8, 9, (N, K), generator=g).double()
    conv = torch.nn.functional.conv2d(img, W.view(N, 3, P, P), stride=P)                  # [B, N, G, G]
    want = conv.permute(0, 2, 3, 1).reshape(-1, N)
    assert torch.equal(F.unfold(img, P) @ W.t(), want)
    Kpad = (K + 63) // 64 * 64 + 64
    padded = F.unfold(img, P, Kpad)
    assert padded.shape == (B * 9, Kpad) and torch.equal(padded[:, :K], F.unfold(img, P)) and not bool(padded[:, K:].any())
    assert not bool(G.bits(F.unfold(-img.half(), P, Kpad)[:, K:]).any()), "the padding is +0"


@pytest.mark.parametrize("key", list(F.FUSED), ids=str)
def test_fold_inverts_unfold(key):
    B, R, N = key
    c = F.fused_case(*key)
    A = G.operands(c)[0]
    img = F.fused_image(c, R)
    assert img.shape == (B, 3, R, R) and img.dtype == torch.float16 and img.is_contiguous()
    assert torch.equal(G.bits(F.unfold(img, 16)), G.bits(A))
    assert torch.equal(G.bits(F.fold(F.unfold(img, 16), R)), G.bits(img))
    G.assert_case_exact(c)


def test_fused_cases_reach_their_branches():
    for key, want in F.FUSED.items():
        assert set(want) == set(G.GEMM_VARIANTS)
        for v, branch in want.items():
            assert F.fused_route(v, *key) == branch, f"{key}, variant {v}: {F.fused_route(v, *key)}, listed for {branch}"
    for v, branch in F.GUARD_WANT.items():
        assert F.fused_route(v, F.GUARD_B, F.GUARD_R, F.GUARD_N) == branch
        assert F.fused_route(v, F.GUARD_B + 1, F.GUARD_R, F.GUARD_N) == ("err", -4)
    image = 3 * F.GUARD_R * F.GUARD_R * 2
    assert F.GUARD_B * image < 2 ** 31 - 1 <= (F.GUARD_B + 1) * image
    F.assert_coverage()
    for key in F.FUSED:                               # ... and the coverage check notices a branch that is gone
        rest = [k for k in F.FUSED if F.FUSED[k] != F.FUSED[key]]
        with pytest.raises(AssertionError):
            F.assert_coverage(rest)


def _patch_rows(c, acc, rows, pos):
    """EPI_PATCH on single rows of the product: h(h(acc) + pos[1 + p]), p the patch of the row."""
    p = rows % c.rows[0]
    return (acc.half().float() + pos.float()[1 + p]).half()


@pytest.mark.parametrize("key", list(F.FUSED), ids=str)
def test_fused_case_rejects_every_mutant(key):
    """Every mutant of the gather changes rows of A, and on (up to 96 of) those rows the expected output bits: the first, the last and
    evenly spaced ones between."""
    B, R, N = key
    c = F.fused_case(*key)
    ops = G.operands(c)
    A, W, _, _, pos = ops
    want, _ = G.expected(c, ops)
    g2 = c.rows[0]
    report = []
    for name, mutant in F.MUTANTS.items():
        if not F.applies(name, B, R // 16, 16, F.K16):
            assert name in ("gy and gx transposed", "padding 1.0 instead of 0") and (R == 16 or name.startswith("padding")), (key, name)
            Am = mutant(A, B, R // 16, 16)
            assert torch.equal(G.bits(Am), G.bits(A)), f"{key}: '{name}' is listed as the same function here and is not"
            report.append(f"{name}: the same function at this shape")
            continue
        Am = mutant(A, B, R // 16, 16)
        changed = (G.bits(Am) != G.bits(A)).any(1).nonzero().flatten()
        assert changed.numel() > 0, f"{key}: '{name}' changes no row of the patch matrix"
        rows = changed[torch.linspace(0, changed.numel() - 1, min(96, changed.numel())).long()]
        got = _patch_rows(c, G.product(Am[rows], W, check64=True), rows, pos)
        out_rows = rows // g2 * (g2 + 1) + 1 + rows % g2
        assert torch.equal(G.bits(_patch_rows(c, G.product(A[rows], W), rows, pos)), G.bits(want[out_rows])), "the row form of the epilogue is not the reference's"
        differ = (G.bits(got) != G.bits(want[out_rows])).any(1)
        assert bool(differ.all()), f"{key}: '{name}' passes on {int((~differ).sum())} of {rows.numel()} changed rows"
        report.append(f"{name}: detected ({changed.numel()} rows change)")
    print(f"\n{key}: " + "; ".join(report))


@pytest.mark.parametrize("case", F.IM2COL, ids=str)
def test_im2col_case_rejects_every_mutant(case):
    P, R, Kpad = case
    G_ = R // P
    report = []
    for dtype in (F.F16, F.F32):
        for B in F.IM2COL_B:
            img = F.im2col_image(dtype, B, R)
            true = F.unfold(img, P, Kpad)
            want = F.im2col_expected(img, P, Kpad)
            assert want.dtype == torch.float16 and want.shape == (B * G_ * G_, Kpad)
            if dtype == F.F32:
                present = {float(v) for v in true.flatten().tolist()}
                assert all(float(torch.tensor(v, dtype=torch.float32)) in present for v in F.CAST_VALUES), "a cast value is in no patch"
            for name, mutant in F.MUTANTS.items():
                if not F.applies(name, B, G_, P, Kpad):
                    assert (G_ == 1 and name.startswith("gy")) or (B == 1 and "neighbour" in name) or (B * G_ * G_ == 1 and "M - 2" in name) \
                        or (Kpad == 3 * P * P and name.startswith("padding")), (case, B, name)
                    continue
                got = mutant(true, B, G_, P).half()
                assert not torch.equal(G.bits(got), G.bits(want)), f"{case}, type {dtype}, B = {B}: '{name}' changes no bit of the expected matrix"
                report.append(name)
    print(f"\n{case}: detected, over 2 types and B in {F.IM2COL_B}: " + "; ".join(f"{n} x{report.count(n)}" for n in F.MUTANTS))


def test_cast_values_round_as_stated():
    """torch's fp32 -> fp16 on the CPU, the reference of the cast: round to nearest even, +-inf beyond 65520, subnormals, signed zero."""
    h = lambda v: float(torch.tensor(v, dtype=torch.float32).half())
    T = 2.0 ** -11
    assert h(1 + T) == 1.0 and h(1 + 3 * T) == 1 + 2.0 ** -9 and h(-(1 + T)) == -1.0 and h(1 + T + 2.0 ** -23) == 1 + 2.0 ** -10 and h(1 + T - 2.0 ** -23) == 1.0
    assert h(2049.0) == 2048.0 and h(2051.0) == 2052.0 and h(65519.0) == 65504.0 and h(65520.0) == float("inf") and h(-65520.0) == float("-inf")
    assert h(1.0e5) == float("inf") and h(-(2.0 ** 127)) == float("-inf")
    assert h(2.0 ** -24) == 2.0 ** -24 and h(2.0 ** -25) == 0.0 and h(2.0 ** -25 * (1 + 2.0 ** -10)) == 2.0 ** -24 and h(3 * 2.0 ** -25) == 2.0 ** -23
    assert h(2.0 ** -14 - 2.0 ** -25) == 2.0 ** -14 and h(1023 * 2.0 ** -24) == 1023 * 2.0 ** -24
    assert int(G.bits(torch.tensor([-0.0, -(2.0 ** -25)], dtype=torch.float32).half())[0]) == -0x8000 and int(G.bits(torch.tensor([-(2.0 ** -25)]).half())[0]) == -0x8000
    assert not any(v != v for v in F.CAST_VALUES)
