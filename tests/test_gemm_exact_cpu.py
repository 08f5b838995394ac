"""CPU companion of test_hip_gemm_exact.py: every case of gemm_exact.CASES keeps the exactness promise, the case list reaches every
branch of the GEMM dispatcher it names (gemm_exact.route restates the dispatcher that gemm_f16_route replaced, branch by branch), and the comparator the GPU
test applies -- bit equality with the reference -- rejects the defects it is there for, planted into a torch emulation of the kernel
(gemm_exact.emulate).  Pure torch: no library, no GPU.

The slow statements run on a row range of the large cases (the first 128 rows, whole images for EPI_PATCH); the exactness condition
itself is asserted on the whole operands.  Shares measured here over all cases (test_report_measured_shares prints them):
    one lost product, share of its 64-row band that changes bits       98.3 % .. 100 %     (bound: 90 %)
    one K-tile read twice in place of its neighbour                    99.8 % .. 100 %     (bound: 90 %)
    one-rounding residual form h(acc + b + res), cases with K >= 768   18.1 % .. 20.3 %    (bound: 5 %)
                                                 cases with K < 768    1.14 % .. 6.28 %    (bound: one element)
    bias of the neighbouring column                                    99.0 % .. 100 %     (bound: 50 %)
    residual / positional row of the neighbouring row                  99.95 % .. 100 %    (bound: 50 %)
"""
import pytest
import torch

import gemm_exact as G

F16_CASES = [c for c in G.CASES if c.kind != "f32"]
_SHARES = {}


def _ids(c):
    return c.id


def _rows(c):
    """The row range the emulation runs on: the first 128 rows, for EPI_PATCH the first images (at least 98 rows)."""
    if c.epi == G.EPI_PATCH:
        return slice(0, c.rows[0] * max(1, 98 // c.rows[0]))
    return slice(0, min(c.M, 128))


def _note(key, case, share):
    lo, hi, _ = _SHARES.get(key, (2.0, -1.0, ""))
    _SHARES[key] = (min(lo, share), max(hi, share), case.id if share < lo else _SHARES[key][2])


@pytest.mark.parametrize("c", G.CASES, ids=_ids)
def test_case_is_exact(c):
    """assert_exact on the whole operands (p <= 8, sum of |products| < K <= 4096); on the row range the fp32 product equals the fp64
    product bit for bit, and so do fp32 sums over K-tiles of 64 in forward and in reverse order and one product at a time over the
    first and last 64 k; the emulation without a defect equals the reference.  Statistics cases: the integer operand set is exact too
    and its stored rows are integers within 64 (expected_stats asserts), on ALL rows."""
    ops = G.operands(c)
    p, bound = G.assert_case_exact(c, ops)
    assert p == 8 and bound < 2 ** 12
    A, W, bias, res, pos = ops
    assert A.shape == (c.M, c.K) and W.shape == (c.N, c.K) and bias.shape == (c.N,) and res.shape == (c.out_rows, c.N)
    rows = _rows(c)
    a, w = A[rows].float(), W.float()
    acc = G.product(A[rows], W, check64=True)
    exact = a.double() @ w.double().t()
    rev = torch.zeros_like(acc)
    for kt in reversed(range(c.K // 64 if c.K % 64 == 0 else 0)):
        rev += a[:, kt * 64:kt * 64 + 64] @ w[:, kt * 64:kt * 64 + 64].t()
    if c.K % 64 == 0:
        assert torch.equal(rev.double(), exact)
    seq = torch.zeros_like(acc)
    ks = sorted(set(range(min(c.K, 64))) | set(range(max(0, c.K - 64), c.K)))
    for k in ks:                                                          # strictly sequential fp32 sums, one product at a time
        seq += a[:, k, None] * w[None, :, k]
    assert torch.equal(seq.double(), a[:, ks].double() @ w[:, ks].double().t())
    if c.kind != "f32" and c.epi != G.EPI_BIAS_QGELU:
        out_rows = slice(0, rows.stop // c.rows[0] * c.rows[1]) if c.epi == G.EPI_PATCH else rows
        want = G.epilogue(c, acc, bias, res[out_rows], pos)
        assert want.dtype == torch.float16 and G.bits_mismatch(G.emulate(c, ops, rows), want) is None
        assert bool(torch.isfinite(want.float()).all())                  # (EPI_SCALE: |h(acc) * 100| stays far below the fp16 range)
        if c.epi != G.EPI_NONE:                                           # the epilogue really rounds: fp32 and fp16 disagree somewhere
            x = acc + bias.float() if c.epi in (G.EPI_BIAS, G.EPI_BIAS_RES) else acc
            assert c.K < 768 or float((x.half().float() != x).float().mean()) > 0.1
    if c.kind == "stats":
        iops = G.operands(c, integer=True)
        G.assert_exact(iops[0], iops[1], c.id + " (integer set)")
        want, _ = G.expected(c, iops)
        st = G.expected_stats(want)
        assert st.shape == (c.M, c.N // 256, 2) and float(st[..., 1].min()) > 0


def test_every_case_takes_the_branch_it_is_listed_for():
    """Case.want against the restated dispatcher, and the list as a whole against the instantiations the dispatcher can reach: both
    tile heights x the three K loops x a_nt for BIAS_RES, nontemporal stores for NONE / BIAS / QGELU / SCALE on both tile heights, both
    n_group arms, every split-K depth, every epilogue on every kernel that takes it and on the ping-pong loop."""
    for c in F16_CASES:
        assert c.want, c.id
        for v, want in c.want.items():
            got = G.route(v, c.M, c.N, c.K, c.epi, c.ldc, c.ldres, c.kind == "stats")
            assert got == want, f"{c.id}, variant {v}: listed for {want}, the dispatcher takes {got}"
    G.assert_coverage()
    # what test_hip_kernels.test_gemm_f16's twelve shapes reach is not enough (no a_nt, no nontemporal store, no boundary loop on 128-row tiles)
    old = [(256, 256, 256, 1), (591, 768, 768, 3), (1000, 3072, 768, 2), (130, 2304, 768, 1), (5, 128, 128, 0), (64, 1000, 512, 5), (37, 6, 128, 5),
           (784, 768, 768, 4), (300, 768, 3072, 3), (1, 512, 768, 0), (2048, 512, 2048, 3), (513, 1536, 512, 1)]
    with pytest.raises(AssertionError):
        G.assert_coverage([G.Case("f16", *s, {}) for s in old])
    got = G.reached()
    assert (G.EPI_BIAS_RES, ("v5", 128, "boundary", "a_nt", "", "")) in got       # boundary loop + nontemporal A stream on 128-row tiles: launched by no earlier kernel test
    f32 = [c for c in G.CASES if c.kind == "f32"]
    for vals, field in (((1, 63, 64, 65, 300), "M"), ((4, 100, 128, 130), "N"), ((32, 96, 512, 2048), "K"), ((0, 1, 3), "epi")):
        assert set(vals) <= {getattr(c, field) for c in f32}


@pytest.mark.parametrize("c", [c for c in G.CASES if c.epi != G.EPI_BIAS_QGELU], ids=_ids)
def test_comparator_rejects_planted_defects(c):
    ops = G.operands(c)
    rows = _rows(c)
    n = rows.stop
    good = G.emulate(c, ops, rows)
    keep = G.compared_rows(c)[:good.shape[0]]
    assert G.bits_mismatch(good.clone(), good) is None

    def share(defect, sel=slice(None), **kw):
        bad = G.emulate(c, ops, rows, defect, **kw)
        assert G.bits_mismatch(bad, good) is not None, f"{c.id}: {defect} went unnoticed"
        k = keep.clone()
        m = torch.zeros_like(k)
        m[sel] = True
        return G.share_differing(bad[k & m], good[k & m])

    # 1. one lost product in one 64-row band: at least 90 % of the band's outputs change bits
    band = slice(0, min(64, n, c.rows[0] or n))
    out_band = slice(1, 1 + band.stop) if c.epi == G.EPI_PATCH else band
    s = share("lost_product", out_band, band=band)
    _note("lost product", c, s)
    assert s >= 0.9, f"{c.id}: a lost product changes only {s:.1%} of its band"
    # 2. one K-tile of 64 read twice in place of its neighbour
    if c.K >= 2 * G.k_tile(c):
        s = share("tile_twice")
        _note("K-tile read twice", c, s)
        assert s >= 0.9, f"{c.id}: a K-tile read twice changes only {s:.1%} of the outputs"
    # 3. the one-rounding residual form h(acc + b + res)
    if c.epi == G.EPI_BIAS_RES and c.kind != "f32":
        s = share("one_rounding")
        _note("one rounding, K >= 768" if c.K >= 768 else "one rounding, K < 768", c, s)
        assert s >= 0.05 or c.K < 768, f"{c.id}: the one-rounding form differs in {s:.2%} of the elements only"
    # 4. bias of the neighbouring column, residual / positional row of the neighbouring row
    if c.epi in (G.EPI_BIAS, G.EPI_BIAS_RES):
        s = share("bias_column")
        _note("bias column", c, s)
        assert s >= 0.5, f"{c.id}: bias_column {s:.1%}"
    if c.epi in (G.EPI_BIAS_RES, G.EPI_PATCH):
        s = share("res_row")
        _note("residual row", c, s)
        assert s >= 0.5, f"{c.id}: res_row {s:.1%}"
    # 5. the message places the defect: one flipped bit at a known (row, column)
    r, col = good.shape[0] - 1, c.N - 1
    moved = good.clone()
    G.bits(moved)[r, col] ^= 1
    msg = G.bits_mismatch(moved, good)
    assert msg is not None and msg.startswith(f"1 of {good.numel()} elements") and f"first at ({r}, {col})" in msg
    assert f"row {r % 256} of its 256-row tile ({r % 64} mod 64), column {col % 256} of its 256-column tile ({col % 64} mod 64)" in msg


@pytest.mark.parametrize("c", [c for c in G.CASES if c.ldc], ids=_ids)
def test_sentinel_check_sees_a_store_into_column_n(c):
    """ldc > N: a store into column N of any row, or into the first row behind M, is reported; the clean buffer is not."""
    assert c.ldc > c.N
    buf = G.sentinel_buffer(c.M + G.PAD_ROWS, c.ldc)
    buf[:c.M, :c.N] = 1.0
    assert G.outside_untouched(buf, c.M, c.N) is None
    for r, col in ((0, c.N), (c.M - 1, c.N), (c.M // 2, c.ldc - 1), (c.M, 0), (c.M + G.PAD_ROWS - 1, c.ldc - 1)):
        bad = buf.clone()
        bad[r, col] = 1.0
        msg = G.outside_untouched(bad, c.M, c.N)
        assert msg is not None and f"({r}, {col})" in msg
    same = buf.clone()
    G.bits(same)[c.M - 1, c.N] = G.SENTINEL                    # (the sentinel written over itself cannot be seen: that is the check's limit)
    assert G.outside_untouched(same, c.M, c.N) is None


def test_statistics_comparison_rejects_a_slot_mixup():
    """The statistics are compared bit for bit: the pair of the neighbouring slot, of the neighbouring row, or a sum over the unrounded
    h(acc + b) + res of the standard set (no integers) all differ from the expected pairs."""
    c = next(c for c in G.CASES if c.kind == "stats" and c.N == 768 and c.M < 1000)
    want, _ = G.expected(c, G.operands(c, integer=True))
    st = G.expected_stats(want)
    assert G.share_differing(st.roll(1, 1).reshape(c.M, -1), st.reshape(c.M, -1)) > 0.9
    assert G.share_differing(st.roll(1, 0).reshape(c.M, -1), st.reshape(c.M, -1)) > 0.9
    with pytest.raises(AssertionError):
        G.expected_stats(G.expected(c)[0])


def test_report_measured_shares():
    """Prints the smallest and largest share per planted defect over the cases run in this session (the figures of the docstring)."""
    for key, (lo, hi, case) in sorted(_SHARES.items()):
        print(f"\n{key}: {lo:.2%} .. {hi:.2%} (smallest: {case})")
        assert lo > 0
