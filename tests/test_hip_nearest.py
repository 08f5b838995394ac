"""The nearest-exemplar search on the device (ovmr_amd/csrc/nearest.hip, include/ovmr_hip_nearest.h) against nearest_cases.py:

  a. every exact case at every forced slice count (1, 2, 3, one per tile, one more): indices bit for bit, values as numbers, equal to the
     stable descending sort of the CPU's fp16 score matrix -- hence equal to each other, whatever the grid;
  b. the named cases: a tie that decides membership, an all-zero bank, signed zeros, a NaN row, +-inf scores, the range table (empty,
     one row, fewer than k, across a tile and a slice boundary, the whole bank, a query tile whose later slices have nothing to do);
  c. the bank of just over 2^31 bytes against its analytic expectation;
  d. clustered L2-normalised features by margin (nearest_cases.general_mismatch);
  e. the production entry equals the hook at the launcher's own slice count;
  f. scratch pre-filled with each of poison.FILLS gives the same bits; guards around values / indices survive;
  g. runtime.nearest_rows repairs a strided queries view.
Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes

import pytest
import torch

import nearest_cases as N
import poison as P

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    yield runtime.load_library()
    torch.cuda.empty_cache()


def hook(lib, Q, X, k, slices, ranges=None, fill=None, out=None):
    """ovmr_debug_nearest_rows on device tensors with a scratch of exactly B * slices * k keys (pre-filled with `fill`)."""
    B, D = Q.shape
    R = X.shape[0]
    scratch = torch.empty((max(1, B * slices * k),), dtype=torch.int64, device=Q.device)
    if fill is not None:                                          # the pattern's bits in every 32-bit word of the keys
        scratch.view(torch.int32).fill_(P._i32(P.FILLS[fill]))
    values, indices = out if out is not None else (torch.empty((B, k), dtype=torch.float32, device=Q.device),
                                                    torch.empty((B, k), dtype=torch.int32, device=Q.device))
    rc = lib.ovmr_debug_nearest_rows(_p(Q), B, _p(X), R, D, k, _p(ranges), _p(values), _p(indices), _p(scratch), B * slices * k * 8, slices,
                                     _stream())
    assert rc == 0, f"ovmr_debug_nearest_rows returned {rc} (B={B} R={R} D={D} k={k} slices={slices})"
    return values, indices


def _check_all_slices(lib, Q, X, k, want, ranges=None, what=""):
    Qd, Xd = Q.cuda(), X.cuda()
    rd = None if ranges is None else ranges.cuda()
    for s in N.slices_for(X.shape[0]):
        msg = N.mismatch(hook(lib, Qd, Xd, k, s, rd), want)
        assert msg is None, f"{what}, slices = {s}: {msg}"


@pytest.mark.parametrize("B,R,D,k", N.SHAPES)
def test_exact_shapes(lib, B, R, D, k):
    Q, X, s16 = N.exact_case(B, R, D, k, seed=B + R + D + k)
    _check_all_slices(lib, Q, X, k, N.expected(s16, k), what=f"B={B} R={R} D={D} k={k}")


@pytest.mark.parametrize("name", ["tie_cut", "zero_bank", "signed_zero", "nan_row", "inf_rows"])
def test_named_cases(lib, name):
    if name == "tie_cut":
        k = 2
        Q, X, s16 = N.tie_cut_case(k)
        want = N.expected(s16, k)
        assert want[1][:, :2].tolist() == [[3, 290]] * Q.shape[0]
    elif name == "zero_bank":
        k = 32
        Q, X, s16 = N.zero_bank_case()
        want = N.expected(s16, k)
        assert want[1][0].tolist() == list(range(k))
    elif name == "signed_zero":
        k = 8
        Q, X, s16 = N.signed_zero_case()
        want = N.expected(s16, k)
        assert want[1][0].tolist() == [X.shape[0] - 1] + list(range(k - 1))
    elif name == "nan_row":
        k = 5
        Q, X, s16 = N.exact_case(65, 1000, 128, k, 9, nan_row=777)
        want = N.expected(s16, k)
        assert bool((want[1][:, 0] == 777).all()) and bool(torch.isnan(want[0][:, 0]).all())
    else:
        k = 5
        Q, X, s16 = N.exact_case(65, 1000, 128, k, 10, inf_row=600)
        want = N.expected(s16, k)
        assert bool(torch.isinf(want[0]).any()) and bool(torch.isinf(s16).any(1)[2::5].all())
    _check_all_slices(lib, Q, X, k, want, what=name)


@pytest.mark.parametrize("B,R,D,k", [(130, 1000, 128, 5), (65, 1000, 1024, 32), (130, 70001, 64, 31)])
def test_ranges(lib, B, R, D, k):
    Q, X, s16 = N.exact_case(B, R, D, k, seed=3 * B + R)
    for cut_slices in (2, 3):
        ranges = N.range_table(B, R, k, cut_slices)
        _check_all_slices(lib, Q, X, k, N.expected(s16, k, ranges), ranges, what=f"ranges (boundary of {cut_slices} slices) B={B} R={R} D={D} k={k}")


def test_bank_beyond_2_31_bytes(lib):
    k = 5
    Q, planted = N.big_bank_plan(k)
    X = N.big_bank_fill(torch.zeros((N.BIG_R, N.BIG_D), dtype=torch.float16, device="cuda"), planted)
    assert X.numel() * 2 > 2 ** 31
    want = N.big_bank_expected(Q, planted, k)
    Qd = Q.cuda()
    for s in (1, 3, 512):
        msg = N.mismatch(hook(lib, Qd, X, k, s), want)
        assert msg is None, f"slices = {s}: {msg}"
    from ovmr_amd import runtime
    msg = N.mismatch(runtime.nearest_rows(Qd, X, k), want)
    assert msg is None, f"production entry: {msg}"
    del X


@pytest.mark.parametrize("D,k", [(512, 5), (128, 32), (1024, 5)])
def test_general_by_margin(lib, D, k):
    from ovmr_amd import runtime
    Q, X = N.general_case(D, seed=D + k)
    Qd, Xd = Q.cuda(), X.cuda()
    for s in (1, 4):
        msg = N.general_mismatch(hook(lib, Qd, Xd, k, s), Q, X, k)
        assert msg is None, f"slices = {s}: {msg}"
    starts = torch.arange(Q.shape[0]) % 50 * 20                   # the rows of one class each
    ranges = torch.stack([starts, starts + 20], 1).to(torch.int32)
    msg = N.general_mismatch(runtime.nearest_rows(Qd, Xd, k, ranges), Q, X, k, ranges)
    assert msg is None, f"one class per query: {msg}"


@pytest.mark.parametrize("B,R,D,k", [(65, 1000, 128, 5), (130, 70001, 64, 32), (1, 257, 1024, 1)])
def test_production_entry_equals_hook(lib, B, R, D, k):
    from ovmr_amd import runtime
    Q, X, s16 = N.exact_case(B, R, D, k, seed=B + R)
    Qd, Xd = Q.cuda(), X.cuda()
    need = lib.ovmr_nearest_scratch_bytes(B, R, k)
    assert need > 0 and need % (B * k * 8) == 0
    S = need // (B * k * 8)
    got = runtime.nearest_rows(Qd, Xd, k)
    want = hook(lib, Qd, Xd, k, S)
    assert torch.equal(got[1], want[1]) and P.same_bits(got[0], want[0]) is None
    assert N.mismatch(got, N.expected(s16, k)) is None


def test_scratch_contents_do_not_matter_and_guards_survive(lib):
    B, R, D, k = 65, 1000, 128, 5
    Q, X, s16 = N.exact_case(B, R, D, k, seed=1)
    ranges = N.range_table(B, R, k)
    want = N.expected(s16, k, ranges)
    first = None
    for fill in P.FILLS:
        arena = P.Arena(fill, device="cuda")
        Qd, Xd = arena.place(Q), arena.place(X)
        rd = arena.place(ranges)
        values = arena.take(B * k, "f32").view(B, k)
        indices = arena.take(B * k, "i32").view(B, k)
        for s in (1, 3, 4):
            got = hook(lib, Qd, Xd, k, s, rd, fill=fill, out=(values, indices))
            torch.cuda.synchronize()
            assert arena.intact(), f"fill '{fill}', slices = {s}: a guard was written to"
            msg = N.mismatch(got, want)
            assert msg is None, f"fill '{fill}', slices = {s}: {msg}"
            if first is None:
                first = (got[0].clone(), got[1].clone())
            assert P.same_bits(got[0], first[0]) is None and torch.equal(got[1], first[1]), f"fill '{fill}', slices = {s}: other bits"


def test_wrapper_repairs_strided_queries(lib):
    from ovmr_amd import runtime
    B, R, D, k = 63, 255, 64, 5
    Q, X, s16 = N.exact_case(B, R, D, k, seed=2)
    wide = torch.zeros((B, 2 * D), dtype=torch.float16, device="cuda")
    wide[:, ::2] = Q.cuda()
    view = wide[:, ::2]
    assert not view.is_contiguous()
    got = runtime.nearest_rows(view, X.cuda(), k)
    want = runtime.nearest_rows(Q.cuda(), X.cuda(), k)
    assert torch.equal(got[1], want[1]) and P.same_bits(got[0], want[0]) is None
    assert N.mismatch(got, N.expected(s16, k)) is None
    out = (torch.empty((B, k), dtype=torch.float32, device="cuda"), torch.empty((B, k), dtype=torch.int32, device="cuda"))
    again = runtime.nearest_rows(Q.cuda(), X.cuda(), k, out=out)
    assert again[0] is out[0] and torch.equal(out[1], want[1])
