"""The neighbour search with exclusions on the device (ovmr_amd/csrc/neighbours.hip and the EXCL instantiations of nearest.hip,
include/ovmr_hip_audit.h) against audit_cases.py.  Both paths are called through ovmr_debug_neighbours_rows:

  a. the short path (one wave per query) on exact operands: every B, D, k and trip length of audit_cases.SHORT_SHAPES with the range
     and exclusion tables of audit_cases.short_tables (lengths around k, a pass and a trip; exactly max_range; max_range + 3, truncated;
     ranges from row 0 and up to R; every kind of exclusion, unclamped values included) -- indices bit for bit, values as numbers;
  b. its planted rows: ties inside a range, the cut at k decided by a tie, a NaN row, +-inf scores, an all-zero query, signed zeros;
  c. the tiled path with exclusions at every forced slice count, with ranges and with ranges NULL;
  d. both paths on the same exact case: equal to the expectation, hence to each other; general operands by margin;
  e. the production entry equals the hook; the short path with scratch = NULL;
  f. a short range past 2^31 bytes of a bank of just over 2^31 bytes;
  g. scratch and arena pre-filled with each of poison.FILLS: same bits, guards intact;
  h. argument refusals, which launch nothing.
Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes
import math

import pytest
import torch

import audit_cases as A
import nearest_cases as N
import poison as P

pytestmark = pytest.mark.gpu


def _p(t):
    return t if t is None or isinstance(t, ctypes.c_void_p) else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    yield runtime.load_library()
    torch.cuda.empty_cache()


def hook(lib, Q, X, k, path, ranges=None, exclude=None, max_range=0, slices=1, fill=None, out=None, no_scratch=False):
    """ovmr_debug_neighbours_rows on device tensors; path 0 gets a scratch of exactly B * slices * k keys (pre-filled with `fill`)."""
    B, D = Q.shape
    R = X.shape[0]
    scratch, nbytes = None, 0
    if not no_scratch:
        scratch = torch.empty((max(1, B * slices * k),), dtype=torch.int64, device=Q.device)
        nbytes = B * slices * k * 8
        if fill is not None:
            scratch.view(torch.int32).fill_(P._i32(P.FILLS[fill]))
    values, indices = out if out is not None else (torch.empty((B, k), dtype=torch.float32, device=Q.device),
                                                    torch.empty((B, k), dtype=torch.int32, device=Q.device))
    rc = lib.ovmr_debug_neighbours_rows(_p(Q), B, _p(X), R, D, k, _p(ranges), _p(exclude), max_range, _p(values), _p(indices), _p(scratch),
                                        nbytes, path, slices, _stream())
    assert rc == 0, f"ovmr_debug_neighbours_rows returned {rc} (B={B} R={R} D={D} k={k} path={path} slices={slices} max_range={max_range})"
    return values, indices


def _dev(t):
    return None if t is None else t.cuda()


# ---- a. the short path ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,R,D,k,max_range", A.SHORT_SHAPES)
def test_short_exact_shapes(lib, B, R, D, k, max_range):
    Q, X, s16 = N.exact_case(B, R, D, k, seed=B + R + D + k + max_range)
    ranges, excl = A.short_tables(B, R, k, max_range, seed=B + D)
    want = A.expected(s16, k, ranges, excl, max_range)
    if B > 12 and max_range + 3 <= R:
        b = 12                                                    # the range of max_range + 3 rows is truncated: the expectation says so
        lo, hi = A.clamp_pair(ranges[b, 0], ranges[b, 1], R)
        assert hi - lo == max_range + 3 and all(r < lo + max_range for r in want[1][b].tolist())
    got = hook(lib, Q.cuda(), X.cuda(), k, 1, ranges.cuda(), excl.cuda(), max_range)
    msg = A.mismatch(got, want)
    assert msg is None, f"with exclusions: {msg}"
    msg = A.mismatch(hook(lib, Q.cuda(), X.cuda(), k, 1, ranges.cuda(), None, max_range), A.expected(s16, k, ranges, None, max_range))
    assert msg is None, f"exclude = NULL: {msg}"


# ---- b. planted rows ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ties", "tie_cut", "nan_row", "inf_rows", "signed_zero"])
def test_short_planted_rows(lib, name):
    max_range = 100
    if name in ("ties", "tie_cut"):
        k = 5 if name == "ties" else 2
        Q, X, s16, ranges = A.planted_short_case(k)
        excl = torch.tensor([[0, 0], [110, 111], [131, 132], [0, 0], [150, 151], [105, 140]], dtype=torch.int32)
        want = A.expected(s16, k, ranges, excl, max_range)
        assert want[1][0, :2].tolist() == [110, 131] and want[1][1, :2].tolist() == [131, 150] and want[1][2, :2].tolist() == [110, 150]
        assert want[1][3].tolist() == list(range(100, 100 + k)), "the all-zero query: the range's first rows"
    elif name == "nan_row":
        k = 5
        Q, X, s16 = N.exact_case(9, 300, 128, k, 9, nan_row=140)
        ranges = torch.tensor([[100, 170]] * 9, dtype=torch.int32)
        excl = torch.tensor([[0, 0]] * 8 + [[140, 141]], dtype=torch.int32)
        want = A.expected(s16, k, ranges, excl, max_range)
        assert bool((want[1][:8, 0] == 140).all()) and bool(torch.isnan(want[0][:8, 0]).all()) and not bool(torch.isnan(want[0][8]).any())
    elif name == "inf_rows":
        k = 5
        Q, X, s16 = N.exact_case(9, 300, 128, k, 10, inf_row=150)
        ranges = torch.tensor([[100, 170]] * 9, dtype=torch.int32)
        excl = None
        want = A.expected(s16, k, ranges, excl, max_range)
        assert bool(torch.isinf(want[0]).any()) and float(want[0][7, 0]) == math.inf and float(s16[2, 150]) == -math.inf
    else:
        k = 8
        Q, X, s16 = N.signed_zero_case(R=400)
        ranges = torch.tensor([[0, 60], [1, 9], [340, 400]], dtype=torch.int32)
        excl = None
        want = A.expected(s16, k, ranges, excl, max_range)
        assert want[1][0].tolist() == list(range(k)) and want[1][2, 0] == 399
    got = hook(lib, Q.cuda(), X.cuda(), k, 1, ranges.cuda(), _dev(excl), max_range)
    msg = A.mismatch(got, want)
    assert msg is None, f"{name}: {msg}"


# ---- c. the tiled path with exclusions ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,R,D,k", A.TILED_SHAPES)
def test_tiled_exclusions(lib, B, R, D, k):
    Q, X, s16 = N.exact_case(B, R, D, k, seed=B + R + D)
    Qd, Xd = Q.cuda(), X.cuda()
    for cut in (2, 3):
        excl = A.tiled_tables(B, R, k, cut)
        ranges = N.range_table(B, R, k, cut)
        for rng in (None, ranges):
            want = A.expected(s16, k, rng, excl)
            for s in N.slices_for(R):
                msg = A.mismatch(hook(lib, Qd, Xd, k, 0, _dev(rng), excl.cuda(), 0, s), want)
                assert msg is None, f"boundary of {cut} slices, ranges {'NULL' if rng is None else 'given'}, slices = {s}: {msg}"
    excl = A.class_tables(B, R)
    want = A.expected(s16, k, None, excl)
    assert all(not (int(excl[b, 0]) <= r < int(excl[b, 1])) for b in range(B) for r in want[1][b].tolist())
    for s in N.slices_for(R):
        msg = A.mismatch(hook(lib, Qd, Xd, k, 0, None, excl.cuda(), 0, s), want)
        assert msg is None, f"ranges NULL, a class left out, slices = {s}: {msg}"
    # exclude = NULL through the new entry is ovmr_nearest_rows
    msg = A.mismatch(hook(lib, Qd, Xd, k, 0, None, None, 0, 2), N.expected(s16, k))
    assert msg is None, f"no exclusion: {msg}"


# ---- d. both paths on one case --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,k", [(128, 5), (512, 32)])
def test_both_paths_agree_on_exact_operands(lib, D, k):
    B, R, max_range = 70, 1000, 64
    Q, X, s16 = N.exact_case(B, R, D, k, seed=D + k)
    ranges, excl = A.short_tables(B, R, k, max_range, seed=3)
    ranges[:, 1] = torch.minimum(ranges[:, 1], ranges[:, 0] + max_range)      # nothing for the short path to truncate
    want = A.expected(s16, k, ranges, excl)
    short = hook(lib, Q.cuda(), X.cuda(), k, 1, ranges.cuda(), excl.cuda(), max_range)
    tiled = hook(lib, Q.cuda(), X.cuda(), k, 0, ranges.cuda(), excl.cuda(), 0, 3)
    assert A.mismatch(short, want) is None and A.mismatch(tiled, want) is None
    assert torch.equal(short[1], tiled[1]) and P.same_bits(short[0], tiled[0]) is None


@pytest.mark.parametrize("D,k", [(512, 5), (128, 32), (1024, 5), (64, 5)])
def test_general_by_margin(lib, D, k):
    Q, X = N.general_case(D, seed=D + k)
    B = Q.shape[0]
    cls = torch.arange(B) % 50
    ranges = torch.stack([cls * 20, cls * 20 + 20], 1).to(torch.int32)
    me = torch.stack([cls * 20 + 7, cls * 20 + 8], 1).to(torch.int32)
    Qd, Xd = Q.cuda(), X.cuda()
    msg = A.margin_mismatch(hook(lib, Qd, Xd, k, 1, ranges.cuda(), me.cuda(), 20), Q, X, k, ranges, me, 20)
    assert msg is None, f"short path: {msg}"
    msg = A.margin_mismatch(hook(lib, Qd, Xd, k, 0, ranges.cuda(), me.cuda(), 0, 2), Q, X, k, ranges, me)
    assert msg is None, f"tiled path, one class: {msg}"
    msg = A.margin_mismatch(hook(lib, Qd, Xd, k, 0, None, ranges.cuda(), 0, 2), Q, X, k, None, ranges)
    assert msg is None, f"tiled path, everything but one class: {msg}"


def test_short_score_does_not_depend_on_position_or_company(lib):
    """General operands: the score of a (query, row) pair is the same bits whatever the row's place in its range, the trip length
    (max_range 16 / 32 / 64 pick different kernels) and the queries that share the workgroup."""
    D, k = 512, 1
    Q, X = N.general_case(D, seed=5, classes=10, per_class=20, B=8)
    Qd, Xd = Q.cuda(), X.cuda()
    row = 77
    seen = set()
    for lo, n, max_range in ((77, 1, 16), (70, 16, 16), (62, 16, 30), (50, 30, 30), (14, 64, 64), (0, 130, 200), (77, 3, 4096)):
        for b in (0, 3, 5):                                       # the query sits in wave 0, 3 and in a workgroup's second block
            q = Qd[:1].repeat(b + 1, 1)
            q[:b] = Qd[1:b + 1]
            ranges = torch.tensor([[lo, lo + n]] * (b + 1), dtype=torch.int32)
            excl = torch.tensor([[lo, row]] * (b + 1), dtype=torch.int32)      # everything before the row: it is the first candidate
            ranges[:, 1] = row + 1
            v, i = hook(lib, q, Xd, k, 1, ranges.cuda(), excl.cuda(), max_range)
            assert int(i[b, 0]) == row
            seen.add(int(v[b, 0].view(torch.int32)))
    assert len(seen) == 1, f"the score of one pair took {len(seen)} values"


# ---- e. the production entry ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,R,D,k,max_range", [(5, 300, 512, 5, 64), (257, 400, 64, 32, 130), (66, 1000, 128, 5, 0)])
def test_production_entry_equals_hook(lib, B, R, D, k, max_range):
    from ovmr_amd import runtime
    Q, X, s16 = N.exact_case(B, R, D, k, seed=B + R)
    Qd, Xd = Q.cuda(), X.cuda()
    if max_range:
        ranges, excl = A.short_tables(B, R, k, max_range, seed=1)
        assert lib.ovmr_neighbours_scratch_bytes(B, R, k, max_range) == 0
        want = hook(lib, Qd, Xd, k, 1, ranges.cuda(), excl.cuda(), max_range, no_scratch=True)       # scratch = NULL
        got = runtime.neighbour_rows(Qd, Xd, k, ranges.cuda(), excl.cuda(), max_range)
    else:
        ranges, excl = N.range_table(B, R, k), A.tiled_tables(B, R, k)
        need = lib.ovmr_neighbours_scratch_bytes(B, R, k, 0)
        assert need == lib.ovmr_nearest_scratch_bytes(B, R, k) and need % (B * k * 8) == 0
        want = hook(lib, Qd, Xd, k, 0, ranges.cuda(), excl.cuda(), 0, need // (B * k * 8))
        with pytest.raises(ValueError, match="neighbour_rows: exclude must be row bounds"):
            runtime.neighbour_rows(Qd, Xd, k, ranges, excl)       # host tables are checked: the unclamped ones are refused
        got = runtime.neighbour_rows(Qd, Xd, k, ranges, excl.clamp(0, R))     # ... and copied
    assert torch.equal(got[1], want[1]) and P.same_bits(got[0], want[0]) is None
    assert A.mismatch(got, A.expected(s16, k, ranges, excl, max_range)) is None


def test_existing_entry_is_unchanged_by_the_new_one(lib):
    from ovmr_amd import runtime
    B, R, D, k = 66, 1000, 128, 5
    Q, X, s16 = N.exact_case(B, R, D, k, seed=4)
    ranges = N.range_table(B, R, k)
    old = runtime.nearest_rows(Q.cuda(), X.cuda(), k, ranges)
    new = runtime.neighbour_rows(Q.cuda(), X.cuda(), k, ranges)
    assert torch.equal(old[1], new[1]) and P.same_bits(old[0], new[0]) is None and N.mismatch(old, N.expected(s16, k, ranges)) is None


# ---- f. past 2^31 bytes -------------------------------------------------------------------------------------------------------------------------

def test_short_range_beyond_2_31_bytes(lib):
    k = 5
    Q, planted = N.big_bank_plan(k)
    X = N.big_bank_fill(torch.zeros((N.BIG_R, N.BIG_D), dtype=torch.float16, device="cuda"), planted)
    assert X.numel() * 2 > 2 ** 31
    first_past = 2 ** 31 // (2 * N.BIG_D)
    B = Q.shape[0]
    lo, hi = N.BIG_R - 230, N.BIG_R                               # every row of the range lies past 2^31 bytes
    assert lo > first_past
    ranges = torch.tensor([[lo, hi]] * B, dtype=torch.int32)
    excl = torch.tensor([[0, 0], [N.BIG_R - 1, N.BIG_R], [N.BIG_R - 200, N.BIG_R - 76]], dtype=torch.int32)
    # the expectation from the planted rows alone: their scores, +0 for every other row of the range
    s = torch.zeros((B, hi - lo), dtype=torch.float16)
    for r, (x0, x1) in planted.items():
        if lo <= r < hi:
            s[:, r - lo] = (Q[:, 0].double() * x0 + Q[:, 1].double() * x1).half()
    want_v, want_i = A.expected(s, k, None, excl - lo)
    want = (want_v, torch.where(want_i >= 0, want_i + lo, want_i))
    assert want[1][0, 0] == N.BIG_R - 1 and want[1][1, 0] != N.BIG_R - 1 and N.BIG_R - 77 not in want[1][0].tolist()
    got = hook(lib, Q.cuda(), X, k, 1, ranges.cuda(), excl.cuda(), 230)
    msg = A.mismatch(got, want)
    assert msg is None, msg
    del X


# ---- g. poisoned scratch, guarded operands ----------------------------------------------------------------------------------------------------------

def test_scratch_contents_do_not_matter_and_guards_survive(lib):
    B, R, D, k, max_range = 66, 1000, 128, 5, 64
    Q, X, s16 = N.exact_case(B, R, D, k, seed=1)
    ranges, excl = A.short_tables(B, R, k, max_range, seed=2)
    want_short = A.expected(s16, k, ranges, excl, max_range)
    want_tiled = A.expected(s16, k, ranges, excl)
    first = {}
    for fill in P.FILLS:
        arena = P.Arena(fill, device="cuda")
        Qd, Xd = arena.place(Q), arena.place(X)
        rd, xd = arena.place(ranges), arena.place(excl)
        values = arena.take(B * k, "f32").view(B, k)
        indices = arena.take(B * k, "i32").view(B, k)
        for path, s, want in ((1, 1, want_short), (0, 1, want_tiled), (0, 4, want_tiled)):
            got = hook(lib, Qd, Xd, k, path, rd, xd, max_range if path else 0, s, fill=fill, out=(values, indices))
            torch.cuda.synchronize()
            assert arena.intact(), f"fill '{fill}', path {path}, slices = {s}: a guard was written to"
            msg = A.mismatch(got, want)
            assert msg is None, f"fill '{fill}', path {path}, slices = {s}: {msg}"
            if path not in first:
                first[path] = (got[0].clone(), got[1].clone())
            assert P.same_bits(got[0], first[path][0]) is None and torch.equal(got[1], first[path][1]), f"fill '{fill}', path {path}: other bits"


# ---- h. refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_argument_refusals_launch_nothing(lib):
    from ovmr_amd import runtime
    Q, X, _ = N.exact_case(4, 100, 128, 5, seed=1)
    Qd, Xd = Q.cuda(), X.cuda()
    values = torch.full((4, 5), 7.0, device="cuda")
    indices = torch.full((4, 5), 7, dtype=torch.int32, device="cuda")
    ranges = torch.tensor([[0, 10]] * 4, dtype=torch.int32, device="cuda")
    scratch = torch.empty(1 << 16, dtype=torch.int64, device="cuda")

    def call(max_range, rng, path=None, excl=None):
        if path is None:
            return lib.ovmr_neighbours_rows(_p(Qd), 4, _p(Xd), 100, 128, 5, _p(rng), _p(excl), max_range, _p(values), _p(indices), _p(scratch),
                                            scratch.numel() * 8, _stream())
        return lib.ovmr_debug_neighbours_rows(_p(Qd), 4, _p(Xd), 100, 128, 5, _p(rng), _p(excl), max_range, _p(values), _p(indices), _p(scratch),
                                              scratch.numel() * 8, path, 1, _stream())

    assert call(16, None) == -1 and call(4097, ranges) == -1 and call(-1, ranges) == -1
    assert call(16, ranges, path=2) == -1 and call(0, ranges, path=1) == -1 and call(16, None, path=1) == -1
    assert call(16, ranges, excl=ctypes.c_void_p(ranges.data_ptr() + 2)) == -1
    torch.cuda.synchronize()
    assert bool((values == 7.0).all()) and bool((indices == 7).all()), "a refused call wrote its outputs"
    with pytest.raises(ValueError, match="neighbour_rows: ranges must be"):
        runtime.neighbour_rows(Qd, Xd, 5, torch.tensor([[0, 20]] * 4), None, 16)
    with pytest.raises(ValueError, match="neighbour_rows: exclude must be"):
        runtime.neighbour_rows(Qd, Xd, 5, None, torch.tensor([[0, 101]] * 4))
    assert call(16, ranges) == 0 and call(0, None) == 0
