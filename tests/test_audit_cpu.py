"""The bank audit without a GPU: the expectations of audit_cases.py against a brute-force loop, the comparators against the defects they are
there for (each on a named case), the header include/ovmr_hip_audit.h against runtime.AUDIT_SIGNATURES and the cross-compiled library's
exports, the pure entry point and the argument errors of the C ABI, the Python boundary of runtime.neighbour_rows on a recording
stand-in, the runner's tables and refusals."""
import contextlib
import csv
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import audit_cases as A
import nearest_cases as N
from conftest import REPO


# ---- the expectation -------------------------------------------------------------------------------------------------------------

def test_expected_equals_brute_force():
    s = torch.tensor([[0.5, -0.0, 0.0, float("nan"), 0.5, float("inf"), -float("inf"), 0.25, float("nan"), -1.0],
                      [0.0, 0.0, -0.0, 0.0, -0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                      [-2.0, -1.0, -1.0, -3.0, -1.0, -2.0, -1.0, -9.0, -1.0, -1.0]], dtype=torch.float16)
    ranges = torch.tensor([[0, 10], [2, 9], [-4, 30]], dtype=torch.int32)
    excl = torch.tensor([[3, 4], [0, 5], [8, 2]], dtype=torch.int32)
    for k in (1, 3, 10):
        for r, x, m in ((None, None, 0), (ranges, excl, 0), (None, excl, 0), (ranges, excl, 4), (ranges, None, 1)):
            assert A.mismatch(A.expected(s, k, r, x, m), A.brute_force(s, k, r, x, m)) is None, (k, m)
    v, i = A.expected(s, 3, ranges, excl)
    assert i.tolist() == [[8, 5, 0], [5, 6, 7], [1, 2, 4]], "row 3 (a NaN) is excluded; [8, 2) clamps to an empty exclusion"
    assert A.expected(s, 4, ranges, excl, 4)[1].tolist() == [[0, 1, 2, -1], [5, -1, -1, -1], [1, 2, 0, 3]], "max_range = 4 cuts the range, not the exclusion"
    assert A.expected(s, 2, None, torch.tensor([[0, 10]] * 3, dtype=torch.int32))[1].tolist() == [[-1, -1]] * 3
    for shape in A.SHORT_SHAPES[:5]:
        B, R, D, k, m = shape
        Q, X, s16 = N.exact_case(min(B, 40), R, D, k, 1)
        r, x = A.short_tables(min(B, 40), R, k, m, seed=2)
        assert A.mismatch(A.expected(s16, k, r, x, m), A.brute_force(s16, k, r, x, m)) is None
        assert A.mismatch(A.simulate(s16, k, r, x, m), A.expected(s16, k, r, x, m)) is None


def test_case_tables_cover_the_issue():
    Bs, Ds, ks = ({s[i] for s in A.SHORT_SHAPES} for i in (0, 2, 3))
    assert {1, 3, 4, 5, 257} <= Bs and {64, 128, 512, 768, 1024} <= Ds and {1, 5, 32} <= ks
    assert {0, 1, 4, 5, 7, 8, 9, 63, 64, 65, 129} <= set(A.short_lengths(5)) and 31 in A.short_lengths(32)
    assert {s[1] for s in A.TILED_SHAPES} == {257, 1000, 70001}
    r, x = A.short_tables(257, 400, 5, 130, seed=1)
    lens = (r[:, 1] - r[:, 0]).tolist()
    assert 130 in lens and 133 in lens and 0 in lens and 129 in lens and any(n < 0 for n in lens), "exactly max_range, max_range + 3, an unclamped range"
    assert int(r[:, 0].min()) == 0 and int(r[:, 1].max()) == 400
    assert int(x[:, 0].min()) < 0 and int(x[:, 1].max()) > 400 and bool((x[:, 1] < x[:, 0]).any()), "unclamped exclusions"
    covered = sum(1 for b in range(257) if lens[b] > 0 and int(x[b, 0]) <= int(r[b, 0]) and int(x[b, 1]) >= int(r[b, 1]))
    assert covered > 5
    t = A.tiled_tables(66, 1000, 5, 2)
    kinds = {tuple(p) for p in t.tolist()}
    assert (247, 263) in kinds and (507, 523) in kinds and (0, 256) in kinds and (0, 1000) in kinds
    c = A.class_tables(33, 70001)
    assert bool(((c[:, 1] - c[:, 0]) == 16).all())


# ---- the comparators reject what they are there for ----------------------------------------------------------------------------------

def _planted():
    k = 5
    Q, X, s16, ranges = A.planted_short_case(k)
    me = torch.tensor([[110, 111], [131, 132], [150, 151], [100, 101], [169, 170], [131, 132]], dtype=torch.int32)
    return k, s16, ranges, me


def test_rejects_self_not_excluded_and_an_inclusive_exclusion_end():
    """Queries 0 .. 2 each ARE one of the three equal best rows 110, 131, 150 (as an audit queries a bank with its own rows)."""
    k, s16, ranges, me = _planted()
    want = A.expected(s16, k, ranges, me)
    assert want[1][0, :2].tolist() == [131, 150] and want[1][1, :2].tolist() == [110, 150]
    assert A.mismatch(A.simulate(s16, k, ranges, me), want) is None
    assert "expected row 131" in A.mismatch(A.simulate(s16, k, ranges, me, defect="self_included"), want)
    # row 131 is excluded, row 132 is not: an inclusive end loses it only where it would be listed -- plant it
    x = torch.tensor([[109, 110]] * 6, dtype=torch.int32)
    want = A.expected(s16, k, ranges, x)
    assert want[1][0, 0] == 110
    assert A.mismatch(A.simulate(s16, k, ranges, x, defect="excl_inclusive"), want) is not None


def test_rejects_an_exclusion_applied_to_the_position_in_the_range():
    k, s16, ranges, me = _planted()
    want = A.expected(s16, k, ranges, me)
    got = A.simulate(s16, k, ranges, me, defect="excl_position")
    assert got[1][0, 0] == 110 and A.mismatch(got, want) is not None
    # the defect and the clean model agree where the range starts at row 0
    r0 = torch.tensor([[0, 70]] * 6, dtype=torch.int32)
    x0 = torch.tensor([[3, 9]] * 6, dtype=torch.int32)
    assert A.mismatch(A.simulate(s16, k, r0, x0, defect="excl_position"), A.expected(s16, k, r0, x0)) is None


def test_rejects_a_range_cut_at_a_pass_or_a_trip():
    """One of the three equal best rows, 150, sits in the last, partial pass of its range: [100, 151) ends three rows into an 8-row pass,
    [86, 151) one row into its second 64-row trip."""
    k, s16, ranges, me = _planted()
    r = torch.tensor([[100, 151]] * 6, dtype=torch.int32)
    want = A.expected(s16, k, r, None)
    assert 150 in want[1][0].tolist()
    assert A.mismatch(A.simulate(s16, k, r, None, defect="cut_8"), want) is not None
    r = torch.tensor([[86, 151]] * 6, dtype=torch.int32)      # 65 rows: the row of the second trip is the third of the equal rows
    want = A.expected(s16, k, r, None)
    assert want[1][0, :3].tolist() == [110, 131, 150]
    assert A.mismatch(A.simulate(s16, k, r, None, defect="cut_64"), want) is not None
    assert A.mismatch(A.simulate(s16, k, r, None), want) is None


def test_rejects_ties_to_the_higher_row_the_unrounded_score_and_a_zero_tail():
    k, s16, ranges, me = _planted()
    want = A.expected(s16, 2, ranges, me)
    assert want[1][5].tolist() == [110, 150], "the cut at k = 2 is decided by the tie: 110 and 150 of the two that are left"
    assert "expected row 110" in A.mismatch(A.simulate(s16, 2, ranges, None, defect="ties_high"), A.expected(s16, 2, ranges, None))
    Q = torch.zeros((1, 64), dtype=torch.float16)
    Q[0, 0], Q[0, 1] = 1 + 2.0 ** -10, 1.0
    X = torch.zeros((8, 64), dtype=torch.float16)
    X[1, 0] = 1.0
    X[4, 0], X[4, 1] = 1.0, 2.0 ** -14
    s32, s = (Q.double() @ X.double().t()).float(), N.scores16(Q, X)
    r, x = torch.tensor([[0, 8]], dtype=torch.int32), torch.tensor([[2, 3]], dtype=torch.int32)
    want = A.expected(s, 2, r, x, 8)
    assert want[1].tolist() == [[1, 4]]
    assert A.mismatch(A.simulate(s, 2, r, x, 8, s32=s32), want) is None
    assert A.mismatch(A.simulate(s, 2, r, x, 8, "unrounded", s32=s32), want) is not None
    covered = torch.tensor([[100, 170]] * 6, dtype=torch.int32)
    want = A.expected(s16, k, ranges, covered)
    assert bool((want[1] == -1).all()) and bool(torch.isinf(want[0]).all())
    assert A.mismatch(A.simulate(s16, k, ranges, covered, defect="tail_zero"), want) is not None
    assert A.mismatch(A.expected(s16, k, ranges, covered, tail_index=0), want) is not None


def test_rejects_a_missing_truncation():
    """The range is three rows longer than max_range and the best row is among the three."""
    k, s16, ranges, me = _planted()
    r = torch.tensor([[100, 151]] * 6, dtype=torch.int32)
    want = A.expected(s16, k, r, None, 48)
    assert 150 not in want[1][0].tolist() and want[1][0, :2].tolist() == [110, 131]
    assert A.mismatch(A.simulate(s16, k, r, None, 48), want) is None
    assert A.mismatch(A.simulate(s16, k, r, None, 48, defect="no_truncation"), want) is not None


def test_margin_comparator():
    Q, X = N.general_case(128, 4, classes=10, per_class=6, B=12)
    s16 = N.scores16(Q, X)
    k = 4
    cls = torch.arange(12) % 10
    own = torch.stack([cls * 6, cls * 6 + 6], 1).to(torch.int32)
    me = torch.stack([cls * 6 + 2, cls * 6 + 3], 1).to(torch.int32)
    for r, x in ((own, me), (None, own)):
        good = A.expected(s16, k, r, x)
        assert A.margin_mismatch(good, Q, X, k, r, x) is None
        assert A.margin_mismatch(A.expected(s16, k, r, None), Q, X, k, r, x) is not None, "a list that ignores the exclusion"
    good = A.expected(s16, k, own, me)
    v = good[0].clone()
    v[:, 1] += 0.01
    assert "from its row's score" in A.margin_mismatch((v, good[1]), Q, X, k, own, me)


# ---- audit_bank's expectation ------------------------------------------------------------------------------------------------------------

def test_audit_expectation_and_its_two_defects():
    for lens in A.PLANTS:
        X, starts, s16 = A.audit_bank_case(128, lens)
        want = A.expected_audit(s16, starts, 3)
        rows = A.plant_rows(lens)
        a, b, c = rows["equal_in"]
        assert not bool(want["suspect"][a]) and int(want["duplicate_of"][a]) == b and bool(want["suspect"][c])
        a, b, c = rows["equal_out"]
        assert not bool(want["suspect"][a]) and int(want["duplicate_of"][a]) == c and int(want["duplicate_of"][b]) == c
        assert A.audit_mismatch(want, want) is None
        assert "suspect" in A.audit_mismatch(A.expected_audit(s16, starts, 3, defect="suspect_ge"), want)
        assert "duplicate_of" in A.audit_mismatch(A.expected_audit(s16, starts, 3, defect="dup_high_row"), want)
        for c, n in enumerate(lens):
            if n == 1:
                assert int(want["in_row"][starts[c], 0]) == -1 and not bool(want["suspect"][starts[c]]), "a class of one image is never suspect"
        sub = A.expected_audit(s16, starts, 3, classes=[4, 2])
        keep = torch.cat([torch.arange(starts[2], starts[3]), torch.arange(starts[4], starts[5])])
        assert torch.equal(sub["rows"], keep) and torch.equal(sub["out_row"], want["out_row"][keep]) and torch.equal(sub["suspect"], want["suspect"][keep])
        at, above = A.expected_audit(s16, starts, 3, dup_threshold=A.NEAR), A.expected_audit(s16, starts, 3, dup_threshold=A.NEAR + 2.0 ** -11)
        src, dst = rows["near"]
        assert int(at["duplicate_of"][dst]) == src and int(above["duplicate_of"][dst]) == -1
    nan = torch.tensor([float("nan"), 1.0, float("nan"), -0.0])
    other = torch.tensor([1.0, float("nan"), float("nan"), 0.0])
    assert A.value_gt(nan, other).tolist() == [True, False, False, False]


def test_default_threshold_finds_every_byte_identical_copy():
    """An fp16 L2-normalised row scores itself at least (1 - 2^-11)^2 rounded to fp16 -- 0.9990 -- over D = 64 .. 1024, spiky rows included."""
    g = torch.Generator().manual_seed(3)
    low = 1.0
    for D in (64, 128, 512, 768, 1024):
        x = torch.randn((200, D), generator=g)
        x[:50] *= torch.rand((50, D), generator=g) ** 8           # spiky rows
        x[50:60, 1:] *= 1e-3
        x = torch.nn.functional.normalize(x, dim=1).half()
        s = (x.double() * x.double()).sum(1).half().float()
        low = min(low, float(s.min()))
    assert low >= 0.9990 > 0.995


# ---- the header, its table and the library ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import build, runtime
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    return runtime.load_library()


def test_audit_header_table_and_exports(lib):
    from ovmr_amd import build, runtime
    text = open(os.path.join(REPO, "include", "ovmr_hip_audit.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = dict(re.findall(r"\b(ovmr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(decls) == set(runtime.AUDIT_SIGNATURES) == {"ovmr_neighbours_scratch_bytes", "ovmr_neighbours_rows", "ovmr_debug_neighbours_rows"}
    assert not set(runtime.AUDIT_SIGNATURES) & (set(runtime.SIGNATURES) | set(runtime.EXT_SIGNATURES))
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long}
    for name, params in decls.items():
        res, args = runtime.AUDIT_SIGNATURES[name]
        assert hasattr(lib, name), f"{name} declared in include/ovmr_hip_audit.h but not exported"
        want = [ctypes.c_void_p if "*" in p or "ovmr_stream" in p else ctype[p.split()[0]] for p in (q.strip() for q in params.split(","))]
        assert args == want, f"{name}: {args} != {want}"
        assert res is (ctypes.c_long if name == "ovmr_neighbours_scratch_bytes" else ctypes.c_int)
        assert getattr(lib, name).argtypes == args
    assert text.count("No counterpart in the reference") == 3
    assert "ovmr_hip_audit.h" in inspect.getsource(build.build), "the build lists the header among its dependencies"
    for other in ("ovmr_hip.h", "ovmr_hip_nearest.h"):
        assert "neighbours" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", other)).read(), flags=re.S)


def test_scratch_bytes_and_argument_errors(lib):
    f, g = lib.ovmr_neighbours_scratch_bytes, lib.ovmr_nearest_scratch_bytes
    for B, R, k in ((1, 1, 1), (256, 640000, 32), (1280, 640000, 5), (130, 70001, 31), (0, 5, 1)):
        assert f(B, R, k, 0) == g(B, R, k)
        for m in (1, 16, 64, 4096):
            assert f(B, R, k, m) == 0, "the short launch needs no scratch"
    for B, R, k, m in ((-1, 5, 1, 0), (4, 0, 1, 8), (4, 2 ** 32 - 1, 1, 0), (4, 5, 0, 8), (4, 5, 33, 0), (4, 5, 1, -1), (4, 5, 1, 4097)):
        assert f(B, R, k, m) == -1
    E_ARG = -1
    q, x, v, i, s, r, e = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000))   # never dereferenced
    ok = dict(q=q, B=4, x=x, R=100, D=128, k=5, ranges=r, excl=e, m=16, v=v, i=i, s=None, n=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ovmr_neighbours_rows(a["q"], a["B"], a["x"], a["R"], a["D"], a["k"], a["ranges"], a["excl"], a["m"], a["v"], a["i"], a["s"], a["n"], None)

    tiled = dict(m=0, s=s, n=1 << 20)
    for kw in (dict(q=None), dict(x=None), dict(v=None), dict(i=None), dict(ranges=None), dict(q=ctypes.c_void_p(0x10008)), dict(x=ctypes.c_void_p(0x20002)),
               dict(v=ctypes.c_void_p(0x30002)), dict(ranges=ctypes.c_void_p(0x60001)), dict(excl=ctypes.c_void_p(0x70002)), dict(D=0), dict(D=96), dict(D=1088),
               dict(k=0), dict(k=33), dict(k=101), dict(R=0), dict(R=2 ** 32 - 1), dict(B=-1), dict(m=-1), dict(m=4097),
               dict(tiled, s=None), dict(tiled, n=4 * 5 * 8 - 1), dict(tiled, n=-1), dict(tiled, s=ctypes.c_void_p(0x50004)), dict(tiled, excl=ctypes.c_void_p(0x70002)),
               dict(tiled, q=None), dict(tiled, D=96)):
        assert call(**kw) == E_ARG, kw
    assert call(B=0) == 0 and call(B=0, q=None, v=None, i=None) == 0 and call(B=0, **tiled) == 0
    assert call(B=0, ranges=None) == E_ARG, "max_range > 0 needs ranges, whatever B"
    hook = lib.ovmr_debug_neighbours_rows
    assert hook(q, 4, x, 100, 128, 5, r, e, 16, v, i, None, 0, 2, 1, None) == E_ARG
    assert hook(q, 4, x, 100, 128, 5, r, e, 0, v, i, None, 0, 1, 1, None) == E_ARG
    assert hook(q, 4, x, 100, 128, 5, None, e, 16, v, i, None, 0, 1, 1, None) == E_ARG
    assert hook(q, 4, x, 100, 128, 5, r, e, 0, v, i, s, 1 << 20, 0, 0, None) == E_ARG
    assert hook(q, 4, x, 100, 128, 5, r, e, 0, v, i, s, 4 * 3 * 5 * 8 - 1, 0, 3, None) == E_ARG
    assert hook(q, 0, x, 100, 128, 5, r, e, 16, v, i, None, 0, 1, 1, None) == 0


# ---- the Python boundary of runtime.neighbour_rows ---------------------------------------------------------------------------------------------

class _Recorder:
    """Stands where the library stands: records every call and says yes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ovmr_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if name == "ovmr_neighbours_scratch_bytes":
                return 0 if args[3] else 8 * 1024
            return 0
        return call


@pytest.fixture
def stub(monkeypatch):
    from ovmr_amd import runtime
    rec, log = _Recorder(), []
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    monkeypatch.setattr(runtime, "_same_device", lambda a, b: True)
    monkeypatch.setattr(runtime, "_nearest_scratch", {})
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: (log.append("stream"), SimpleNamespace(cuda_stream=0))[1])
    return SimpleNamespace(rec=rec, log=log, call=runtime.neighbour_rows, scratch=runtime._nearest_scratch)


def _ops(B=5, R=40, D=128):
    return dict(queries=torch.zeros((B, D), dtype=torch.float16), bank=torch.zeros((R, D), dtype=torch.float16), k=3)


_PAIRS = torch.tensor([[0, 3]] * 5, dtype=torch.int32)

VIOLATIONS = [
    ("queries", "three dimensions", lambda o: o.update(queries=torch.zeros((5, 2, 64), dtype=torch.float16))),
    ("queries", "fp32", lambda o: o.update(queries=o["queries"].float())),
    ("queries", "a numpy array", lambda o: o.update(queries=np.zeros((5, 128), dtype=np.float16))),
    ("queries", "width 96", lambda o: o.update(queries=torch.zeros((5, 96), dtype=torch.float16), bank=torch.zeros((40, 96), dtype=torch.float16))),
    ("bank", "another width", lambda o: o.update(bank=torch.zeros((40, 64), dtype=torch.float16))),
    ("bank", "fp32", lambda o: o.update(bank=o["bank"].float())),
    ("k", "zero", lambda o: o.update(k=0)),
    ("k", "33", lambda o: o.update(k=33, bank=torch.zeros((64, 128), dtype=torch.float16))),
    ("k", "more than the bank's rows", lambda o: o.update(k=5, bank=torch.zeros((4, 128), dtype=torch.float16))),
    ("k", "a float", lambda o: o.update(k=2.0)),
    ("ranges", "shape [B, 3]", lambda o: o.update(ranges=torch.zeros((5, 3), dtype=torch.int32))),
    ("ranges", "floating point", lambda o: o.update(ranges=torch.zeros((5, 2)))),
    ("ranges", "negative lo (host)", lambda o: o.update(ranges=torch.tensor([[0, 3]] * 4 + [[-1, 3]], dtype=torch.int64))),
    ("ranges", "hi beyond R (host)", lambda o: o.update(ranges=torch.tensor([[0, 3]] * 4 + [[2, 41]], dtype=torch.int32))),
    ("ranges", "lo above hi (host)", lambda o: o.update(ranges=torch.tensor([[0, 3]] * 4 + [[7, 6]], dtype=torch.int32))),
    ("ranges", "missing with max_range > 0", lambda o: o.update(max_range=16)),
    ("ranges", "longer than max_range (host)", lambda o: o.update(max_range=8, ranges=torch.tensor([[0, 3]] * 4 + [[2, 11]], dtype=torch.int32))),
    ("exclude", "shape [B, 3]", lambda o: o.update(exclude=torch.zeros((5, 3), dtype=torch.int32))),
    ("exclude", "a row short", lambda o: o.update(exclude=torch.zeros((4, 2), dtype=torch.int32))),
    ("exclude", "bool", lambda o: o.update(exclude=torch.zeros((5, 2), dtype=torch.bool))),
    ("exclude", "negative lo (host)", lambda o: o.update(exclude=np.array([[0, 3]] * 4 + [[-1, 3]]))),
    ("exclude", "hi beyond R (host)", lambda o: o.update(exclude=torch.tensor([[0, 3]] * 4 + [[2, 41]], dtype=torch.int32))),
    ("exclude", "lo above hi (host)", lambda o: o.update(exclude=torch.tensor([[0, 3]] * 4 + [[7, 6]], dtype=torch.int32))),
    ("max_range", "negative", lambda o: o.update(max_range=-1, ranges=_PAIRS)),
    ("max_range", "4097", lambda o: o.update(max_range=4097, ranges=_PAIRS)),
    ("max_range", "a float", lambda o: o.update(max_range=16.0, ranges=_PAIRS)),
    ("max_range", "a bool", lambda o: o.update(max_range=True, ranges=_PAIRS)),
    ("out", "not a pair", lambda o: o.update(out=torch.zeros((5, 3)))),
    ("out[0]", "fp16 values", lambda o: o.update(out=(torch.zeros((5, 3), dtype=torch.float16), torch.zeros((5, 3), dtype=torch.int32)))),
    ("out[1]", "another k", lambda o: o.update(out=(torch.zeros((5, 3)), torch.zeros((5, 4), dtype=torch.int32)))),
    ("out[0]", "strided", lambda o: o.update(out=(torch.zeros((5, 6))[:, ::2], torch.zeros((5, 3), dtype=torch.int32)))),
]


@pytest.mark.parametrize("arg,what,change", VIOLATIONS, ids=[f"{a}: {w}" for a, w, _ in VIOLATIONS])
def test_violation_is_refused_before_anything_reaches_the_library(arg, what, change, stub):
    ops = _ops()
    change(ops)
    with pytest.raises(ValueError) as err:
        stub.call(**ops)
    msg = str(err.value)
    assert msg.startswith("neighbour_rows: ") and re.search(rf"(?<![\w]){re.escape(arg)}(?![\w\[])", msg), msg
    assert "must be" in msg and "got" in msg, msg
    assert stub.rec.calls == [] and stub.log == [], (stub.rec.calls, stub.log)


def test_device_mismatch_is_refused(monkeypatch):
    from ovmr_amd import runtime
    rec = _Recorder()
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    with pytest.raises(ValueError, match="neighbour_rows: queries must be on cuda"):
        runtime.neighbour_rows(**_ops())
    assert rec.calls == []


def test_accepted_calls_hand_over_what_the_header_asks(stub):
    ops = _ops()
    wide = torch.zeros((5, 256), dtype=torch.float16)
    ranges = np.array([[0, 16], [3, 3], [39, 40], [0, 1], [5, 9]], dtype=np.int64)
    excl = torch.tensor([[0, 40], [3, 3], [39, 40], [0, 1], [5, 9]], dtype=torch.int64)[:, [0, 1]]
    values, indices = stub.call(wide[:, ::2], ops["bank"], 3, ranges, excl, 16)
    assert values.shape == indices.shape == (5, 3) and values.dtype == torch.float32 and indices.dtype == torch.int32
    assert [n for n, _ in stub.rec.calls] == ["ovmr_neighbours_scratch_bytes", "ovmr_neighbours_rows"]
    assert stub.rec.calls[0][1] == (5, 40, 3, 16)
    a = stub.rec.calls[1][1]
    assert len(a) == 14 and (a[1], a[3], a[4], a[5], a[8]) == (5, 40, 128, 3, 16)
    assert a[0].value != wide.data_ptr(), "a strided view goes to the library as a dense copy"
    assert a[2].value == ops["bank"].data_ptr() and a[6].value is not None and a[7].value is not None
    assert a[9].value == values.data_ptr() and a[10].value == indices.data_ptr()
    assert a[11] is None and a[12] == 0 and stub.scratch == {}, "the short launch takes no scratch"
    stub.rec.calls.clear()                                  # max_range = 0: the tiled pair, with nearest_rows' cached scratch; operands may be absent
    out = (torch.zeros((5, 3)), torch.zeros((5, 3), dtype=torch.int32))
    res = stub.call(ops["queries"], ops["bank"], 3, exclude=excl, out=out)
    a = stub.rec.calls[1][1]
    assert res[0] is out[0] and res[1] is out[1] and a[6] is None and a[7].value is not None and a[8] == 0 and a[11].value is not None and a[12] >= 8 * 1024
    first = a[11].value
    stub.rec.calls.clear()
    stub.call(ops["queries"], ops["bank"], 3)
    a = stub.rec.calls[1][1]
    assert a[6] is None and a[7] is None and a[11].value == first, "the scratch buffer is reused"
    stub.rec.calls.clear()                                  # an empty batch launches nothing
    v, i = stub.call(torch.zeros((0, 128), dtype=torch.float16), ops["bank"], 3)
    assert v.shape == (0, 3) and stub.rec.calls == []


# ---- the model, the trainer and the runner -----------------------------------------------------------------------------------------------------

def test_trainer_and_model_share_the_signature():
    from ovmr_amd import modules, trainer
    a, b = inspect.signature(modules.CustomCLIP.audit_bank), inspect.signature(trainer.MM_CLS_OP.audit_bank)
    assert [(p.name, p.default) for p in a.parameters.values()] == [(p.name, p.default) for p in b.parameters.values()]
    assert [(p.name, p.default) for p in a.parameters.values()][1:] == [("k", 5), ("classes", None), ("dup_threshold", 0.995), ("batch", 1024)]


def test_model_refuses_in_one_line():
    from ovmr_amd import modules
    m = object.__new__(modules.CustomCLIP)
    m._dist, m.mm_classifier, m._has_features = None, None, False
    with pytest.raises(ValueError, match="audit_bank: the model has no classifiers yet") as err:
        m.audit_bank()
    m.mm_classifier = torch.zeros(1)
    with pytest.raises(ValueError, match="audit_bank: the model holds no exemplar features") as err:
        m.audit_bank()
    assert "\n" not in str(err.value)
    m._has_features = True
    for k in (0, 33, True, 1.5):
        with pytest.raises(ValueError, match=r"audit_bank: k must be an integer in \[1, 32\]"):
            m.audit_bank(k)


def test_audit_tables_and_files(tmp_path):
    from ovmr_amd import cli
    lens = (3, 1, 4, 2, 4, 1, 2, 4)
    X, starts, s16 = A.audit_bank_case(128, lens)
    audit = A.expected_audit(s16, starts, 2)
    names = ["cat", "dog, big", "emu", "fox", "gnu", "hen", "ibis", "jay"]
    paths = [f"bank/{i}.png" for i in range(sum(lens))]
    rows, neighbours, classes = cli.bank_audit_tables(audit, names, lens, paths)
    assert len(rows) == 21 and len(classes) == 8
    r = A.plant_rows(lens)["cross"][1]
    assert rows[r][:4] == (r, 4, "gnu", f"bank/{r}.png") and rows[r][6] == A.plant_rows(lens)["cross"][0] and rows[r][7:9] == (2, "emu")
    assert rows[r][9] == 1.0 and rows[r][10] == 1 and rows[r][11] == rows[r][6]
    assert rows[3][4:6] == (-1, -np.inf) and rows[3][10] == 0, "a class of one image: no class-mate, never suspect"
    assert classes[1] == (1, "dog, big", 1, 0, 0) and sum(c[3] for c in classes) == sum(x[10] for x in rows)
    assert sum(1 for n in neighbours if n[0] == 3 and n[1] == "in") == 0 and sum(1 for n in neighbours if n[0] == 3 and n[1] == "out") == 2
    cli.write_bank_audit(str(tmp_path / "deep"), (rows, neighbours, classes))
    for name, cols, n in zip(cli.AUDIT_FILES, (cli.AUDIT_COLUMNS, cli.AUDIT_NEIGHBOUR_COLUMNS, cli.AUDIT_CLASS_COLUMNS), (21, len(neighbours), 8)):
        lines = list(csv.reader(open(tmp_path / "deep" / name)))
        assert lines[0] == cols and len(lines) == 1 + n
    lines = list(csv.reader(open(tmp_path / "deep" / "bank_audit.csv")))
    assert lines[1 + r] == [str(r), "4", "gnu", f"bank/{r}.png", str(rows[r][4]), repr(rows[r][5]), str(rows[r][6]), "2", "emu", "1.0", "1", str(rows[r][6])]
    assert lines[4][4:6] == ["-1", "-inf"] and float(lines[4][5]) == -np.inf
    assert cli.AUDIT_COLUMNS == ["row", "label", "classname", "exemplar", "in_row", "in_similarity", "out_row", "out_label", "out_classname",
                                 "out_similarity", "suspect", "duplicate_of"]
    assert cli.bank_audit_tables(audit, names, lens)[0][0][3] == "", "a bank without paths: the column stays empty"


def test_runner_refusals():
    from ovmr_amd import cli
    w = ["--clip-weights", "clip.pt"]
    cli.check_audit(cli.parse(w + ["--audit-bank", "3"]), "MM_CLS_OP", False)
    cli.check_audit(cli.parse(w), "ZeroshotCLIP", True)                       # (no --audit-bank: nothing to refuse)
    assert cli.parse(w + ["--audit-bank"]).audit_bank == 5 and cli.parse(w + ["--audit-bank", "--dup-threshold", "0.9"]).dup_threshold == 0.9
    for argv, trainer, zeroshot, msg in (
            (w + ["--audit-bank", "3"], "ZeroshotCLIP", True, "--trainer ZeroshotCLIP has no exemplars to audit"),
            (w + ["--audit-bank", "3", "--classifiers", "mm_classifiers.pt"], "MM_CLS_OP", False, "holds no exemplar features"),
            (w + ["--audit-bank", "0"], "MM_CLS_OP", False, r"--audit-bank 0: K must lie in \[1, 32\]"),
            (w + ["--audit-bank", "33"], "MM_CLS_OP", False, r"--audit-bank 33: K must lie in \[1, 32\]"),
            (w + ["--audit-bank", "3", "--dup-threshold", "nan"], "MM_CLS_OP", False, "T must be a number"),
            (w + ["--dup-threshold", "0.9"], "MM_CLS_OP", False, "--dup-threshold T belongs to --audit-bank")):
        with pytest.raises(SystemExit, match=msg) as err:
            cli.check_audit(cli.parse(argv), trainer, zeroshot)
        assert "\n" not in str(err.value)


def test_help_says_what_nobody_has_measured(capsys):
    from ovmr_amd import cli
    with pytest.raises(SystemExit):
        cli.parse(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--audit-bank [K]" in text and "--dup-threshold T" in text and "nobody has measured on real images" in text
