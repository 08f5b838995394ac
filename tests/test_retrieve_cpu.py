"""Search by class without a GPU: the expectation of retrieve_cases.py against a brute-force loop, the comparator against the defects it
is there for (each on a named case; the honest model passes them all), the header include/ovmr_hip_retrieve.h against
runtime.RETRIEVE_SIGNATURES and the cross-compiled library's exports, the pure entry point and the argument errors of the C ABI (addresses
that are never dereferenced), the Python boundary of runtime.ColumnTopM on a recording stand-in."""
import contextlib
import ctypes
import inspect
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import retrieve_cases as R
from conftest import REPO

NAN, INF = float("nan"), float("inf")


# ---- the expectation -------------------------------------------------------------------------------------------------------------

def test_expected_equals_brute_force():
    s = torch.tensor([[0.5, 0.0, -2.0], [-0.0, 0.0, -1.0], [0.0, -0.0, -1.0], [NAN, 0.0, -3.0], [0.5, -0.0, -1.0], [INF, 0.0, -2.0],
                      [-INF, 0.0, -1.0], [0.25, 0.0, -9.0], [NAN, 0.0, -1.0], [-1.0, 0.0, -1.0]], dtype=torch.float16)
    floor = torch.tensor([-INF, 0.0, 0.0009765625, INF, NAN, 0.5, -INF, 0.25, -1.0, -1.0])
    for m in (1, 3, 10, 12):
        for f in (None, floor):
            for base in (0, 2 ** 31 - 3):
                assert R.mismatch(R.expected(s, m, f, base), R.brute_force(s, m, f, base)) is None, (m, base)
    v, i = R.expected(s, 4)
    assert i[0].tolist() == [3, 8, 5, 0] and i[1].tolist() == [0, 1, 2, 3] and i[2].tolist() == [1, 2, 4, 6]
    assert math.isnan(v[0, 0]) and v[0, 2] == INF
    v, i = R.expected(s, 4, floor)
    assert i[0].tolist() == [3, 8, 5, 0], "a NaN is above a floor of +inf (row 3); a NaN floor keeps 0.5 out (row 4); row 2 is a step below its floor"
    assert i[1].tolist() == [0, 1, 6, 8], "rows 2 (a step above 0), 3 (+inf), 4 (NaN), 5 (0.5), 7 (0.25) are out; row 1 equals its floor"
    assert R.expected(s[:2], 3)[1][0].tolist() == [0, 1, -1] and R.expected(s[:2], 3)[0][0, 2] == -INF
    for N, C in ((5, 3), (63, 7), (65, 17)):
        p = R.planted_pool(N, C)
        assert R.mismatch(R.expected(p, 5), R.brute_force(p, 5)) is None
        assert R.mismatch(R.expected(p, 5, R.floor_table(p)), R.brute_force(p, 5, R.floor_table(p))) is None


def test_planted_pool_holds_what_the_tests_lean_on():
    p = R.planted_pool(300, 130)
    want = R.expected(p, 2)
    assert want[1][0].tolist() == [3, 90], "three equal best values in three batches: the tie decides membership"
    assert R.expected(p, 5)[1][1].tolist() == [0, 1, 2, 3, 4] and bool((p[1::3, 1].view(torch.int16) == -32768).all()), "-0 among +0"
    assert want[1][2, 0] == 7 and math.isnan(want[0][2, 0]) and want[1][3, 0] == 70 and want[0][3, 0] == INF
    assert R.expected(p, 300)[1][3, -1] == 2 and want[1][4].tolist() == [299, 298] and want[1][5].tolist() == [0, 1]
    assert want[1][129].tolist() == [299, 298]
    f = R.floor_table(p)
    assert math.isnan(f[4]) and f[3] == INF and f[0] == -INF and f[1] == float(p[1, 1]) and f[7] > float(p[7, 7]) > f[7] - 0.01


# ---- the comparator rejects what it is there for ------------------------------------------------------------------------------------

CASES = {
    "ties across batches": dict(N=300, C=8, m=2, cuts=(64, 64, 64, 64, 44)),
    "one call": dict(N=300, C=8, m=5),
    "padded rows": dict(N=65, C=7, m=5, gap=3, cuts=(64, 1)),
    "partial class tile": dict(N=65, C=130, m=3, cuts=(1, 64)),
    "reversed batches": dict(N=300, C=8, m=32, cuts=(65, 235), reverse=True),
    "floor": dict(N=65, C=17, m=31, floor=True, cuts=(64, 1)),
    "short pool": dict(N=5, C=8, m=8, cuts=(2, 3)),
    "merge": dict(N=300, C=8, m=3, split=100, cuts=(65, 235)),
    "past 2^31": dict(N=8, C=8, m=5, base=2 ** 31 - 3),
    "the last images": dict(N=8, C=8, m=5, base=2 ** 32 - 1 - 8),
}
REJECTED_ON = {"ties_later": "ties across batches", "local_base": "ties across batches", "ld_C": "padded rows", "drop_row_chunk": "one call",
               "drop_class_tile": "partial class tile", "no_carry": "ties across batches", "floor_gt": "floor", "tail_zero": "short pool",
               "merge_drop_equal": "merge", "index31": "past 2^31"}


def _run(case, defect=None):
    kw = dict(CASES[case])
    p = R.planted_pool(kw.pop("N"), kw.pop("C"))
    m = kw.pop("m")
    floor = R.floor_table(p) if kw.pop("floor", False) else None
    base = kw.get("base", 0)
    return R.simulate(p, m, floor=floor, defect=defect, **kw), R.expected(p, m, floor, base)


@pytest.mark.parametrize("case", sorted(CASES))
def test_honest_model_passes(case):
    got, want = _run(case)
    assert R.mismatch(got, want) is None


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defect_is_rejected(defect):
    assert set(REJECTED_ON) == set(R.DEFECTS)
    got, want = _run(REJECTED_ON[defect], defect)
    assert R.mismatch(got, want) is not None, f"{defect} passes on {REJECTED_ON[defect]!r}"
    if defect == "ties_later":
        assert "expected image 90" in R.mismatch(got, want) or "expected image 3" in R.mismatch(got, want)
    if defect == "tail_zero":
        assert R.mismatch(R.expected(R.planted_pool(5, 8), 8, tail_index=0), want) is not None


# ---- the header, its table and the library ---------------------------------------------------------------------------------------------

NAMES = {"ovmr_retrieve_state_bytes", "ovmr_retrieve_reset", "ovmr_retrieve_update", "ovmr_retrieve_merge", "ovmr_retrieve_finish"}


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import build, runtime
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    return runtime.load_library()


def test_retrieve_header_table_and_exports(lib):
    from ovmr_amd import build, runtime
    text = open(os.path.join(REPO, "include", "ovmr_hip_retrieve.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = dict(re.findall(r"\b(ovmr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(decls) == set(runtime.RETRIEVE_SIGNATURES) == NAMES
    assert not set(runtime.RETRIEVE_SIGNATURES) & (set(runtime.SIGNATURES) | set(runtime.EXT_SIGNATURES) | set(runtime.AUDIT_SIGNATURES))
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long}
    for name, params in decls.items():
        res, args = runtime.RETRIEVE_SIGNATURES[name]
        assert hasattr(lib, name), f"{name} declared in include/ovmr_hip_retrieve.h but not exported"
        want = [ctypes.c_void_p if "*" in p or "ovmr_stream" in p else ctype[p.split()[0]] for p in (q.strip() for q in params.split(","))]
        assert args == want, f"{name}: {args} != {want}"
        assert res is (ctypes.c_long if name == "ovmr_retrieve_state_bytes" else ctypes.c_int)
        assert getattr(lib, name).argtypes == args
    assert text.count("No counterpart in the reference") == 5
    assert "ALL-ZERO BYTES ARE THE EMPTY STATE" in text and "base is a SCALAR" in text
    assert "ovmr_hip_retrieve.h" in inspect.getsource(build.build), "the build lists the header among its dependencies"
    for other in ("ovmr_hip.h", "ovmr_hip_nearest.h", "ovmr_hip_audit.h"):
        assert "retrieve" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", other)).read(), flags=re.S)


def test_state_bytes_and_argument_errors(lib):
    f = lib.ovmr_retrieve_state_bytes
    for C, m in ((1, 1), (1000, 5), (21841, 32), (65, 31)):
        assert f(C, m) == C * m * 8
    for C, m in ((0, 5), (-1, 5), (5, 0), (5, 33), (5, -1)):
        assert f(C, m) == -1
    E_ARG = -1
    o, s, t, v, i, fl = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))   # never dereferenced
    ok = dict(out=o, f32=0, ld=10, B=4, C=10, m=5, base=0, floor=fl, state=s)

    def update(**kw):
        a = dict(ok, **kw)
        return lib.ovmr_retrieve_update(a["out"], a["f32"], a["ld"], a["B"], a["C"], a["m"], a["base"], a["floor"], a["state"], None)

    for kw in (dict(out=None), dict(state=None), dict(m=0), dict(m=33), dict(C=0), dict(B=-1), dict(ld=9), dict(base=-1),
               dict(base=2 ** 32 - 1 - 3), dict(base=2 ** 32 - 1, B=1), dict(base=2 ** 40), dict(out=ctypes.c_void_p(0x10001)),
               dict(out=ctypes.c_void_p(0x10002), f32=1), dict(floor=ctypes.c_void_p(0x60002)), dict(state=ctypes.c_void_p(0x20004))):
        assert update(**kw) == E_ARG, kw
    assert update(B=0) == 0 and update(B=0, floor=None) == 0 and update(B=0, base=2 ** 32 - 1) == 0
    for fn, bad in ((lambda **k: lib.ovmr_retrieve_reset(k.get("s", s), k.get("C", 10), k.get("m", 5), None),
                     (dict(s=None), dict(s=ctypes.c_void_p(0x20004)), dict(C=0), dict(m=0), dict(m=33))),
                    (lambda **k: lib.ovmr_retrieve_merge(k.get("s", s), k.get("t", t), k.get("C", 10), k.get("m", 5), None),
                     (dict(s=None), dict(t=None), dict(s=ctypes.c_void_p(0x20004)), dict(t=ctypes.c_void_p(0x30004)), dict(C=0), dict(m=0), dict(m=33))),
                    (lambda **k: lib.ovmr_retrieve_finish(k.get("s", s), k.get("C", 10), k.get("m", 5), k.get("v", v), k.get("i", i), None),
                     (dict(s=None), dict(v=None), dict(i=None), dict(s=ctypes.c_void_p(0x20004)), dict(i=ctypes.c_void_p(0x50004)),
                      dict(v=ctypes.c_void_p(0x40002)), dict(C=0), dict(m=0), dict(m=33)))):
        for kw in bad:
            assert fn(**kw) == E_ARG, kw


# ---- the Python boundary of runtime.ColumnTopM -------------------------------------------------------------------------------------------

class _Recorder:
    """Stands where the library stands: records every call and says yes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ovmr_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def stub(monkeypatch):
    from ovmr_amd import runtime
    rec, log = _Recorder(), []
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    monkeypatch.setattr(runtime, "_same_device", lambda a, b: True)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: (log.append("stream"), SimpleNamespace(cuda_stream=0))[1])
    return SimpleNamespace(rec=rec, log=log, top=runtime.ColumnTopM(10, 5, "cpu"), runtime=runtime)


def _out(B=4, C=10, dtype=torch.float16):
    return torch.zeros((B, C), dtype=dtype)


UPDATE_VIOLATIONS = [
    ("out", "three dimensions", lambda: dict(out=torch.zeros((4, 2, 10), dtype=torch.float16), base=0)),
    ("out", "fp64", lambda: dict(out=_out(dtype=torch.float64), base=0)),
    ("out", "another C", lambda: dict(out=_out(C=11), base=0)),
    ("out", "a column stride", lambda: dict(out=torch.zeros((4, 20), dtype=torch.float16)[:, ::2], base=0)),
    ("out", "an expanded row", lambda: dict(out=torch.zeros((1, 10), dtype=torch.float16).expand(4, 10), base=0)),
    ("out", "a numpy array", lambda: dict(out=_out().numpy(), base=0)),
    ("base", "negative", lambda: dict(out=_out(), base=-1)),
    ("base", "past the last image", lambda: dict(out=_out(), base=2 ** 32 - 1 - 3)),
    ("base", "a float", lambda: dict(out=_out(), base=0.0)),
    ("base", "a bool", lambda: dict(out=_out(), base=True)),
    ("floor", "fp16", lambda: dict(out=_out(), base=0, floor=torch.zeros(4, dtype=torch.float16))),
    ("floor", "a row short", lambda: dict(out=_out(), base=0, floor=torch.zeros(3))),
    ("floor", "two dimensions", lambda: dict(out=_out(), base=0, floor=torch.zeros((4, 1)))),
    ("floor", "strided", lambda: dict(out=_out(), base=0, floor=torch.zeros(8)[::2])),
]


@pytest.mark.parametrize("arg,what,make", UPDATE_VIOLATIONS, ids=[f"{a}: {w}" for a, w, _ in UPDATE_VIOLATIONS])
def test_update_violation_is_refused_before_anything_reaches_the_library(arg, what, make, stub):
    with pytest.raises(ValueError) as err:
        stub.top.update(**make())
    msg = str(err.value)
    assert msg.startswith("ColumnTopM.update: ") and re.search(rf"(?<![\w]){re.escape(arg)}(?![\w\[])", msg), msg
    assert "must be" in msg and "got" in msg, msg
    assert stub.rec.calls == [] and stub.log == [], (stub.rec.calls, stub.log)


def test_merge_finish_and_constructor_refusals(stub):
    top, rt = stub.top, stub.runtime
    for other in (torch.zeros((10, 4), dtype=torch.int64), torch.zeros((10, 5), dtype=torch.int32), torch.zeros((10, 10), dtype=torch.int64)[:, ::2],
                  rt.ColumnTopM(10, 4, "cpu"), rt.ColumnTopM(9, 5, "cpu")):
        with pytest.raises(ValueError, match=r"^ColumnTopM\.merge: other must be"):
            top.merge(other)
    for out, name in ((torch.zeros((10, 5)), "out"), ((torch.zeros((10, 5), dtype=torch.float16), torch.zeros((10, 5), dtype=torch.int64)), r"out\[0\]"),
                      ((torch.zeros((10, 5)), torch.zeros((10, 5), dtype=torch.int32)), r"out\[1\]"),
                      ((torch.zeros((10, 5)), torch.zeros((10, 4), dtype=torch.int64)), r"out\[1\]")):
        with pytest.raises(ValueError, match=rf"^ColumnTopM\.finish: {name} must be"):
            top.finish(out)
    for C, m, name in ((0, 5, "C"), (10, 0, "m"), (10, 33, "m"), (10, 5.0, "m"), (10, True, "m")):
        with pytest.raises(ValueError, match=rf"^ColumnTopM: {name} must be an integer in"):
            rt.ColumnTopM(C, m, "cpu")
    assert stub.rec.calls == [] and stub.log == []


def test_device_mismatch_is_refused(monkeypatch):
    from ovmr_amd import runtime
    rec = _Recorder()
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    with pytest.raises(ValueError, match="ColumnTopM.update: out must be on cuda"):
        runtime.ColumnTopM(10, 5, "cpu").update(_out(), 0)
    assert rec.calls == []


def test_accepted_calls_hand_over_what_the_header_asks(stub):
    top, rt = stub.top, stub.runtime
    assert top.state.shape == (10, 5) and top.state.dtype == torch.int64 and not bool(top.state.any()), "all-zero: the empty state"
    big = torch.zeros((6, 13), dtype=torch.float32)
    floor = torch.zeros(4)
    assert top.update(big[1:5, :10], 2 ** 32 - 1 - 4, floor) is top
    (name, a), = stub.rec.calls
    assert name == "ovmr_retrieve_update" and len(a) == 10
    assert a[0].value == big[1:5].data_ptr() and a[1:7] == (rt.F32, 13, 4, 10, 5, 2 ** 32 - 1 - 4), "a row view goes as it is, with its stride"
    assert a[7].value == floor.data_ptr() and a[8].value == top.state.data_ptr()
    stub.rec.calls.clear()
    top.update(_out(B=1), 7)                                  # one row: ld is at least C; no floor: NULL
    a = stub.rec.calls[0][1]
    assert a[1:7] == (rt.F16, 10, 1, 10, 5, 7) and a[7] is None
    stub.rec.calls.clear()
    top.update(_out(B=0), 2 ** 32 - 1)                        # an empty batch launches nothing
    assert stub.rec.calls == []
    other = rt.ColumnTopM(10, 5, "cpu")
    top.merge(other)
    top.merge(torch.zeros((3, 10, 5), dtype=torch.int64)[1])  # a rank's slice of an all-gather
    assert [n for n, _ in stub.rec.calls] == ["ovmr_retrieve_merge"] * 2
    assert stub.rec.calls[0][1][:1][0].value == top.state.data_ptr() and stub.rec.calls[0][1][1].value == other.state.data_ptr()
    assert stub.rec.calls[0][1][2:4] == (10, 5)
    stub.rec.calls.clear()
    values, indices = top.finish()
    assert values.shape == indices.shape == (10, 5) and values.dtype == torch.float32 and indices.dtype == torch.int64
    a = stub.rec.calls[0][1]
    assert stub.rec.calls[0][0] == "ovmr_retrieve_finish" and a[0].value == top.state.data_ptr() and a[1:3] == (10, 5)
    assert a[3].value == values.data_ptr() and a[4].value == indices.data_ptr()
    out = (torch.zeros((10, 5)), torch.zeros((10, 5), dtype=torch.int64))
    res = top.finish(out)
    assert res[0] is out[0] and res[1] is out[1]
    top.reset()
    assert stub.rec.calls[-1][0] == "ovmr_retrieve_reset" and stub.rec.calls[-1][1][1:3] == (10, 5)


def test_models_and_trainers_share_the_signature():
    from ovmr_amd import modules, trainer
    want = [("batches", inspect.Parameter.empty), ("m", inspect.Parameter.empty), ("within_top", None), ("base", 0), ("eval_set_loader", None),
            ("overlap", None), ("stable_inputs", False)]
    for cls in (modules.CustomCLIP, modules.ZeroshotCLIP, modules.ZeroshotCLIP2):
        assert [(p.name, p.default) for p in inspect.signature(cls.retrieve_batches).parameters.values()][1:] == want
        assert cls.retrieve_batches is modules._TwoInFlight.retrieve_batches
    for cls in (trainer.MM_CLS_OP, trainer.ZeroshotCLIP, trainer.ZeroshotCLIP2):
        assert [(p.name, p.default) for p in inspect.signature(cls.retrieve).parameters.values()][1:] == [
            ("data_loader", inspect.Parameter.empty), ("m", 32), ("within_top", None)]
    doc = " ".join(modules._TwoInFlight.retrieve_batches.__doc__.split())
    assert "Ties at the cut are INCLUDED" in doc


def test_model_constants_are_the_kernels():
    """retrieve_cases.TILE / CHUNK place the planted defects of the CPU model at the kernel's own tile and chunk boundaries."""
    src = open(os.path.join(REPO, "ovmr_amd", "csrc", "retrieve.hip")).read()
    assert int(re.search(r"constexpr int RT_TILE = (\d+);", src).group(1)) == R.TILE
    assert int(re.search(r"constexpr int RT_ROWS = (\d+);", src).group(1)) == R.CHUNK
    assert int(re.search(r"constexpr int RT_TILE_NARROW = (\d+);", src).group(1)) == R.TILE_NARROW
    assert int(re.search(r"constexpr int RT_NARROW_MAX_C = (\d+);", src).group(1)) == R.NARROW_MAX_C
    import test_hip_retrieve as G
    cs = {shape[1] for shape in G.SHAPES}
    assert {R.NARROW_MAX_C, R.NARROW_MAX_C + 1} <= cs and any(c > R.NARROW_MAX_C and c % R.TILE for c in cs) and any(c % R.TILE_NARROW for c in cs)
    assert CASES["partial class tile"]["C"] % R.TILE_NARROW, "the case is a partial tile under either tiling"
    for case in ("partial class tile", "one call"):           # the cases the two defects are rejected on cross those boundaries
        assert CASES[case]["C"] % R.TILE or CASES[case]["N"] % R.CHUNK
    assert CASES["partial class tile"]["C"] > R.TILE and CASES["partial class tile"]["C"] % R.TILE
    assert CASES["one call"]["N"] > R.CHUNK and CASES["one call"]["N"] % R.CHUNK


def test_a_state_merged_with_itself_is_refused(lib, stub):
    s = ctypes.c_void_p(0x20000)
    assert lib.ovmr_retrieve_merge(s, s, 10, 5, None) == -1
    with pytest.raises(ValueError, match=r"^ColumnTopM\.merge: other must be the state of ANOTHER stream"):
        stub.top.merge(stub.top)
    with pytest.raises(ValueError, match=r"^ColumnTopM\.merge: other must be"):
        stub.top.merge(stub.top.state)
    assert stub.rec.calls == []


# ---- the runner --------------------------------------------------------------------------------------------------------------------------

def test_runner_refusals():
    from ovmr_amd import cli
    w = ["--clip-weights", "clip.pt"]
    r = w + ["--retrieve", "pool"]
    cli.check_retrieve(cli.parse(r), "MM_CLS_OP", False, "fusion")
    cli.check_retrieve(cli.parse(r + ["--per-class", "1", "--within-top", "32"]), "ZeroshotCLIP", True, "all")    # (the zero-shot trainers ignore EVAL_MODE)
    cli.check_retrieve(cli.parse(w), "MM_CLS_OP", False, "all")                                                  # (no --retrieve: nothing to refuse)
    a = cli.parse(r)
    assert a.retrieve == "pool" and a.per_class is None and a.within_top is None and cli.MAX_PER_CLASS == 32
    for argv, mode, msg in (
            (r + ["--predict", "pics"], "fusion", "--retrieve .* --predict"),
            (r, "all", "--retrieve .* --eval_mode all"),
            (r + ["--per-class-result"], "fusion", "--per-class-result belongs to the test pass: --retrieve"),
            (r + ["--confusion-matrix"], "fusion", "--confusion-matrix belongs to the test pass: --retrieve"),
            (r + ["--topk", "3"], "fusion", "--topk K belongs to --predict"),
            (w + ["--per-class", "5"], "fusion", "--per-class M belongs to --retrieve PATH"),
            (w + ["--within-top", "2"], "fusion", "--within-top K belongs to --retrieve PATH"),
            (r + ["--per-class", "0"], "fusion", r"--per-class 0: M must lie in \[1, 32\]"),
            (r + ["--per-class", "33"], "fusion", r"--per-class 33: M must lie in \[1, 32\]"),
            (r + ["--within-top", "0"], "fusion", r"--within-top 0: K must lie in \[1, min\(32, number of classes\)\]"),
            (r + ["--within-top", "33"], "fusion", r"--within-top 33: K must lie in \[1, min\(32, number of classes\)\]")):
        with pytest.raises(SystemExit, match=msg) as err:
            cli.check_retrieve(cli.parse(argv), "MM_CLS_OP", False, mode)
        assert "\n" not in str(err.value)
    cli.check_pool_size(2 ** 32 - 2, "pool")
    for n in (2 ** 32 - 1, 2 ** 32 + 5):
        with pytest.raises(SystemExit, match=r"--retrieve 'pool': a pool of [\d,]+ images"):
            cli.check_pool_size(n, "pool")
    # main refuses before anything is listed or loaded: PATH does not exist, the weights do not exist
    for argv, msg in ((r + ["--predict", "pics"], "--retrieve"), (r + ["--per-class", "40"], "--per-class 40"), (w + ["--within-top", "2"], "--within-top K belongs")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(["--eval-only", "--trainer", "MM_CLS_OP", "--eval_mode", "fusion"] + argv)
    with pytest.raises(SystemExit, match="--retrieve .* --eval_mode all"):
        cli.main(["--eval-only", "--trainer", "MM_CLS_OP", "--eval_mode", "all"] + r)
    with pytest.raises(SystemExit, match="--retrieve 'pool': no such directory or list file"):
        cli.main(["--eval-only", "--trainer", "MM_CLS_OP", "--eval_mode", "fusion"] + r)
    assert cli.PREDICT_ONE_PROCESS.startswith("--predict runs in one process")


def test_retrieval_table_and_file(tmp_path):
    import csv
    from ovmr_amd import cli
    values = torch.tensor([[0.5, 0.25, -INF], [NAN, 1e-3, 0.0], [-INF, -INF, -INF]])
    indices = torch.tensor([[2, 0, -1], [1, 2, 0], [-1, -1, -1]])
    rows = cli.retrieval_rows(values, indices, ["a.jpg", "b, c.jpg", "d.jpg"], ["cat", "dog, big", "emu"])
    assert [r[:4] for r in rows] == [(0, "cat", 0, "d.jpg"), (0, "cat", 1, "a.jpg"), (1, "dog, big", 0, "b, c.jpg"), (1, "dog, big", 1, "d.jpg"),
                                     (1, "dog, big", 2, "a.jpg")]
    cli.write_retrieval(str(tmp_path / "deep" / "retrieval.csv"), rows)
    lines = list(csv.reader(open(tmp_path / "deep" / "retrieval.csv")))
    assert lines[0] == cli.RETRIEVAL_COLUMNS == ["label", "classname", "rank", "image", "score"] and len(lines) == 6
    assert lines[1] == ["0", "cat", "0", "d.jpg", "0.5"] and lines[3] == ["1", "dog, big", "0", "b, c.jpg", "nan"]
    assert all(l[4] == repr(r[4]) for l, r in zip(lines[1:], rows)) and float(lines[4][4]) == rows[3][4]
