"""The nearest-exemplar search without a GPU: the expectation of nearest_cases.py against a brute-force loop, the comparator against the
defects it is there for (each on a named case), the extension header include/ovmr_hip_nearest.h against runtime.EXT_SIGNATURES and the
cross-compiled library's exports, the pure entry points and argument errors of the C ABI, the Python boundary of runtime.nearest_rows
on a recording stand-in, the neighbours.csv writer and the runner's refusals."""
import contextlib
import csv
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nearest_cases as N
from conftest import REPO


# ---- the expectation -------------------------------------------------------------------------------------------------------------

def _tiny_scores():
    s = torch.tensor([[0.5, -0.0, 0.0, float("nan"), 0.5, float("inf"), -float("inf"), 0.25, float("nan"), -1.0],
                      [0.0, 0.0, -0.0, 0.0, -0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                      [-2.0, -1.0, -1.0, -3.0, -1.0, -2.0, -1.0, -9.0, -1.0, -1.0]], dtype=torch.float16)
    return s


def test_expected_equals_brute_force():
    s = _tiny_scores()
    for k in (1, 3, 10):
        want = N.brute_force(s, k)
        assert N.mismatch(N.expected(s, k), want) is None
    assert N.expected(s, 4)[1].tolist() == [[3, 8, 5, 0], [0, 1, 2, 3], [1, 2, 4, 6]]
    ranges = torch.tensor([[2, 9], [4, 4], [8, 10]], dtype=torch.int32)
    for k in (1, 3, 8):
        assert N.mismatch(N.expected(s, k, ranges), N.brute_force(s, k, ranges)) is None
    v, i = N.expected(s, 3, ranges)
    assert i.tolist() == [[3, 8, 5], [-1, -1, -1], [8, 9, -1]] and v[1].tolist() == [-np.inf] * 3 and v[2, 2] == -np.inf
    Q, X, s16 = N.exact_case(9, 40, 64, 5, 1, nan_row=7, inf_row=20)
    r = N.range_table(9, 40, 5)
    assert N.mismatch(N.expected(s16, 5), N.brute_force(s16, 5)) is None and N.mismatch(N.expected(s16, 5, r), N.brute_force(s16, 5, r)) is None


def test_case_table_covers_the_issue():
    Bs, Rs, Ds, ks = ({s[i] for s in N.SHAPES} for i in range(4))
    assert {1, 63, 64, 65, 130} <= Bs and {1, 255, 256, 257, 1000, 70001} <= Rs and {64, 128, 512, 768, 1024} <= Ds and {1, 5, 31, 32} <= ks
    assert any(R == k for _, R, _, k in N.SHAPES)
    assert N.slices_for(1000) == [1, 2, 3, 4, 5] and N.slices_for(70001) == [1, 2, 3, 274, 275]
    assert N.BIG_R * N.BIG_D * 2 > 2 ** 31 and N.dup_pairs(1000) == [(1, 2), (6, 300), (9, 771)]
    r = N.range_table(130, 1000, 5)
    kinds = {(int(lo), int(hi)) for lo, hi in r[:64].tolist()}
    assert (17, 17) in kinds and (999, 1000) in kinds and (0, 1000) in kinds and (250, 262) in kinds and (500, 530) in kinds and (40, 43) in kinds
    assert int(r[64:, 1].max()) <= 100                      # the second query tile: every slice but the first has nothing to do
    assert N.margin(512) == 2 * (2.0 ** -12 + 512 * 2.0 ** -24)


# ---- the comparator rejects what it is there for --------------------------------------------------------------------------------------

def test_clean_model_passes_at_every_slice_count():
    Q, X, s16 = N.exact_case(6, 700, 64, 5, 3, nan_row=650)
    r = N.range_table(6, 700, 5)
    for slices in N.slices_for(700):
        assert N.mismatch(N.simulate(s16, 5, None, slices), N.expected(s16, 5)) is None
        assert N.mismatch(N.simulate(s16, 5, r, slices), N.expected(s16, 5, r)) is None


def test_rejects_ties_to_the_higher_row():
    Q, X, s16 = N.tie_cut_case(2)
    want = N.expected(s16, 2)
    assert want[1].tolist() == [[3, 290]] * 5
    assert N.mismatch(N.simulate(s16, 2, None, 1), want) is None
    assert "expected row 3" in N.mismatch(N.simulate(s16, 2, None, 1, "ties_high"), want)
    Q, X, s16 = N.zero_bank_case()
    assert N.mismatch(N.simulate(s16[:2], 4, None, 2, "ties_high"), N.expected(s16[:2], 4)) is not None


def test_rejects_ordering_by_the_unrounded_score():
    """Row 4's fp32 score exceeds row 1's by 2^-14 and rounds to the same fp16 number: rounded, row 1 comes first."""
    Q = torch.zeros((1, 64), dtype=torch.float16)
    Q[0, 0], Q[0, 1] = 1 + 2.0 ** -10, 1.0
    X = torch.zeros((8, 64), dtype=torch.float16)
    X[1, 0] = 1.0
    X[4, 0], X[4, 1] = 1.0, 2.0 ** -14
    s32 = (Q.double() @ X.double().t()).float()
    s16 = N.scores16(Q, X)
    assert float(s32[0, 4]) > float(s32[0, 1]) and float(s16[0, 4]) == float(s16[0, 1])
    want = N.expected(s16, 2)
    assert want[1].tolist() == [[1, 4]]
    assert N.mismatch(N.simulate(s16, 2, None, 1, s32=s32), want) is None
    assert N.mismatch(N.simulate(s16, 2, None, 1, "unrounded", s32=s32), want) is not None


def test_rejects_a_dropped_tile_and_a_deduplicating_merge():
    """Query 5 is aligned with bank row 6, of which row 300 (the second tile) is a copy: the pair takes the first two ranks."""
    Q, X, s16 = N.exact_case(6, 700, 64, 3, 11)
    want = N.expected(s16, 3)
    assert want[1][5, :2].tolist() == [6, 300] and want[1][1, :2].tolist() == [1, 2]
    for slices in (1, 3):
        assert N.mismatch(N.simulate(s16, 3, None, slices), want) is None
        assert N.mismatch(N.simulate(s16, 3, None, slices, "drop_tile", t_bad=1), want) is not None
    assert N.mismatch(N.simulate(s16, 3, None, 3, "dedup_merge"), want) is not None


def test_rejects_an_inclusive_range_end_and_a_zero_tail():
    Q, X, s16 = N.exact_case(8, 700, 64, 5, 12)
    r = N.range_table(8, 700, 5)
    want = N.expected(s16, 5, r)
    assert bool((want[1] == -1).any())
    assert N.mismatch(N.simulate(s16, 5, r, 2), want) is None
    assert N.mismatch(N.simulate(s16, 5, r, 2, "range_inclusive"), want) is not None
    assert N.mismatch(N.simulate(s16, 5, r, 2, "tail_zero"), want) is not None
    assert N.mismatch(N.expected(s16, 5, r, tail_index=0), want) is not None


def test_rejects_a_32_bit_offset_on_the_large_bank():
    """A 32-bit byte offset makes the rows from 2^31 bytes on read the bank's first rows again: the last tile then shows copies of rows
    0 .. and loses its planted rows."""
    k = 5
    Q, planted = N.big_bank_plan(k)
    want = N.big_bank_expected(Q, planted, k)
    first_past = 2 ** 31 // (2 * N.BIG_D)
    assert want[1][0].tolist() == [N.BIG_R - 1, first_past, 0, N.BIG_R - 200, 1] and max(planted) == N.BIG_R - 1
    assert N.mismatch(N.big_bank_expected(Q, planted, k), want) is None
    assert N.mismatch(N.big_bank_expected(Q, planted, k, alias=first_past), want) is not None


def test_general_comparator():
    Q, X = N.general_case(128, 4, classes=10, per_class=6, B=12)
    s16 = N.scores16(Q, X)
    k = 5
    good = N.expected(s16, k)
    assert N.general_mismatch(good, Q, X, k) is None
    v, i = good[0].clone(), good[1].clone()
    worst = (Q.double() @ X.double().t()).argmin(1)
    i[:, 2] = worst.to(torch.int32)
    assert "k-th best" in N.general_mismatch((v, i), Q, X, k)
    v2 = good[0].clone()
    v2[:, 1] += 0.01
    assert N.general_mismatch((v2, good[1]), Q, X, k) is not None
    sw = good[1].clone()
    sw[:, [0, 1]] = sw[:, [1, 0]]
    assert N.general_mismatch((good[0], sw), Q, X, k) is not None or bool((good[0][:, 0] == good[0][:, 1]).any())
    ranges = torch.tensor([[6 * (b % 10), 6 * (b % 10) + 6] for b in range(12)], dtype=torch.int32)
    assert N.general_mismatch(N.expected(s16, k, ranges), Q, X, k, ranges) is None
    assert "outside" in N.general_mismatch(good, Q, X, k, ranges)


# ---- the extension header, its table and the library ------------------------------------------------------------------------------------

def _header():
    text = open(os.path.join(REPO, "include", "ovmr_hip_nearest.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import build, runtime
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    return runtime.load_library()


def test_extension_header_table_and_exports(lib):
    from ovmr_amd import runtime
    text, code = _header()
    decls = dict(re.findall(r"\b(ovmr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(decls) == set(runtime.EXT_SIGNATURES) == {"ovmr_nearest_scratch_bytes", "ovmr_nearest_rows", "ovmr_debug_nearest_rows"}
    assert not set(runtime.EXT_SIGNATURES) & set(runtime.SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ovmr_hip.h")).read(), flags=re.S)
    assert "nearest" not in main
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long}
    for name, params in decls.items():
        res, args = runtime.EXT_SIGNATURES[name]
        assert hasattr(lib, name), f"{name} declared in include/ovmr_hip_nearest.h but not exported"
        want = [ctypes.c_void_p if "*" in p or "ovmr_stream" in p else ctype[p.split()[0]] for p in (q.strip() for q in params.split(","))]
        assert args == want, f"{name}: {args} != {want}"
        assert res is (ctypes.c_long if name == "ovmr_nearest_scratch_bytes" else ctypes.c_int)
        assert getattr(lib, name).argtypes == args
    assert text.count("No counterpart in the reference") == 3


def test_scratch_bytes_and_argument_errors(lib):
    f = lib.ovmr_nearest_scratch_bytes
    for B, R, k in ((1, 1, 1), (256, 640000, 32), (256, 16000, 5), (1280, 640000, 5), (130, 70001, 31), (0, 5, 1)):
        n = f(B, R, k)
        assert n >= 0 and n % 8 == 0 and (B == 0 or n % (B * k * 8) == 0)
        if B:
            S = n // (B * k * 8)
            assert 1 <= S <= N.n_tiles(R), "never a slice below one tile"
    assert f(256, 640000, 32) // (256 * 32 * 8) > 1
    for B, R, k in ((-1, 5, 1), (4, 0, 1), (4, 2 ** 32 - 1, 1), (4, 5, 0), (4, 5, 33)):
        assert f(B, R, k) == -1
    assert f(4, 2 ** 32 - 2, 1) > 0
    E_ARG = -1
    q, x, v, i, s = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))   # never dereferenced: every call below is refused
    ok = dict(q=q, B=4, x=x, R=100, D=128, k=5, ranges=None, v=v, i=i, s=s, n=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ovmr_nearest_rows(a["q"], a["B"], a["x"], a["R"], a["D"], a["k"], a["ranges"], a["v"], a["i"], a["s"], a["n"], None)

    for kw in (dict(q=None), dict(x=None), dict(v=None), dict(i=None), dict(s=None), dict(q=ctypes.c_void_p(0x10008)), dict(x=ctypes.c_void_p(0x20002)),
               dict(s=ctypes.c_void_p(0x50004)), dict(v=ctypes.c_void_p(0x30002)), dict(ranges=ctypes.c_void_p(0x60001)), dict(D=0), dict(D=96),
               dict(D=1088), dict(D=32), dict(k=0), dict(k=33), dict(k=101, R=100), dict(R=0), dict(R=2 ** 32 - 1), dict(B=-1), dict(n=4 * 5 * 8 - 1),
               dict(n=-1)):
        assert call(**kw) == E_ARG, kw
    assert call(B=0) == 0 and call(B=0, q=None, v=None, i=None) == 0
    hook = lib.ovmr_debug_nearest_rows
    assert hook(q, 4, x, 100, 128, 5, None, v, i, s, 1 << 20, 0, None) == E_ARG
    assert hook(q, 4, x, 100, 128, 5, None, v, i, s, 4 * 3 * 5 * 8 - 1, 3, None) == E_ARG
    assert hook(q, 0, x, 100, 128, 5, None, v, i, s, 0, 3, None) == 0


# ---- the Python boundary of runtime.nearest_rows ------------------------------------------------------------------------------------------

class _Recorder:
    """Stands where the library stands: records every call and says yes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ovmr_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 8 * 1024 if name == "ovmr_nearest_scratch_bytes" else 0
        return call


@pytest.fixture
def stub(monkeypatch):
    """runtime.nearest_rows on a recording library, host tensors standing for device tensors (every check but the device's stays)."""
    from ovmr_amd import runtime
    rec, log = _Recorder(), []
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    monkeypatch.setattr(runtime, "_same_device", lambda a, b: True)
    monkeypatch.setattr(runtime, "_nearest_scratch", {})
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: (log.append("stream"), SimpleNamespace(cuda_stream=0))[1])
    return SimpleNamespace(rec=rec, log=log, call=runtime.nearest_rows)


def _ops(B=5, R=40, D=128):
    return dict(queries=torch.zeros((B, D), dtype=torch.float16), bank=torch.zeros((R, D), dtype=torch.float16), k=3)


VIOLATIONS = [
    ("queries", "three dimensions", lambda o: o.update(queries=torch.zeros((5, 2, 64), dtype=torch.float16))),
    ("queries", "fp32", lambda o: o.update(queries=o["queries"].float())),
    ("queries", "not a tensor", lambda o: o.update(queries=[[0.0] * 128])),
    ("queries", "a numpy array", lambda o: o.update(queries=np.zeros((5, 128), dtype=np.float16))),
    ("queries", "width 96", lambda o: o.update(queries=torch.zeros((5, 96), dtype=torch.float16), bank=torch.zeros((40, 96), dtype=torch.float16))),
    ("queries", "width 2048", lambda o: o.update(queries=torch.zeros((5, 2048), dtype=torch.float16), bank=torch.zeros((40, 2048), dtype=torch.float16))),
    ("bank", "another width", lambda o: o.update(bank=torch.zeros((40, 64), dtype=torch.float16))),
    ("bank", "fp32", lambda o: o.update(bank=o["bank"].float())),
    ("bank", "one dimension", lambda o: o.update(bank=torch.zeros((128,), dtype=torch.float16))),
    ("k", "zero", lambda o: o.update(k=0)),
    ("k", "33", lambda o: o.update(k=33, bank=torch.zeros((64, 128), dtype=torch.float16))),
    ("k", "more than the bank's rows", lambda o: o.update(k=5, bank=torch.zeros((4, 128), dtype=torch.float16))),
    ("k", "a float", lambda o: o.update(k=2.0)),
    ("ranges", "shape [B, 3]", lambda o: o.update(ranges=torch.zeros((5, 3), dtype=torch.int32))),
    ("ranges", "a row short", lambda o: o.update(ranges=torch.zeros((4, 2), dtype=torch.int32))),
    ("ranges", "floating point", lambda o: o.update(ranges=torch.zeros((5, 2)))),
    ("ranges", "negative lo (host)", lambda o: o.update(ranges=torch.tensor([[0, 3]] * 4 + [[-1, 3]], dtype=torch.int64))),
    ("ranges", "hi beyond R (host)", lambda o: o.update(ranges=torch.tensor([[0, 3]] * 4 + [[2, 41]], dtype=torch.int32))),
    ("ranges", "lo above hi (host)", lambda o: o.update(ranges=torch.tensor([[0, 3]] * 4 + [[7, 6]], dtype=torch.int32))),
    ("out", "not a pair", lambda o: o.update(out=torch.zeros((5, 3)))),
    ("out[0]", "fp16 values", lambda o: o.update(out=(torch.zeros((5, 3), dtype=torch.float16), torch.zeros((5, 3), dtype=torch.int32)))),
    ("out[1]", "int64 indices", lambda o: o.update(out=(torch.zeros((5, 3)), torch.zeros((5, 3), dtype=torch.int64)))),
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
    assert msg.startswith("nearest_rows: ") and re.search(rf"(?<![\w]){re.escape(arg)}(?![\w\[])", msg), msg
    assert "must be" in msg and "got" in msg, msg
    assert stub.rec.calls == [] and stub.log == [], (stub.rec.calls, stub.log)


def test_device_mismatch_is_refused(monkeypatch):
    from ovmr_amd import runtime
    rec = _Recorder()
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    with pytest.raises(ValueError, match="nearest_rows: queries must be on cuda"):
        runtime.nearest_rows(**_ops())
    assert rec.calls == []


def test_accepted_call_hands_over_what_the_header_asks(stub):
    ops = _ops()
    wide = torch.zeros((5, 256), dtype=torch.float16)
    ops.update(queries=wide[:, ::2], ranges=np.array([[0, 40], [3, 3], [39, 40], [0, 1], [5, 9]], dtype=np.int64))
    values, indices = stub.call(**ops)
    assert values.shape == indices.shape == (5, 3) and values.dtype == torch.float32 and indices.dtype == torch.int32
    names = [n for n, _ in stub.rec.calls]
    assert names == ["ovmr_nearest_scratch_bytes", "ovmr_nearest_rows"]
    assert stub.rec.calls[0][1] == (5, 40, 3)
    a = stub.rec.calls[1][1]
    assert a[1] == 5 and a[3] == 40 and a[4] == 128 and a[5] == 3 and a[10] >= 8 * 1024 and len(a) == 12
    assert a[0].value != wide.data_ptr(), "a strided view goes to the library as a dense copy"
    assert a[2].value == ops["bank"].data_ptr() and a[6].value is not None and a[7].value == values.data_ptr() and a[8].value == indices.data_ptr()
    stub.rec.calls.clear()
    out = (torch.zeros((5, 3)), torch.zeros((5, 3), dtype=torch.int32))
    res = stub.call(ops["queries"], ops["bank"], 3, out=out)
    assert res[0] is out[0] and res[1] is out[1] and stub.rec.calls[1][1][6] is None
    stub.rec.calls.clear()                                  # an empty batch launches nothing
    v, i = stub.call(torch.zeros((0, 128), dtype=torch.float16), ops["bank"], 3)
    assert v.shape == (0, 3) and stub.rec.calls == []


# ---- the runner: neighbours.csv and the refusals of --nearest -------------------------------------------------------------------------------

def test_neighbours_csv(tmp_path):
    from ovmr_amd import cli
    names = ["cat", "dog, big", "emu"]
    indices = torch.tensor([[2, 0], [1, 2]])
    sims = torch.tensor([[[0.75, 0.5], [0.25, -np.inf]], [[1.0, 0.1015625], [0.5, 0.5]]])
    rows = torch.tensor([[[5, 4], [0, -1]], [[2, 3], [4, 5]]])
    paths = [f"bank/{i}.png" for i in range(6)]
    got = cli.nearest_neighbours(["a.png", "b.png"], indices, sims, rows, names, paths)
    assert got[0] == ("a.png", 0, 2, "emu", 0, 5, "bank/5.png", 0.75) and len(got) == 7
    out = tmp_path / "deep" / "neighbours.csv"
    cli.write_neighbours(str(out), got)
    lines = list(csv.reader(open(out)))
    assert lines[0] == ["image", "rank", "label", "classname", "neighbour", "row", "exemplar", "similarity"] == cli.NEIGHBOUR_COLUMNS
    assert lines[1:] == [["a.png", "0", "2", "emu", "0", "5", "bank/5.png", "0.75"], ["a.png", "0", "2", "emu", "1", "4", "bank/4.png", "0.5"],
                         ["a.png", "1", "0", "cat", "0", "0", "bank/0.png", "0.25"], ["b.png", "0", "1", "dog, big", "0", "2", "bank/2.png", "1.0"],
                         ["b.png", "0", "1", "dog, big", "1", "3", "bank/3.png", "0.1015625"], ["b.png", "1", "2", "emu", "0", "4", "bank/4.png", "0.5"],
                         ["b.png", "1", "2", "emu", "1", "5", "bank/5.png", "0.5"]]
    assert all(float(l[7]) == g[7] for l, g in zip(lines[1:], got))
    # a bank without paths: the column stays empty
    assert cli.nearest_neighbours(["a.png"], indices[:1], sims[:1], rows[:1], names)[0][6] == ""
    # the similarity has the format of predictions.csv's score
    cli.write_predictions(str(tmp_path / "p.csv"), [("a.png", [(2, "emu", 0.1015625)])])
    assert list(csv.reader(open(tmp_path / "p.csv")))[1][4] == lines[5][7]


def test_runner_refusals():
    from ovmr_amd import cli
    w = ["--clip-weights", "clip.pt"]
    base = w + ["--predict", "pics", "--nearest", "3"]
    cli.check_nearest(cli.parse(base), "MM_CLS_OP", False)
    cli.check_nearest(cli.parse(w + ["--predict", "pics"]), "ZeroshotCLIP", True)        # (no --nearest: nothing to refuse)
    for argv, trainer, zeroshot, msg in (
            (w + ["--nearest", "3"], "MM_CLS_OP", False, "--nearest N belongs to --predict PATH"),
            (base, "ZeroshotCLIP", True, "--trainer ZeroshotCLIP has no exemplars to search"),
            (base, "ZeroshotCLIP2", True, "--trainer ZeroshotCLIP2 has no exemplars to search"),
            (base + ["--classifiers", "mm_classifiers.pt"], "MM_CLS_OP", False, "holds no exemplar features"),
            (w + ["--predict", "pics", "--nearest", "0"], "MM_CLS_OP", False, r"--nearest 0: N must lie in \[1, 32\]"),
            (w + ["--predict", "pics", "--nearest", "33"], "MM_CLS_OP", False, r"--nearest 33: N must lie in \[1, 32\]")):
        with pytest.raises(SystemExit, match=msg) as err:
            cli.check_nearest(cli.parse(argv), trainer, zeroshot)
        assert "\n" not in str(err.value)


def test_zero_shot_trainer_refuses_in_one_line():
    from ovmr_amd import trainer
    t = object.__new__(trainer.ZeroshotCLIP)
    t.cfg = SimpleNamespace(TRAINER=SimpleNamespace(NAME="ZeroshotCLIP"))
    with pytest.raises(ValueError, match="--trainer ZeroshotCLIP: nearest exemplars need a model that holds exemplar features") as err:
        t.explained(iter(()), 5, 3)
    assert "\n" not in str(err.value)
