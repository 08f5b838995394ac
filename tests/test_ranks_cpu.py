"""Exact ranking figures without a GPU: the reference of ranks_cases.py against its literal restatement, the comparator against planted
defects, the header against runtime.RANKS_SIGNATURES and the library's exports, the argument errors through the loaded library, the
Python boundary of runtime.eval_ranks, the host evaluator against sklearn on the raw scores, the files, and the runner's refusals."""
import contextlib
import csv
import ctypes
import inspect
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ranks_cases as K
from conftest import REPO

INF, NAN = math.inf, math.nan


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def test_reference_equals_its_literal_restatement():
    for fp16 in (False, True):
        counts = [0, 1, 2, 7, 20, 64, 65]
        edges, estart = K.make_edges(counts, 3, special=True, fp16=fp16)
        out = K.scores(90, len(counts), edges, estart, "special", fp16, seed=3).float().numpy()
        got = K.cells(out, edges, estart)
        for c, n in enumerate(counts):
            mine = edges[estart[c]:estart[c + 1]]
            assert len(mine) == n and all(K.value_key(a) > K.value_key(b) for a, b in zip(mine[:-1], mine[1:])), "strictly descending"
            assert got[:, c].tolist() == [K.cell_literal(x, mine) for x in out[:, c]]
            assert got[:, c].min() >= 0 and got[:, c].max() <= 2 * n
        assert (got % 2 == 1).sum() > 100 and (got % 2 == 0).sum() > 100, "ties and gaps both occur"


def test_the_order_is_the_selection_keys():
    nan, nnan = (np.array([b], dtype=np.uint32).view(np.float32)[0] for b in (0x7FC00000, 0xFFC00000))
    tiny = np.float32(1e-45)
    edges = [nan, np.float32(INF), np.float32(1.0), tiny, np.float32(0.0), -tiny, np.float32(-INF)]
    cell = lambda x: K.cell_literal(np.float32(x), edges)       # noqa: E731
    assert cell(nan) == cell(nnan) == 1, "every NaN is one value, the largest"
    assert cell(INF) == 3 and cell(2.0) == 4 and cell(1.0) == 5 and cell(0.5) == 6
    assert cell(tiny) == 7 and cell(0.0) == cell(-0.0) == 9 and cell(-tiny) == 11, "-0 == +0; a denormal is its own number"
    assert cell(-1.0) == 12 and cell(-INF) == 13
    assert K.cell_literal(np.float32(0.3), []) == 0 and K.cell_literal(nan, []) == 0, "a class without a positive has one cell"
    from ovmr_amd.evaluator import rank_cells, rank_keys
    v = np.concatenate([K.specials(), K.specials(True), np.linspace(-3, 3, 41, dtype=np.float32)])
    assert rank_keys(v).tolist() == K.keys(v).tolist()
    got = rank_cells(torch.from_numpy(v).unsqueeze(1), torch.tensor(edges), torch.tensor([0, len(edges)], dtype=torch.int32))
    assert got[:, 0].tolist() == [K.cell_literal(x, edges) for x in v]


def test_rank_edges_is_the_value_by_value_table_and_ignores_order():
    from ovmr_amd.evaluator import rank_edges
    C = 9
    edges, estart = K.make_edges([4] * C, 1, special=True)
    out, y = K.scores(200, C, edges, estart, "special", seed=1), K.labels(200, C, "bad", seed=1)
    out[y == 7] = 0.5                                            # a class whose positives all tie
    y[y == 8] = 0                                                # and one without a positive
    want_e, want_s = K.edges_of(out, y, C)
    ok = (y >= 0) & (y < C)
    s = out[torch.arange(200)[ok], y[ok]]
    for perm in (torch.arange(len(s)), torch.randperm(len(s), generator=torch.Generator().manual_seed(0))):
        e, st = rank_edges(s[perm], y[ok][perm], C)
        assert e.dtype == torch.float32 and st.dtype == torch.int32 and st.tolist() == want_s.tolist()
        assert e.numpy().view(np.uint32).tolist() == want_e.view(np.uint32).tolist(), "canonical bits: one NaN, +0"
    e, st = rank_edges(out[:, 0], y, C)                          # labels outside [0, C) are left out, not refused
    assert st[-1] == len(e) and int(st[8]) == int(st[9]) and int(st[8] - st[7]) == 1
    e, st = rank_edges(torch.zeros(0), torch.zeros(0, dtype=torch.int64), 3)
    assert e.shape == (0,) and st.tolist() == [0, 0, 0, 0]
    e, st = rank_edges(torch.tensor([0.0, -0.0, NAN, -NAN, 1.0]), torch.zeros(5, dtype=torch.int64), 1)
    assert e.numpy().view(np.uint32).tolist() == [0x7FC00000, 0x3F800000, 0] and st.tolist() == [0, 3]


# ---- the comparator and the planted defects --------------------------------------------------------------------------------------------

# name -> (B, edge counts, score kind, label kind, special edges, fp16, estart override): the GPU tests' own sizes -- a partial last chunk
# of rows, a partial last tile of classes
GARBAGE = [5, -7, 900, 3, 2 ** 31 - 1, -2 ** 31, 100, 99, 0, 900, 10, 10, 700, 2, 101, -1, 64, 63]
CASES = {
    "ties": (130, [3, 0, 9, 1] * 8 + [5], "mixed", "random", False, False, None),
    "special values": (130, [12] * 17, "special", "bad", True, False, None),
    "softmax": (65, [2, 5, 0] * 11, "softmax", "hot", False, True, None),
    "garbage estart": (65, [6] * 17, "mixed", "bad", False, False, GARBAGE),
}
REJECTED_ON = {"tie_in_gap": "ties", "neg_zero_differs": "special values", "nan_lowest": "special values", "base_without_c": "ties",
               "planes_swapped": "ties", "last_cell_dropped": "softmax", "neighbour_edges": "ties", "estart_unclamped": "garbage estart"}


def _run(case, defect=None):
    B, counts, kind, label_kind, special, fp16, override = CASES[case]
    C = len(counts)
    edges, estart = K.make_edges(counts, 3, special, fp16)
    out, y = K.scores(B, C, edges, estart, kind, fp16, seed=3), K.labels(B, C, label_kind, seed=3)
    before = K.random_state(C, len(edges), seed=3)
    if override is not None:                                     # (no brute-force rule for ranges that do not descend: the honest walk)
        estart = np.array(override, dtype=np.int32)
        want, outside = K.model(out, y, edges, estart, max(counts), before.clone())
        offered = int(((y >= 0) & (y < C)).sum())
        assert outside == 0 and int((want - before).sum()) == offered * C and int((want - before).min()) >= 0
    else:
        want = K.expected(out, y, edges, estart, max(counts), before)
    got, outside = K.model(out, y, edges, estart, max(counts), before.clone(), defect)
    return K.mismatch(got, want) or (f"{outside} adds fell outside the state" if outside else None)


@pytest.mark.parametrize("case", sorted(CASES))
def test_honest_model_passes(case):
    assert _run(case) is None


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_defect_is_rejected(defect):
    msg = _run(REJECTED_ON[defect], defect)
    assert msg is not None and ("cells differ" in msg or "outside the state" in msg), f"{defect} passes on {REJECTED_ON[defect]!r}"


def test_defect_table_is_the_issues_and_mismatch_reads():
    assert set(REJECTED_ON) == set(K.DEFECTS) and len(K.DEFECTS) == 8 and set(REJECTED_ON.values()) <= set(CASES)
    a = torch.zeros((2, 15), dtype=torch.int32)
    b = a.clone()
    assert K.mismatch(a, b) is None and "shape" in K.mismatch(a, b[:, :4])
    b[1, 4] = 2
    assert K.mismatch(a, b) == "1 of 30 cells differ, the first at plane 1, cell 4 of 15: got 0, expected 2"


def test_model_constants_are_the_kernels():
    src = open(os.path.join(REPO, "ovmr_amd", "csrc", "eval_ranks.hip")).read()
    for name, want in (("RK_TILE", K.TILE), ("RK_ROWS", K.CHUNK), ("RK_MAX_ROW_BLOCKS", K.MAX_ROW_BLOCKS), ("RK_STAGE", K.STAGE)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == want, name
    assert '#include "eval_common.h"' in src and "wave_histogram_add(" in src and "load_tile_transposed<" in src and "topk_key(" in src
    for copied in ("wave_histogram_add(int*", "topk_key(float", "void load_tile_transposed"):
        assert copied not in src, "the helpers are shared through eval_common.h, not copied"
    assert "atomicAdd(float" not in src and "float*>(state" not in src, "no float atomics"
    for case in CASES.values():
        assert case[0] % K.CHUNK and case[0] > K.CHUNK and len(case[1]) % K.TILE and len(case[1]) > K.TILE


# ---- the header, its table and the library ---------------------------------------------------------------------------------------------

NAMES = {"ovmr_eval_ranks_state_cells", "ovmr_eval_ranks"}


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import build, runtime
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    return runtime.load_library()


def test_ranks_header_table_and_exports(lib):
    from ovmr_amd import build, runtime
    text = open(os.path.join(REPO, "include", "ovmr_hip_ranks.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = dict(re.findall(r"\b(ovmr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(decls) == set(runtime.RANKS_SIGNATURES) == NAMES
    assert not set(runtime.RANKS_SIGNATURES) & (set(runtime.SIGNATURES) | set(runtime.EXT_SIGNATURES) | set(runtime.AUDIT_SIGNATURES)
                                                | set(runtime.RETRIEVE_SIGNATURES) | set(runtime.CURVES_SIGNATURES))
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    for name, params in decls.items():
        res, args = runtime.RANKS_SIGNATURES[name]
        assert hasattr(lib, name), f"{name} declared in include/ovmr_hip_ranks.h but not exported"
        want = [ctypes.c_void_p if "*" in p or "ovmr_stream" in p else ctype[p.split()[0]] for p in (q.strip() for q in params.split(","))]
        assert args == want, f"{name}: {args} != {want}"
        assert res is (ctypes.c_long if name == "ovmr_eval_ranks_state_cells" else ctypes.c_int)
        assert getattr(lib, name).argtypes == args
    assert text.count("No counterpart in the reference") == 2
    flat = " ".join(re.sub(r"\n \* ?", " ", text).split())
    for phrase in ("ALL-ZERO BYTES ARE THE EMPTY STATE", "fewer than 2^31 images", "STRICTLY DESCENDING", "never used as an address",
                   "-0.0 == +0.0", "2 estart[c] + c", "integer atomics"):
        assert phrase in flat, phrase
    assert "ovmr_hip_ranks.h" in inspect.getsource(build.build), "the build lists the header among its dependencies"
    assert '#include "ovmr_hip.h"' in code and "ovmr_hip_curves.h" not in code, "the header stands alone"
    for other in ("ovmr_hip.h", "ovmr_hip_nearest.h", "ovmr_hip_audit.h", "ovmr_hip_retrieve.h", "ovmr_hip_curves.h"):
        assert "ranks" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", other)).read(), flags=re.S)


def test_state_cells_and_argument_errors(lib):
    f = lib.ovmr_eval_ranks_state_cells
    for C, E in ((1, 0), (1000, 50_000), (21841, 2 ** 31), (65, 7)):
        assert f(C, E) == 2 * (2 * E + C)
    for C, E in ((0, 5), (-1, 5), (5, -1)):
        assert f(C, E) == -1
    E_ARG = -1
    o, y, e, s, st = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))       # never dereferenced
    ok = dict(out=o, f32=0, ld=10, labels=y, B=4, C=10, edges=e, estart=s, E=30, me=5, state=st)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ovmr_eval_ranks(a["out"], a["f32"], a["ld"], a["labels"], a["B"], a["C"], a["edges"], a["estart"], a["E"], a["me"],
                                   a["state"], None)

    for kw in (dict(out=None), dict(labels=None), dict(edges=None), dict(estart=None), dict(state=None), dict(C=0), dict(B=-1), dict(ld=9),
               dict(E=-1), dict(me=-1), dict(me=31), dict(E=0), dict(out=ctypes.c_void_p(0x10001)), dict(out=ctypes.c_void_p(0x10002), f32=1),
               dict(labels=ctypes.c_void_p(0x20004)), dict(edges=ctypes.c_void_p(0x30002)), dict(estart=ctypes.c_void_p(0x40002)),
               dict(state=ctypes.c_void_p(0x50002))):
        assert call(**kw) == E_ARG, kw
        assert call(**dict(dict(B=0), **kw)) == E_ARG, ("B == 0 excuses no argument", kw)
    assert call(B=0) == 0 and call(B=0, f32=1) == 0 and call(B=0, out=ctypes.c_void_p(0x10002)) == 0 and call(B=0, me=30) == 0
    assert call(B=0, E=0, me=0, edges=None) == 0 and call(B=0, E=0, me=0) == 0, "edges may be NULL when E == 0"


# ---- the Python boundary of runtime.eval_ranks -------------------------------------------------------------------------------------------

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
    rec, log, ptrs = _Recorder(), [], []
    real_ptr = runtime._ptr
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    monkeypatch.setattr(runtime, "_same_device", lambda a, b: True)
    monkeypatch.setattr(runtime, "_ptr", lambda t: (ptrs.append(t), real_ptr(t))[1])
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: (log.append("stream"), SimpleNamespace(cuda_stream=0))[1])
    return SimpleNamespace(rec=rec, log=log, ptrs=ptrs, runtime=runtime)


def _ok(B=4, C=10, E=30, dtype=torch.float16):
    return dict(mo=torch.zeros((B, C), dtype=dtype), labels=torch.zeros(B, dtype=torch.int64), edges=torch.zeros(E), max_edges=min(E, 5),
                estart=torch.zeros(C + 1, dtype=torch.int32), state=torch.zeros((2, 2 * E + C), dtype=torch.int32))


VIOLATIONS = [
    ("mo", "three dimensions", lambda: dict(mo=torch.zeros((4, 2, 10), dtype=torch.float16))),
    ("mo", "fp64", lambda: dict(mo=torch.zeros((4, 10), dtype=torch.float64))),
    ("mo", "a column stride", lambda: dict(mo=torch.zeros((4, 20), dtype=torch.float16)[:, ::2])),
    ("mo", "an expanded row", lambda: dict(mo=torch.zeros((1, 10), dtype=torch.float16).expand(4, 10))),
    ("mo", "a numpy array", lambda: dict(mo=np.zeros((4, 10), dtype=np.float16))),
    ("mo", "no column", lambda: dict(mo=torch.zeros((4, 0), dtype=torch.float16), estart=torch.zeros(1, dtype=torch.int32),
                                     state=torch.zeros((2, 60), dtype=torch.int32))),
    ("labels", "int32", lambda: dict(labels=torch.zeros(4, dtype=torch.int32))),
    ("labels", "a row short", lambda: dict(labels=torch.zeros(3, dtype=torch.int64))),
    ("labels", "strided", lambda: dict(labels=torch.zeros(8, dtype=torch.int64)[::2])),
    ("edges", "fp16", lambda: dict(edges=torch.zeros(30, dtype=torch.float16))),
    ("edges", "two dimensions", lambda: dict(edges=torch.zeros((10, 3)))),
    ("edges", "strided", lambda: dict(edges=torch.zeros(60)[::2])),
    ("edges", "a numpy array", lambda: dict(edges=np.zeros(30, dtype=np.float32))),
    ("estart", "int64", lambda: dict(estart=torch.zeros(11, dtype=torch.int64))),
    ("estart", "C entries", lambda: dict(estart=torch.zeros(10, dtype=torch.int32))),
    ("estart", "strided", lambda: dict(estart=torch.zeros(22, dtype=torch.int32)[::2])),
    ("state", "int64", lambda: dict(state=torch.zeros((2, 70), dtype=torch.int64))),
    ("state", "2E + C - 1 cells", lambda: dict(state=torch.zeros((2, 69), dtype=torch.int32))),
    ("state", "one plane", lambda: dict(state=torch.zeros((1, 70), dtype=torch.int32))),
    ("state", "flat", lambda: dict(state=torch.zeros(140, dtype=torch.int32))),
    ("state", "strided", lambda: dict(state=torch.zeros((2, 140), dtype=torch.int32)[:, ::2])),
    ("max_edges", "negative", lambda: dict(max_edges=-1)),
    ("max_edges", "beyond E", lambda: dict(max_edges=31)),
    ("max_edges", "a float", lambda: dict(max_edges=5.0)),
    ("max_edges", "a bool", lambda: dict(max_edges=True)),
]


@pytest.mark.parametrize("arg,what,make", VIOLATIONS, ids=[f"{a}: {w}" for a, w, _ in VIOLATIONS])
def test_violation_is_refused_before_anything_reaches_the_library(arg, what, make, stub):
    with pytest.raises(ValueError) as err:
        stub.runtime.eval_ranks(**dict(_ok(), **make()))
    msg = str(err.value)
    assert msg.startswith("eval_ranks: ") and re.search(rf"(?<![\w]){re.escape(arg)}(?![\w\[])", msg), msg
    assert "must be" in msg and "got" in msg, msg
    assert stub.rec.calls == [] and stub.log == [] and stub.ptrs == [], (stub.rec.calls, stub.log)


def test_device_mismatch_is_refused(monkeypatch):
    from ovmr_amd import runtime
    rec = _Recorder()
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    with pytest.raises(ValueError, match="eval_ranks: mo must be on cuda"):
        runtime.eval_ranks(**_ok())
    assert rec.calls == []


def test_accepted_calls_hand_over_what_the_header_asks(stub, lib):
    rt = stub.runtime
    big = torch.zeros((6, 13), dtype=torch.float32)
    a = _ok(dtype=torch.float32)
    a["mo"] = big[1:5, :10]
    rt.eval_ranks(**a)
    (name, g), = stub.rec.calls
    assert name == "ovmr_eval_ranks" and len(g) == 12
    assert g[0].value == big[1:5].data_ptr() and g[1:3] == (rt.F32, 13), "a row view goes as it is, with its stride"
    assert g[3].value == a["labels"].data_ptr() and g[4:6] == (4, 10) and g[6].value == a["edges"].data_ptr()
    assert g[7].value == a["estart"].data_ptr() and g[8:10] == (30, 5) and g[10].value == a["state"].data_ptr()
    assert [t.data_ptr() for t in stub.ptrs] == [g[0].value, g[3].value, g[6].value, g[7].value, g[10].value], "every address went through runtime._ptr"
    assert a["state"].numel() == lib.ovmr_eval_ranks_state_cells(10, 30), "the state covers what the header derives from C and E"
    stub.rec.calls.clear()
    rt.eval_ranks(**_ok(B=1, E=0))                              # one row, no positive in the pass: ld is at least C, edges go as NULL
    g = stub.rec.calls[0][1]
    assert g[1:3] == (rt.F16, 10) and g[4:6] == (1, 10) and g[6] is None and g[8:10] == (0, 0)
    stub.rec.calls.clear()
    rt.eval_ranks(**_ok(B=0))                                   # an empty batch launches nothing
    assert stub.rec.calls == []


# ---- the figures -------------------------------------------------------------------------------------------------------------------------

TOL = 1e-12           # a figure is a sum of at most P fp64 ratios in [0, 1], P <= 4096: 4096 x 2^-52 = 9e-13


def _sets():
    """name -> (scores [n, C] fp32 torch, labels [n]): continuous and heavily tied, finite."""
    g = torch.Generator().manual_seed(7)
    n, C = 400, 40
    y = torch.randint(0, C, (n,), generator=g)
    cont = torch.randn((n, C), generator=g)
    cont[torch.arange(n), y] += 1.0
    soft = torch.softmax(cont * 2, dim=1)
    tied = torch.round(cont * 2) / 2                             # a dozen distinct values
    coarse = (cont > 0.3).float()                                # two
    few = torch.randint(0, 3, (n,), generator=g)                 # 3 of 40 classes present: skips counted below
    return {"continuous": (cont, y), "softmax": (soft, y), "tied": (tied, y), "two values": (coarse, y), "fp16": (cont.half().float(), y),
            "few classes": (tied[:, :3].contiguous(), few)}


def _evaluator(C, **kw):
    from ovmr_amd.evaluator import Classification
    return Classification(C, [f"class {i}, the" if i == 1 else f"c{i}" for i in range(C)], device="cpu", exact=True, **kw)


@pytest.mark.parametrize("name", ["continuous", "softmax", "tied", "two values", "fp16", "few classes"])
def test_figures_are_sklearns_on_the_raw_scores(name):
    from sklearn.metrics import average_precision_score, precision_recall_curve, roc_auc_score
    mo, y = _sets()[name]
    n, C = mo.shape
    assert torch.isfinite(mo).all()
    ev = _evaluator(C)
    for a in range(0, n, 150):
        ev.process(mo[a:a + 150], y[a:a + 150])
    ev.evaluate(report=False)
    fig, skipped, worst = ev.ranks, 0, 0.0
    for c in range(C):
        t, s = (y == c).numpy().astype(int), mo[:, c].double().numpy()
        assert fig["positives"][c] == t.sum() and fig["negatives"][c] == n - t.sum() and t.sum() <= 4096
        if t.sum() == 0 or t.sum() == n:
            skipped += 1
            assert np.isnan(fig["auroc"][c]) and (t.sum() > 0 or np.isnan(fig["ap"][c]))
            continue
        p, r, thr = precision_recall_curve(t, s)
        f1 = 2 * p * r / np.maximum(p + r, 1e-300)
        want = dict(ap=average_precision_score(t, s), auroc=roc_auc_score(t, s), best_f1=f1.max())
        for k, w in want.items():
            d = abs(fig[k][c] - w)
            print(f"{name}: class {c} {k} {fig[k][c]!r} sklearn {w!r} diff {d:.3e}")
            worst = max(worst, d)
            assert d <= TOL, (c, k, fig[k][c], w)
        assert fig["threshold"][c] in thr and float(fig["threshold"][c]) in s[t == 1], "the threshold is a positive's own score"
        hit = s >= fig["threshold"][c]
        assert fig["precision"][c] == (hit & (t == 1)).sum() / hit.sum() and fig["recall"][c] == (hit & (t == 1)).sum() / t.sum()
    print(f"{name}: {skipped} of {C} classes skipped, worst difference {worst:.3e}")
    assert skipped <= C // 10, f"{skipped} of {C} classes have no positive or no negative"


def test_best_f1_and_its_tie_rule():
    from ovmr_amd.evaluator import rank_figures
    # class 0, edges 0.9 0.5, cells 0..4: two positives at 0.9, one at 0.5, seven negatives below both.  The cut at 0.9 has p 1, r 2/3
    # (F1 0.8), the cut at 0.5 p 1, r 1 (F1 1).  class 1, edges 0.8 0.6 0.2, cells 5..11: a positive at each, one negative tied with 0.8:
    # F1 is 2/5, 4/6, 6/7 down the edges.  class 2 has no positive
    edges, estart = torch.tensor([0.9, 0.5, 0.8, 0.6, 0.2]), torch.tensor([0, 2, 5, 5], dtype=torch.int32)
    st = np.zeros((2, 2 * 5 + 3), dtype=np.int64)
    st[1, [1, 3]], st[0, 4] = (2, 1), 7
    base = 2 * 2 + 1
    st[1, [base + 1, base + 3, base + 5]] = 1
    st[0, base + 1] = 1
    f = rank_figures(st, edges, estart)
    assert f["best_f1"][0] == 1.0 and f["threshold"][0] == 0.5 and f["precision"][0] == 1.0 and f["recall"][0] == 1.0
    assert f["ap"][0] == 1.0 and f["auroc"][0] == 1.0 and f["positives"].tolist() == [3, 3, 0] and f["negatives"].tolist() == [7, 1, 0]
    assert f["best_f1"][1] == 6 / 7 and f["threshold"][1] == np.float32(0.2) and f["recall"][1] == 1.0 and f["precision"][1] == 0.75
    assert f["auroc"][1] == (0.5 + 0 + 0) / 3 and f["ap"][1] == (1 / 2 + 2 / 3 + 3 / 4) / 3
    assert all(np.isnan(f[k][2]) for k in ("ap", "auroc", "best_f1", "threshold", "precision", "recall")), "no positive: no figure"
    two = (torch.tensor([2.0, 1.0]), torch.tensor([0, 2], dtype=torch.int32))
    st2 = np.zeros((2, 5), dtype=np.int64)                       # one class, edges 2 > 1: a positive at each, a negative between them
    st2[1, [1, 3]], st2[0, 2] = 1, 1                             # the cut at 2: tp 1, fp 0 -> 2/3; at 1: tp 2, fp 1 -> 4/5
    f = rank_figures(st2, *two)
    assert f["best_f1"][0] == 0.8 and f["threshold"][0] == 1.0
    st2[0, 2], st2[0, 4], st2[1, 3] = 0, 5, 0                    # the one positive at 2, negatives below both edges: F1 is 1 at either cut
    f = rank_figures(st2, *two)
    assert f["best_f1"][0] == 1.0 and f["threshold"][0] == 2.0, "ties go to the higher threshold"
    # brute force: F1 at every edge, the highest threshold among the best
    rng = np.random.default_rng(2)
    n = 8
    st3 = np.zeros((2, 2 * n + 1), dtype=np.int64)
    for _ in range(50):
        st3[0] = rng.integers(0, 3, size=2 * n + 1)
        st3[1, 1::2] = rng.integers(1, 3, size=n)
        ed = torch.arange(n, 0, -1).float()
        f = rank_figures(st3, ed, torch.tensor([0, n], dtype=torch.int32))
        P = st3[1].sum()
        f1 = [2 * st3[1, :2 * k + 2].sum() / (st3[1, :2 * k + 2].sum() + st3[0, :2 * k + 2].sum() + P) for k in range(n)]
        assert f["threshold"][0] == float(ed[min(k for k in range(n) if f1[k] == max(f1))]) and abs(f["best_f1"][0] - max(f1)) < 1e-15
    st2[1, 2] = 1
    with pytest.raises(ValueError, match="class 0 holds 1 positive.s. between its edges"):
        rank_figures(st2, *two)
    with pytest.raises(ValueError, match=r"state must be of shape \[2, 5\]"):
        rank_figures(st2[:, :4], *two)


# ---- the host evaluator ------------------------------------------------------------------------------------------------------------------

def _batches(C=6, n=(40, 1, 23), seed=0, present=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in n:
        y = torch.randint(0, C if present is None else present, (b,), generator=g)
        out.append((torch.softmax(torch.randn((b, C), generator=g) * 2, dim=1), y))
    return out


def test_host_evaluator_counts_what_the_reference_counts():
    C = 6
    ev = _evaluator(C)
    batches = _batches(n=(40, 1, 23, 64, 7))
    sp = torch.from_numpy(K.specials())
    batches[0][0].view(-1)[:len(sp)] = sp                        # NaN, infinities, zeros of both signs, denormals among the scores
    for mo, y in batches:
        ev.process(mo, y)
    assert len(ev._kept) == 5 and ev._kept_bytes == 135 * 6 * 4 and ev._kept[0][0].data_ptr() != batches[0][0].data_ptr(), "a copy of its own"
    ev.count_ranks()
    assert ev._kept == [] and ev._kept_bytes == 0, "the kept scores are freed"
    mo, y = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches])
    edges, estart = K.edges_of(mo, y, C)
    got_e, got_s, state = ev._rank
    assert got_e.numpy().view(np.uint32).tolist() == edges.view(np.uint32).tolist() and got_s.tolist() == estart.tolist()
    assert state.dtype == torch.int32 and K.mismatch(state, K.expected(mo, y, edges, estart)) is None
    assert int(state[1].sum()) == 135 and not bool(state[1].view(-1)[[2 * int(estart[c]) + c + 2 * k for c in range(C)
                                                                    for k in range(int(estart[c + 1] - estart[c]) + 1)]].any())
    with pytest.raises(ValueError, match="after the exact figures of the pass were counted"):
        ev.process(*batches[0])
    ev.reset()
    ev.process(*batches[1])
    assert len(ev._kept) == 1 and ev._rank is None


def test_states_add_across_cuts_orders_and_ranks():
    from ovmr_amd.evaluator import Classification
    C = 6
    batches = _batches(n=(40, 1, 23, 64, 7))
    whole = _evaluator(C)
    for mo, y in batches:
        whole.process(mo, y)
    whole.count_ranks()
    rev = _evaluator(C)
    mo, y = torch.cat([b[0] for b in batches][::-1]), torch.cat([b[1] for b in batches][::-1])
    for a in range(0, 135, 9):
        rev.process(mo[a:a + 9], y[a:a + 9])
    rev.count_ranks()
    for a, b in zip(whole._rank, rev._rank):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same bytes from any cut and order"

    # three ranks in one process, rank 2 without a batch: the gathers answer with what every rank would have sent
    ranks = [_evaluator(C) for _ in range(3)]
    for i, (mo, y) in enumerate(batches):
        ranks[i % 2].process(mo, y)
    ranks[2].begin()
    parts = []
    for ev in ranks:
        s = [m.gather(1, g.unsqueeze(1)).squeeze(1) for m, g in ev._kept]
        parts.append((torch.cat(s), torch.cat([g for _, g in ev._kept])) if s else (torch.zeros(0), torch.zeros(0, dtype=torch.int64)))
    log = []

    class Group:
        def get_backend(self): return "gloo"
        def get_world_size(self): return 3

        def all_gather_into_tensor(self, out, t):
            log.append(("gather", tuple(t.shape)))
            if t.numel() == 1:
                out.copy_(torch.tensor([len(p[0]) for p in parts]))
                return
            rows = out.view(3, t.shape[0], 2)
            rows.fill_(-7)                                       # (what lies beyond a rank's length is never read)
            for r, (sc, g) in enumerate(parts):
                rows[r, :len(sc), 0] = sc.view(torch.int32).long()
                rows[r, :len(sc), 1] = g

        def all_reduce(self, t): log.append(("reduce", tuple(t.shape)))

    from ovmr_amd import shard
    sc, g = shard.all_gather_positives(*parts[0], Group())
    assert len(sc) == 135 and sc.dtype == torch.float32 and g.dtype == torch.int64
    assert torch.equal(sc.view(torch.int32), torch.cat([p[0] for p in parts]).view(torch.int32)) and torch.equal(g, torch.cat([p[1] for p in parts]))
    del log[:]
    Classification.all_reduce(ranks, Group())
    E = int(whole._rank[1][-1])
    longest = max(len(p[0]) for p in parts)
    assert log == [("reduce", (3 * (3 * C + 1),))] + [("gather", (1,)), ("gather", (longest, 2)), ("reduce", (2, 2 * E + C))] * 3
    for ev in ranks:
        assert torch.equal(ev._rank[0].view(torch.int32), whole._rank[0].view(torch.int32)) and torch.equal(ev._rank[1], whole._rank[1])
        assert ev._kept == []
    states = [ev._rank[2] for ev in ranks]
    assert torch.equal(states[0] + states[1] + states[2], whole._rank[2]) and not bool(states[2].any()) and bool(states[1].any())
    del log[:]
    Classification.all_reduce(ranks[:1], Group())
    assert log == [("reduce", (3 * C + 1,))] and torch.equal(ranks[0]._rank[2], states[0]), "counted already: not counted twice"


def test_results_files_and_empty_fields(tmp_path, capsys):
    from ovmr_amd.evaluator import RANK_COLUMNS, Classification
    C = 6
    ev = _evaluator(C, curves=16)
    plain = Classification(C, ev.classnames, device="cpu", curves=16)
    for mo, y in _batches(present=4):                           # classes 4 and 5 have no image
        ev.process(mo, y)
        plain.process(mo, y)
    res0 = plain.evaluate(str(tmp_path / "plain"))
    before = capsys.readouterr().out
    res = ev.evaluate(str(tmp_path / "out"))
    after = capsys.readouterr().out
    assert after.startswith(before) and list(res)[:5] == list(res0) and list(res)[5:] == ["exact_mAP", "exact_mean_auroc"]
    assert all(res[k] == v for k, v in res0.items())
    assert after[len(before):].splitlines() == [f"* exact_mAP: {res['exact_mAP']:.1f}%", f"* exact_mean_auroc: {res['exact_mean_auroc']:.4f}"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert sorted(os.listdir(tmp_path / "out")) == sorted(names + ["ranks_per_class.csv", "rank_state.pt"])
    for name in names:
        if name.endswith(".csv"):
            assert (tmp_path / "out" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), "--score-curves beside the new flag is unchanged"
    assert torch.equal(torch.load(tmp_path / "out" / "score_hist.pt")["hist"], torch.load(tmp_path / "plain" / "score_hist.pt")["hist"])
    fig = ev.ranks
    assert res["exact_mAP"] == 100.0 * float(np.mean(fig["ap"][:4])) and res["exact_mean_auroc"] == float(np.mean(fig["auroc"][:4]))
    rows = list(csv.reader(open(tmp_path / "out" / "ranks_per_class.csv")))
    assert rows[0] == RANK_COLUMNS == ["label", "classname", "positives", "negatives", "ap", "auroc", "best_f1", "threshold", "precision", "recall"]
    assert len(rows) == 7 and rows[2][:2] == ["1", "class 1, the"]
    for c in range(4):
        r = rows[1 + c]
        assert [int(r[2]), int(r[3])] == [int(fig["positives"][c]), int(fig["negatives"][c])] and int(r[2]) + int(r[3]) == 64
        assert [float(v) for v in r[4:]] == [fig[k][c] for k in ("ap", "auroc", "best_f1", "threshold", "precision", "recall")]
    for c in (4, 5):
        assert rows[1 + c][2:] == ["0", "64"] + [""] * 6, "a class without an image has no figure"
    saved = torch.load(tmp_path / "out" / "rank_state.pt")
    assert set(saved) == {"edges", "estart", "state", "classnames"} and saved["classnames"] == ev.classnames
    E = int(saved["estart"][-1])
    assert saved["edges"].dtype == torch.float32 and saved["edges"].shape == (E,) and saved["estart"].dtype == torch.int32
    assert saved["state"].dtype == torch.int64 and saved["state"].shape == (2, 2 * E + C) and int(saved["state"].sum()) == 64 * C
    assert all(torch.equal(a, b) for a, b in zip(ev.rank_state, (saved["edges"], saved["estart"], saved["state"])))
    one = _evaluator(1)                                          # no negative: one class only
    one.process(torch.rand(5, 1), torch.zeros(5, dtype=torch.int64))
    r = one.evaluate(str(tmp_path / "one"))
    assert r["exact_mAP"] == 100.0 and r["exact_mean_auroc"] == 0.0
    row = list(csv.reader(open(tmp_path / "one" / "ranks_per_class.csv")))[1]
    assert row[2:6] == ["5", "0", "1.0", ""] and row[6] == "1.0"
    quiet = _evaluator(C)                                        # report=False: figures, no file
    quiet.process(*_batches()[0])
    capsys.readouterr()
    assert "exact_mAP" in quiet.evaluate(str(tmp_path / "quiet"), report=False) and capsys.readouterr().out == "" and not (tmp_path / "quiet").exists()
    empty = _evaluator(C)                                        # a pass without a batch
    assert empty.evaluate(report=False)["exact_mAP"] == 0.0 and empty._rank[2].shape == (2, C)


def test_off_means_off_byte_for_byte(tmp_path, capsys, monkeypatch):
    from ovmr_amd import evaluator, runtime
    from ovmr_amd.evaluator import Classification
    called = []
    for name in ("rank_edges", "rank_cells", "rank_count", "rank_figures"):
        monkeypatch.setattr(evaluator, name, lambda *a, _n=name, **k: called.append(_n))
    monkeypatch.setattr(runtime, "eval_ranks", lambda *a, **k: called.append("eval_ranks"))
    outs = {}
    for key, kw in (("default", {}), ("off", dict(exact=False, exact_max_bytes=0))):
        ev = Classification(6, device="cpu", per_class=True, confusion=True, curves=16, **kw)
        for mo, y in _batches():
            ev.process(mo, y)
        assert ev._kept == [] and ev._kept_bytes == 0 and ev._rank is None
        res = ev.evaluate(str(tmp_path / key))
        text = capsys.readouterr().out.replace(str(tmp_path / key), "OUT")
        outs[key] = (list(res.items()), text, {n: (tmp_path / key / n).read_bytes() for n in sorted(os.listdir(tmp_path / key)) if n.endswith(".csv")})
        assert ev.ranks is None and ev.rank_state is None and not any("exact" in k for k in res) and "exact" not in text
        assert sorted(os.listdir(tmp_path / key)) == ["acc_per_class.csv", "cmat.pt", "curves_per_class.csv", "f1_per_class.csv", "score_hist.pt"]
    assert outs["default"] == outs["off"] and called == []
    p = inspect.signature(Classification.__init__).parameters
    assert p["exact"].default is False and p["exact_max_bytes"].default == 16 << 30
    for kw, msg in ((dict(exact=1), "exact must be True or False"), (dict(exact=True, exact_max_bytes=-1), "exact_max_bytes must be"),
                    (dict(exact=True, exact_max_bytes=1.5), "exact_max_bytes must be")):
        with pytest.raises(ValueError, match=msg):
            Classification(6, device="cpu", **kw)


def test_budget_refusal_names_both_figures():
    ev = _evaluator(6, exact_max_bytes=40 * 6 * 4 + 1 * 6 * 4)
    (a, ya), (b, yb), (c, yc) = _batches()
    ev.process(a, ya)
    ev.process(b, yb)                                           # exactly at the budget
    with pytest.raises(ValueError) as err:
        ev.process(c, yc)
    assert "1,536 bytes" in str(err.value) and "exact_max_bytes = 984" in str(err.value) and str(err.value).startswith("Classification(exact=True)")
    assert len(ev._kept) == 2 and ev._kept_bytes == 984
    half = _evaluator(6, exact_max_bytes=40 * 6 * 2)            # fp16 outputs are kept as fp16
    half.process(a.half(), ya)
    assert half._kept[0][0].dtype == torch.float16 and half._kept_bytes == 480


def test_trainers_share_the_keyword():
    from ovmr_amd import trainer
    for cls in (trainer.MM_CLS_OP, trainer.ZeroshotCLIP, trainer.ZeroshotCLIP2):
        p = inspect.signature(cls.__init__).parameters
        assert p["exact_curves"].default is False and p["exact_max_bytes"].default is None
        names = list(p)
        assert names.index("score_range") < names.index("exact_curves") < names.index("exact_max_bytes")


# ---- the runner --------------------------------------------------------------------------------------------------------------------------

def test_runner_refusals():
    from ovmr_amd import cli
    w = ["--clip-weights", "clip.pt"]
    x = w + ["--exact-curves"]
    assert cli.check_exact_curves(cli.parse(w)) == (False, None)
    assert cli.check_exact_curves(cli.parse(x)) == (True, 16 << 30) and cli.DEFAULT_EXACT_GIB == 16.0
    assert cli.check_exact_curves(cli.parse(x + ["--exact-budget", "0.5"])) == (True, 1 << 29)
    for argv, msg in (
            (x + ["--predict", "pics"], "--exact-curves belongs to the test pass: --predict reads unlabelled images, a score has no label to be held against"),
            (x + ["--retrieve", "pool"], "--exact-curves belongs to the test pass: --retrieve reads unlabelled images, a score has no label to be held against"),
            (w + ["--exact-budget", "4"], "--exact-budget GIB belongs to --exact-curves: the memory the kept scores of the test pass may take"),
            (x + ["--exact-budget", "0"], "--exact-budget 0.0: GIB must be a positive number of GiB"),
            (x + ["--exact-budget", "-1"], "--exact-budget -1.0: GIB must be a positive number of GiB"),
            (x + ["--exact-budget", "nan"], "--exact-budget nan: GIB must be a positive number of GiB"),
            (x + ["--exact-budget", "inf"], "--exact-budget inf: GIB must be a positive number of GiB")):
        with pytest.raises(SystemExit) as err:
            cli.check_exact_curves(cli.parse(argv))
        assert str(err.value) == msg
    # main refuses before anything is listed or loaded: the paths do not exist, the weights do not exist
    base = ["--eval-only", "--eval_mode", "fusion"]
    for trainer, argv, msg in (("MM_CLS_OP", x + ["--predict", "pics"], "--exact-curves belongs to the test pass: --predict"),
                               ("ZeroshotCLIP", x + ["--retrieve", "pool"], "--exact-curves belongs to the test pass: --retrieve"),
                               ("MM_CLS_OP", w + ["--exact-budget", "2"], "--exact-budget GIB belongs to --exact-curves"),
                               ("ZeroshotCLIP2", x + ["--exact-budget", "0"], "GIB must be a positive number")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(base + ["--trainer", trainer] + argv)
    # the zero-shot trainers need no range, and the plan carries the flag
    from ovmr_amd import config
    for trainer in ("ZeroshotCLIP", "ZeroshotCLIP2", "MM_CLS_OP"):
        args = cli.parse(["--clip-weights", "none.pt", "--root", "nowhere", "--exact-curves", "--exact-budget", "2", "--eval-only", "--trainer",
                          trainer, "DATASET.NAME", "Caltech101", "DATASET.NUM_SHOTS", "2"])
        p = cli.plan_job(args, config.setup_cfg(args))
        assert (p.mode, p.exact, p.exact_bytes, p.curve_bins) == ("test", True, 2 << 30, None)
    args = cli.parse(["--clip-weights", "none.pt", "--root", "nowhere", "--eval-only", "--trainer", "MM_CLS_OP", "DATASET.NUM_SHOTS", "2"])
    p = cli.plan_job(args, config.setup_cfg(args))
    assert (p.exact, p.exact_bytes) == (False, None)
