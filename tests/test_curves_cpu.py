"""Score curves without a GPU: the reference of curves_cases.py against itself, the comparator against planted defects, the header against
runtime.CURVES_SIGNATURES and the library's exports, the argument errors through the loaded library, the Python boundary of
runtime.eval_curves, the host evaluator against sklearn, the files, and the runner's refusals."""
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

import curves_cases as K
from conftest import REPO

INF, NAN = math.inf, math.nan


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

ALL_CASES = [(lo, hi, b) for lo, hi in K.RANGES for b in K.BINS] + K.CLAMP_CASES + K.NO_CLAMP_CASES


@pytest.mark.parametrize("lo,hi,bins", ALL_CASES)
def test_reference_equals_its_literal_restatement_on_the_edge_table(lo, hi, bins):
    for fp16 in (False, True):
        v = K.edge_table(lo, hi, bins, fp16)
        got = K.slots(v, lo, hi, bins)
        want = [K.slot_literal(x, lo, hi, bins) for x in v]
        assert got.tolist() == want
        assert set(got.tolist()) >= {0, bins + 1, bins + 2, 1}, "the table reaches both outer slots, the NaN slot and the first bin"
        assert fp16 or bins in got, "and the last bin (an fp16 below hi need not reach it: 1 - 2^-11 lies in bin 4095 of 4096)"
        assert got.min() >= 0 and got.max() == bins + 2


def test_edge_table_holds_what_the_issue_lists():
    v = K.edge_table(0.0, 1.0, 7)
    bits = set(v.view(np.uint32).tolist())
    f = lambda x: int(np.array([x], dtype=np.float32).view(np.uint32)[0])
    for x in (0.0, -0.0, 1.0, INF, -INF, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)),
              np.nextafter(np.float32(0), np.float32(1)), np.nextafter(np.float32(0), np.float32(-1))):
        assert f(x) in bits, x
    assert 0x7FC00000 in bits and 0xFFC00000 in bits, "NaN of both signs"
    assert 0x00000001 in bits and 0x80000001 in bits, "a denormal of either sign"
    s = K.slots(v, 0.0, 1.0, 7)
    by = dict(zip(v.view(np.uint32).tolist(), s.tolist()))
    assert by[f(-0.0)] == 1 and by[f(0.0)] == 1 and by[0x00000001] == 1 and by[0x80000001] == 0, "-0.0 == +0.0; a denormal is not flushed"
    assert by[0x7FC00000] == by[0xFFC00000] == 9 and by[f(INF)] == 8 and by[f(-INF)] == 0 and by[f(1.0)] == 8
    scale = K.scale_of(0.0, 1.0, 7)
    for j in range(8):
        e = np.float32(np.float32(j) / scale)
        for n in (np.nextafter(e, np.float32(-INF)), e, np.nextafter(e, np.float32(INF))):
            assert f(n) in bits, (j, n)
    h = K.edge_table(0.0, 1.0, 256, fp16=True)
    assert all(np.float32(j / 256) in h for j in range(65)), "fp16 inputs that are exact edges"
    assert np.array_equal(K.slots(np.arange(256, dtype=np.float32) / 256, 0.0, 1.0, 256), 1 + np.arange(256))


def test_the_min_is_not_decoration():
    for cases, clamps in ((K.CLAMP_CASES, True), (K.NO_CLAMP_CASES, False)):
        for lo, hi, bins in cases:
            x = np.nextafter(np.float32(hi), np.float32(-INF))
            t = np.float32(np.float32(x - np.float32(lo)) * K.scale_of(lo, hi, bins))
            assert (t == bins) == clamps, (lo, hi, bins, t)
            assert K.slots(x, lo, hi, bins) == bins and K.slot_literal(x, lo, hi, bins) == bins


@pytest.mark.parametrize("lo,hi", K.RANGES)
def test_reference_is_monotone(lo, hi):
    rng = np.random.default_rng(5)
    w = hi - lo
    x = np.sort(np.concatenate([rng.uniform(lo - 0.05 * w, hi + 0.05 * w, 199_000).astype(np.float32), K.edge_table(lo, hi, 4096)[:1000]]))
    x = x[~np.isnan(x)][:200_000]
    assert len(x) >= 199_000
    for bins in K.BINS + [1000]:
        s = K.slots(x, lo, hi, bins)
        assert (np.diff(s) >= 0).all(), (lo, hi, bins)
        assert s[0] == 0 and s[-1] == bins + 1


# ---- the comparator and the planted defects --------------------------------------------------------------------------------------------

# name -> (B, C, lo, hi, bins, fp16, label kind): the GPU tests' own sizes -- a partial last chunk of rows, a partial last tile of classes
CASES = {
    "interior edges": (130, 33, 0.1, 0.7, 7, False, "random"),
    "clamp": (65, 17, -100.0, 100.0, 1024, False, "random"),
    "around zero": (130, 17, 0.0, 1.0, 256, False, "bad"),
    "fp16": (65, 33, 0.0, 1.0, 256, True, "hot"),
}
REJECTED_ON = {"fma": "interior edges", "no_min": "clamp", "neg_zero_under": "around zero", "bad_label_negative": "around zero"}


def _run(case, defect=None):
    B, C, lo, hi, bins, fp16, kind = CASES[case]
    out, y = K.scores(B, C, lo, hi, bins, fp16, seed=3), K.labels(B, C, kind, seed=3)
    before = K.random_state(C, bins, seed=3)
    got = K.model(out, y, lo, hi, bins, before.clone(), defect)
    return K.mismatch(got, K.expected(out, y, lo, hi, bins, before))


@pytest.mark.parametrize("case", sorted(CASES))
def test_honest_model_passes(case):
    assert _run(case) is None


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_defect_is_rejected(defect):
    case = REJECTED_ON.get(defect, "interior edges")
    msg = _run(case, defect)
    assert msg is not None and "cells differ" in msg, f"{defect} passes on {case!r}"


def test_mismatch_reads():
    a = torch.zeros((3, 2, 5), dtype=torch.int32)
    b = a.clone()
    assert K.mismatch(a, b) is None and "shape" in K.mismatch(a, b[:2])
    b[1, 1, 4] = 2
    assert K.mismatch(a, b) == "1 of 30 cells differ, the first at class 1, plane 1, slot 4 of 5: got 0, expected 2"


def test_model_constants_are_the_kernels():
    src = open(os.path.join(REPO, "ovmr_amd", "csrc", "eval_curves.hip")).read()
    for name, want in (("EC_TILE", K.TILE), ("EC_ROWS", K.CHUNK), ("EC_MAX_ROW_BLOCKS", K.MAX_ROW_BLOCKS), ("EC_MAX_BINS", K.MAX_BINS)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == want, name
    assert '#include "eval_common.h"' in src and "wave_histogram_add(" in src and "topk_key(" in src
    assert "wave_histogram_add(int*" not in src and "topk_key(float" not in src, "the helpers are shared through eval_common.h, not copied"
    for case in CASES.values():
        assert case[0] % K.CHUNK and case[0] > K.CHUNK and case[1] % K.TILE and case[1] > K.TILE
    from ovmr_amd import runtime, cli
    assert runtime.MAX_BINS == cli.MAX_BINS == K.MAX_BINS


# ---- the header, its table and the library ---------------------------------------------------------------------------------------------

NAMES = {"ovmr_eval_curves_state_bytes", "ovmr_eval_curves"}


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import build, runtime
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    return runtime.load_library()


def test_curves_header_table_and_exports(lib):
    from ovmr_amd import build, runtime
    text = open(os.path.join(REPO, "include", "ovmr_hip_curves.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = dict(re.findall(r"\b(ovmr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(decls) == set(runtime.CURVES_SIGNATURES) == NAMES
    assert not set(runtime.CURVES_SIGNATURES) & (set(runtime.SIGNATURES) | set(runtime.EXT_SIGNATURES) | set(runtime.AUDIT_SIGNATURES)
                                                 | set(runtime.RETRIEVE_SIGNATURES))
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    for name, params in decls.items():
        res, args = runtime.CURVES_SIGNATURES[name]
        assert hasattr(lib, name), f"{name} declared in include/ovmr_hip_curves.h but not exported"
        want = [ctypes.c_void_p if "*" in p or "ovmr_stream" in p else ctype[p.split()[0]] for p in (q.strip() for q in params.split(","))]
        assert args == want, f"{name}: {args} != {want}"
        assert res is (ctypes.c_long if name == "ovmr_eval_curves_state_bytes" else ctypes.c_int)
        assert getattr(lib, name).argtypes == args
    assert text.count("No counterpart in the reference") == 2
    flat = " ".join(re.sub(r"\n \* ?", " ", text).split())
    for phrase in ("ALL-ZERO BYTES ARE THE EMPTY STATE", "fewer than 2^31 images", "NON-DECREASING", "never used as an address",
                   "no fused multiply-add", "-0.0 == +0.0"):
        assert phrase in flat, phrase
    assert "ovmr_hip_curves.h" in inspect.getsource(build.build), "the build lists the header among its dependencies"
    for other in ("ovmr_hip.h", "ovmr_hip_nearest.h", "ovmr_hip_audit.h", "ovmr_hip_retrieve.h"):
        assert "curves" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", other)).read(), flags=re.S)


def test_state_bytes_and_argument_errors(lib):
    f = lib.ovmr_eval_curves_state_bytes
    for C, bins in ((1, 1), (1000, 256), (21841, 4096), (65, 7)):
        assert f(C, bins) == C * 2 * (bins + 3) * 4
    assert f(21841, 4096) == 716_210_072
    for C, bins in ((0, 5), (-1, 5), (5, 0), (5, 4097), (5, -1)):
        assert f(C, bins) == -1
    E_ARG = -1
    o, y, s = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000))       # never dereferenced
    ok = dict(out=o, f32=0, ld=10, labels=y, B=4, C=10, lo=0.0, hi=1.0, bins=16, state=s)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ovmr_eval_curves(a["out"], a["f32"], a["ld"], a["labels"], a["B"], a["C"], a["lo"], a["hi"], a["bins"], a["state"], None)

    big = float(np.finfo(np.float32).max)
    for kw in (dict(out=None), dict(labels=None), dict(state=None), dict(bins=0), dict(bins=4097), dict(C=0), dict(B=-1), dict(ld=9),
               dict(out=ctypes.c_void_p(0x10001)), dict(out=ctypes.c_void_p(0x10002), f32=1), dict(labels=ctypes.c_void_p(0x20004)),
               dict(state=ctypes.c_void_p(0x30002)), dict(lo=NAN), dict(hi=NAN), dict(lo=-INF), dict(hi=INF), dict(lo=1.0), dict(lo=2.0),
               dict(lo=-big, hi=big), dict(lo=0.0, hi=1e-45, bins=4096)):
        assert call(**kw) == E_ARG, kw
        assert call(**dict(dict(B=0), **kw)) == E_ARG, ("B == 0 excuses no argument", kw)
    assert call(B=0) == 0 and call(B=0, f32=1) == 0 and call(B=0, out=ctypes.c_void_p(0x10002)) == 0 and call(B=0, lo=-0.0, hi=1e-30) == 0


# ---- the Python boundary of runtime.eval_curves ------------------------------------------------------------------------------------------

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


def _ok(B=4, C=10, bins=16, dtype=torch.float16):
    return dict(mo=torch.zeros((B, C), dtype=dtype), labels=torch.zeros(B, dtype=torch.int64), lo=0.0, hi=1.0, bins=bins,
                state=torch.zeros((C, 2, bins + 3), dtype=torch.int32))


VIOLATIONS = [
    ("mo", "three dimensions", lambda: dict(mo=torch.zeros((4, 2, 10), dtype=torch.float16))),
    ("mo", "fp64", lambda: dict(mo=torch.zeros((4, 10), dtype=torch.float64))),
    ("mo", "a column stride", lambda: dict(mo=torch.zeros((4, 20), dtype=torch.float16)[:, ::2])),
    ("mo", "an expanded row", lambda: dict(mo=torch.zeros((1, 10), dtype=torch.float16).expand(4, 10))),
    ("mo", "a numpy array", lambda: dict(mo=np.zeros((4, 10), dtype=np.float16))),
    ("mo", "no column", lambda: dict(mo=torch.zeros((4, 0), dtype=torch.float16), state=torch.zeros((0, 2, 19), dtype=torch.int32))),
    ("labels", "int32", lambda: dict(labels=torch.zeros(4, dtype=torch.int32))),
    ("labels", "a row short", lambda: dict(labels=torch.zeros(3, dtype=torch.int64))),
    ("labels", "two dimensions", lambda: dict(labels=torch.zeros((4, 1), dtype=torch.int64))),
    ("labels", "strided", lambda: dict(labels=torch.zeros(8, dtype=torch.int64)[::2])),
    ("state", "int64", lambda: dict(state=torch.zeros((10, 2, 19), dtype=torch.int64))),
    ("state", "another C", lambda: dict(state=torch.zeros((11, 2, 19), dtype=torch.int32))),
    ("state", "bins + 2 slots", lambda: dict(state=torch.zeros((10, 2, 18), dtype=torch.int32))),
    ("state", "one plane", lambda: dict(state=torch.zeros((10, 1, 19), dtype=torch.int32))),
    ("state", "flat", lambda: dict(state=torch.zeros(10 * 2 * 19, dtype=torch.int32))),
    ("state", "strided", lambda: dict(state=torch.zeros((10, 2, 38), dtype=torch.int32)[:, :, ::2])),
    ("bins", "zero", lambda: dict(bins=0, state=torch.zeros((10, 2, 3), dtype=torch.int32))),
    ("bins", "4097", lambda: dict(bins=4097, state=torch.zeros((10, 2, 4100), dtype=torch.int32))),
    ("bins", "a float", lambda: dict(bins=16.0)),
    ("bins", "a bool", lambda: dict(bins=True, state=torch.zeros((10, 2, 4), dtype=torch.int32))),
    ("lo", "NaN", lambda: dict(lo=NAN)),
    ("lo", "-inf", lambda: dict(lo=-INF)),
    ("lo", "a string", lambda: dict(lo="0")),
    ("hi", "inf", lambda: dict(hi=INF)),
    ("hi", "beyond fp32", lambda: dict(hi=1e39)),
    ("hi", "equal to lo", lambda: dict(lo=1.0)),
    ("hi", "below lo", lambda: dict(lo=2.0)),
    ("hi", "equal to lo as fp32", lambda: dict(lo=1.0, hi=1.0 + 1e-9)),
    ("hi", "a range whose width overflows", lambda: dict(lo=-3e38, hi=3e38)),
]


@pytest.mark.parametrize("arg,what,make", VIOLATIONS, ids=[f"{a}: {w}" for a, w, _ in VIOLATIONS])
def test_violation_is_refused_before_anything_reaches_the_library(arg, what, make, stub):
    with pytest.raises(ValueError) as err:
        stub.runtime.eval_curves(**dict(_ok(), **make()))
    msg = str(err.value)
    assert msg.startswith("eval_curves: ") and re.search(rf"(?<![\w]){re.escape(arg)}(?![\w\[])", msg), msg
    assert "must be" in msg and "got" in msg, msg
    assert stub.rec.calls == [] and stub.log == [] and stub.ptrs == [], (stub.rec.calls, stub.log)


def test_device_mismatch_is_refused(monkeypatch):
    from ovmr_amd import runtime
    rec = _Recorder()
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    with pytest.raises(ValueError, match="eval_curves: mo must be on cuda"):
        runtime.eval_curves(**_ok())
    assert rec.calls == []


def test_accepted_calls_hand_over_what_the_header_asks(stub, lib):
    rt = stub.runtime
    big = torch.zeros((6, 13), dtype=torch.float32)
    a = _ok(dtype=torch.float32)
    a["mo"] = big[1:5, :10]
    rt.eval_curves(**dict(a, lo=0.1, hi=0.7))
    (name, g), = stub.rec.calls
    assert name == "ovmr_eval_curves" and len(g) == 11
    assert g[0].value == big[1:5].data_ptr() and g[1:3] == (rt.F32, 13), "a row view goes as it is, with its stride"
    assert g[3].value == a["labels"].data_ptr() and g[4:6] == (4, 10) and g[8] == 16 and g[9].value == a["state"].data_ptr()
    assert g[6] == float(np.float32(0.1)) and g[7] == float(np.float32(0.7)), "the range goes as the fp32 values that decide"
    assert [t.data_ptr() for t in stub.ptrs] == [g[0].value, g[3].value, g[9].value], "every address went through runtime._ptr"
    assert a["state"].numel() * 4 == lib.ovmr_eval_curves_state_bytes(10, 16), "the state covers what the header derives from C and bins"
    assert a["labels"].numel() == g[4] and (g[4] - 1) * g[2] + g[5] <= big[1:].numel()
    stub.rec.calls.clear()
    rt.eval_curves(**_ok(B=1, bins=4096))                      # one row: ld is at least C
    g = stub.rec.calls[0][1]
    assert g[1:3] == (rt.F16, 10) and g[4:6] == (1, 10) and g[8] == 4096
    stub.rec.calls.clear()
    rt.eval_curves(**_ok(B=0))                                 # an empty batch launches nothing
    assert stub.rec.calls == []


# ---- the host evaluator ------------------------------------------------------------------------------------------------------------------

def _sklearn_figures(hist):
    """ap and auroc of every class from sklearn, the slot index as the score, one sample per counted row."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    C, _, S = hist.shape
    ap, auc = np.full(C, NAN), np.full(C, NAN)
    for c in range(C):
        score = np.concatenate([np.repeat(np.arange(S), hist[c, 0]), np.repeat(np.arange(S), hist[c, 1])])
        y = np.concatenate([np.zeros(hist[c, 0].sum(), dtype=int), np.ones(hist[c, 1].sum(), dtype=int)])
        if y.sum():
            ap[c] = average_precision_score(y, score)
            if (1 - y).sum():
                auc[c] = roc_auc_score(y, score)
    return ap, auc


TOL = 1e-12           # both sides are fp64 sums of at most 4099 terms in [0, 1] taken in different orders: each within about 4.6e-13


def test_ap_and_auroc_are_sklearns():
    from ovmr_amd.evaluator import curve_figures
    rng = np.random.default_rng(11)
    for bins in (1, 7, 64):
        S = bins + 3
        hist = rng.integers(0, 6, size=(40, 2, S)).astype(np.int64)
        hist[rng.random(hist.shape) < 0.5] = 0
        hist[0, 1] = 0; hist[0, 1, 4 % S] = 1                   # one positive
        hist[1] = 0; hist[1, :, 2] = (7, 5)                     # all scores in one slot
        hist[2, 1] = 0; hist[2, 1, S - 1] = 9; hist[2, 0, S - 1] = 0; hist[2, 0, 1] = 3      # positives only in the NaN slot, alone there
        hist[3, 0] = 0                                          # no negative: ap is 1, no AUROC
        hist[4, 1] = 0                                          # no positive: no figure
        hist[5] = 0                                             # nothing at all
        fig = curve_figures(hist, 0.0, 1.0, bins)
        ap, auc = _sklearn_figures(hist)
        for got, want in ((fig["ap"], ap), (fig["auroc"], auc)):
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert np.nanmax(np.abs(got - want)) <= TOL
        assert fig["ap"][3] == 1.0 and np.isnan(fig["auroc"][3]) and np.isnan(fig["ap"][4]) and np.isnan(fig["ap"][5])
        assert fig["auroc"][1] == 0.5 and fig["ap"][1] == 5 / 12 and fig["ap"][2] == 1.0 and fig["auroc"][2] == 1.0
        assert fig["positives"].tolist() == hist[:, 1].sum(1).tolist() and fig["negatives"].tolist() == hist[:, 0].sum(1).tolist()


def test_best_f1_and_its_tie_rule():
    from ovmr_amd.evaluator import curve_figures
    bins = 4
    hist = np.zeros((4, 2, 7), dtype=np.int64)
    hist[0, 1, 5], hist[0, 0, 1] = 3, 4                         # separable: every cut from slot 2 to slot 5 has F1 = 1 -> the HIGHEST, 5
    hist[1, 1, 2], hist[1, 1, 4], hist[1, 0, 3] = 2, 2, 2       # cut at 4: p 1, r 1/2, F1 2/3; cut at 2 (and 1, 0): p 2/3, r 1, F1 4/5
    hist[2, 0, 3] = 5                                           # no positive
    hist[3, 1, 6], hist[3, 0, 6] = 1, 1                         # only NaN scores
    f = curve_figures(hist, -1.0, 1.0, bins)
    assert f["slot"].tolist() == [5, 2, -1, 6]
    assert f["best_f1"][0] == 1.0 and f["precision"][0] == 1.0 and f["recall"][0] == 1.0 and f["threshold"][0] == 1.0
    assert f["best_f1"][1] == 0.8 and f["precision"][1] == 2 / 3 and f["recall"][1] == 1.0 and f["threshold"][1] == -0.5
    assert all(np.isnan(f[k][2]) for k in ("best_f1", "threshold", "precision", "recall", "ap", "auroc"))
    assert np.isnan(f["threshold"][3]) and f["best_f1"][3] == 2 / 3
    hist[1, 1, 0] = 1                                           # a positive below lo: the best cut is slot 0, which admits everything
    f = curve_figures(hist, -1.0, 1.0, bins)
    assert f["slot"][1] == 0 and f["threshold"][1] == -INF and f["recall"][1] == 1.0
    # brute force: F1 at every cut, the highest slot among the best
    rng = np.random.default_rng(2)
    hist = rng.integers(0, 4, size=(50, 2, 9)).astype(np.int64)
    hist[:, 1, 0] += 1
    f = curve_figures(hist, 0.0, 1.0, 6)
    for c in range(50):
        P = hist[c, 1].sum()
        f1 = [2 * hist[c, 1, s:].sum() / (hist[c, 1, s:].sum() + hist[c, 0, s:].sum() + P) for s in range(9)]
        assert f["slot"][c] == max(s for s in range(9) if f1[s] == max(f1)) and f["best_f1"][c] == max(f1)


def _evaluator(C=6, bins=16, **kw):
    from ovmr_amd.evaluator import Classification
    return Classification(C, [f"class {i}, the" if i == 1 else f"c{i}" for i in range(C)], device="cpu", curves=bins, **kw)


def _batches(C=6, n=(40, 1, 23), seed=0, present=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in n:
        y = torch.randint(0, C if present is None else present, (b,), generator=g)
        out.append((torch.softmax(torch.randn((b, C), generator=g) * 2, dim=1), y))
    return out


def test_host_evaluator_counts_what_the_reference_counts():
    lo, hi, bins = 0.1, 0.7, 16
    ev = _evaluator(bins=bins, score_range=(lo, hi))
    want = None
    for mo, y in _batches():
        mo.view(-1)[:len(K.edge_table(lo, hi, bins))] = torch.from_numpy(K.edge_table(lo, hi, bins))[:mo.numel()]
        ev.process(mo, y)
        want = K.expected(mo, y, lo, hi, bins, want)
    assert ev._curves.dtype == torch.int32 and K.mismatch(ev._curves, want) is None
    from ovmr_amd.evaluator import curve_slots
    for lo, hi, bins in ALL_CASES:
        for fp16 in (False, True):
            v = K.edge_table(lo, hi, bins, fp16)
            assert curve_slots(torch.from_numpy(v), lo, hi, bins).tolist() == K.slots(v, lo, hi, bins).tolist(), (lo, hi, bins, fp16)


def test_results_files_and_empty_fields(tmp_path, capsys):
    ev = _evaluator()
    plain = _evaluator()
    plain.curve_bins = None                                     # the same pass without curves: what the existing lines must stay
    for mo, y in _batches(present=4):                           # classes 4 and 5 have no image
        ev.process(mo, y)
        plain.process(mo, y)
    res0 = plain.evaluate(str(tmp_path / "plain"))
    before = capsys.readouterr().out
    res = ev.evaluate(str(tmp_path / "out"))
    after = capsys.readouterr().out
    assert after.startswith(before) and list(res)[:3] == list(res0) and list(res)[3:] == ["mAP", "mean_auroc"]
    extra = after[len(before):].splitlines()
    assert extra == [f"* mAP: {res['mAP']:.1f}%", f"* mean_auroc: {res['mean_auroc']:.4f}"]
    assert sorted(os.listdir(tmp_path / "plain")) == ["acc_per_class.csv", "f1_per_class.csv"]
    assert sorted(os.listdir(tmp_path / "out")) == ["acc_per_class.csv", "curves_per_class.csv", "f1_per_class.csv", "score_hist.pt"]
    for name in ("acc_per_class.csv", "f1_per_class.csv"):
        assert (tmp_path / "out" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes()
    fig = ev.curves
    assert res["mAP"] == 100.0 * float(np.mean(fig["ap"][:4])) and res["mean_auroc"] == float(np.mean(fig["auroc"][:4]))
    rows = list(csv.reader(open(tmp_path / "out" / "curves_per_class.csv")))
    from ovmr_amd.evaluator import CURVE_COLUMNS
    assert rows[0] == CURVE_COLUMNS == ["label", "classname", "positives", "negatives", "ap", "auroc", "best_f1", "slot", "threshold", "precision",
                                        "recall"] and len(rows) == 7
    assert rows[2][:2] == ["1", "class 1, the"]
    for c in range(4):
        r = rows[1 + c]
        assert [int(r[2]), int(r[3])] == [int(fig["positives"][c]), int(fig["negatives"][c])] and int(r[2]) + int(r[3]) == 64
        assert [float(v) for v in r[4:7] + r[8:]] == [fig[k][c] for k in ("ap", "auroc", "best_f1", "threshold", "precision", "recall")]
        assert int(r[7]) == fig["slot"][c] and float(r[8]) == (int(r[7]) - 1) / 16
    for c in (4, 5):
        assert rows[1 + c][2:] == ["0", "64"] + [""] * 7, "a class without an image has no figure"
    saved = torch.load(tmp_path / "out" / "score_hist.pt")
    assert set(saved) == {"hist", "lo", "hi", "bins"} and (saved["lo"], saved["hi"], saved["bins"]) == (0.0, 1.0, 16)
    assert saved["hist"].dtype == torch.int64 and saved["hist"].shape == (6, 2, 19) and torch.equal(saved["hist"], ev._curves.long())
    assert int(saved["hist"].sum()) == 64 * 6 and torch.equal(ev.score_hist, saved["hist"])
    # no negative: one class only
    one = _evaluator(C=1)
    one.process(torch.rand(5, 1), torch.zeros(5, dtype=torch.int64))
    r = one.evaluate(str(tmp_path / "one"), report=True)
    assert r["mAP"] == 100.0 and r["mean_auroc"] == 0.0
    row = list(csv.reader(open(tmp_path / "one" / "curves_per_class.csv")))[1]
    assert row[2:6] == ["5", "0", "1.0", ""] and row[6] == "1.0"
    # report=False: figures, no file
    quiet = _evaluator()
    quiet.process(*_batches()[0])
    capsys.readouterr()
    assert "mAP" in quiet.evaluate(str(tmp_path / "quiet"), report=False) and capsys.readouterr().out == "" and not (tmp_path / "quiet").exists()


def test_states_add_and_off_means_off():
    from ovmr_amd.evaluator import Classification
    a, b, both = _evaluator(), _evaluator(), _evaluator()
    batches = _batches(n=(40, 1, 23, 64, 7))
    for i, (mo, y) in enumerate(batches):
        (a if i % 2 else b).process(mo, y)
    for mo, y in reversed(batches):
        both.process(mo, y)
    assert torch.equal(a._curves + b._curves, both._curves) and int(both._curves.sum()) == 135 * 6

    class Dist:
        def get_backend(self): return "gloo"
        def all_reduce(self, t): t.mul_(2)                       # two ranks that counted the same
    before = a._curves.clone()
    cm = Classification(6, device="cpu", curves=16, confusion=True)
    cm.begin()
    Classification.all_reduce([a, cm], Dist())
    assert torch.equal(a._curves, 2 * before) and cm._curves is not None and not bool(cm._curves.any())
    off = Classification(6, device="cpu")
    off.process(*batches[0])
    assert off._curves is None and off.curve_bins is None and "mAP" not in off.evaluate(report=False) and off.curves is None
    idle = _evaluator()
    idle.begin()
    assert idle._curves.shape == (6, 2, 19) and idle._curves.dtype == torch.int32, "begin() allocates: a rank without a batch holds the tensor"
    idle.reset()
    assert idle._curves is None
    for kw, msg in ((dict(curves=0), "curves must be"), (dict(curves=4097), "curves must be"), (dict(curves=16.0), "curves must be"),
                    (dict(curves=16, score_range=(1.0, 1.0)), "Classification: hi must be"), (dict(curves=16, score_range=(0.0, INF)), "hi must be"),
                    (dict(curves=16, score_range=0.5), "score_range must be a pair")):
        with pytest.raises(ValueError, match=msg):
            Classification(6, device="cpu", **kw)


def test_trainers_share_the_keywords():
    from ovmr_amd import trainer
    for cls in (trainer.MM_CLS_OP, trainer.ZeroshotCLIP, trainer.ZeroshotCLIP2):
        p = inspect.signature(cls.__init__).parameters
        assert p["score_curves"].default is None and p["score_range"].default is None
        names = list(p)
        assert names.index("compute_cmat") < names.index("score_curves") < names.index("score_range")


# ---- the runner --------------------------------------------------------------------------------------------------------------------------

def test_runner_refusals():
    from ovmr_amd import cli
    w = ["--clip-weights", "clip.pt"]
    s = w + ["--score-curves"]
    assert cli.check_score_curves(cli.parse(w), "MM_CLS_OP", False) == (None, None)
    assert cli.check_score_curves(cli.parse(s), "MM_CLS_OP", False) == (256, (0.0, 1.0)) and cli.DEFAULT_BINS == 256
    assert cli.check_score_curves(cli.parse(w + ["--score-curves", "4096", "--score-range", "-30", "45.5"]), "ZeroshotCLIP", True) == (4096, (-30.0, 45.5))
    assert cli.check_score_curves(cli.parse(s + ["--score-range", "0.1", "0.7"]), "MM_CLS_OP", False) == (256, (0.1, 0.7))
    for argv, zeroshot, msg in (
            (s + ["--predict", "pics"], False, "--score-curves belongs to the test pass: --predict"),
            (s + ["--retrieve", "pool"], False, "--score-curves belongs to the test pass: --retrieve"),
            (w + ["--score-range", "0", "1"], False, r"--score-range LO HI belongs to --score-curves \[BINS\]"),
            (w + ["--score-curves", "0"], False, r"--score-curves 0: BINS must lie in \[1, 4096\]"),
            (w + ["--score-curves", "4097"], False, r"--score-curves 4097: BINS must lie in \[1, 4096\]"),
            (s, True, "--score-curves: --trainer ZeroshotCLIP returns logits, which have no natural range: give --score-range LO HI"),
            (s + ["--score-range", "0", "inf"], False, "--score-range 0.0 inf: LO and HI must be finite"),
            (s + ["--score-range", "nan", "1"], True, "--score-range nan 1.0: LO and HI must be finite"),
            (s + ["--score-range", "1", "1"], False, "--score-range 1.0 1.0: LO must lie below HI"),
            (s + ["--score-range", "2", "1"], True, "--score-range 2.0 1.0: LO must lie below HI"),
            (s + ["--score-range", "1", "1.000000001"], False, "--score-range 1.0 1.000000001: as fp32 the range must be"),
            (s + ["--score-range", "0", "1e39"], False, "--score-range 0.0 1e\\+39: as fp32 the range must be")):
        with pytest.raises(SystemExit, match=msg) as err:
            cli.check_score_curves(cli.parse(argv), "ZeroshotCLIP" if zeroshot else "MM_CLS_OP", zeroshot)
        assert "\n" not in str(err.value)
    # main refuses before anything is listed or loaded: the paths do not exist, the weights do not exist
    base = ["--eval-only", "--eval_mode", "fusion"]
    for trainer, argv, msg in (("MM_CLS_OP", s + ["--predict", "pics"], "--score-curves belongs to the test pass: --predict"),
                               ("MM_CLS_OP", s + ["--retrieve", "pool"], "--score-curves belongs to the test pass: --retrieve"),
                               ("MM_CLS_OP", w + ["--score-range", "0", "1"], "--score-range LO HI belongs"),
                               ("MM_CLS_OP", w + ["--score-curves", "5000"], "--score-curves 5000"),
                               ("ZeroshotCLIP", s, "returns logits"), ("ZeroshotCLIP2", s, "returns logits"),
                               ("MM_CLS_OP", s + ["--score-range", "3", "2"], "LO must lie below HI")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(base + ["--trainer", trainer] + argv)
