"""Score curves: the reference and the tables behind test_curves_cpu.py, test_hip_curves.py and test_hip_curves_model.py.  Plain numpy and
torch, importable without a GPU.

The reference is written from the text of include/ovmr_hip_curves.h, in numpy float32, and shares nothing with the product's torch slot
function (ovmr_amd/evaluator.py: curve_slots): `slots` is the vectorised statement, `slot_literal` a second one, value by value, whose
two comparisons are made on the selection key's bits as the header says.  `expected` builds the state by brute force over (b, c).

`model` is a CPU model of the kernel's walk (class tiles of TILE, row chunks of CHUNK) that can carry ONE planted defect of DEFECTS:
test_curves_cpu.py holds the comparator to rejecting each of them on the cases the GPU tests run.
"""
import struct

import numpy as np
import torch

TILE, CHUNK, MAX_ROW_BLOCKS = 16, 64, 256          # eval_curves.hip: EC_TILE, EC_ROWS, EC_MAX_ROW_BLOCKS (held by test_curves_cpu.py)
MAX_BINS = 4096
RANGES = [(0.0, 1.0), (0.1, 0.7), (-100.0, 100.0)]
BINS = [1, 7, 256, 4096]
CLAMP_CASES = [(-100.0, 100.0, 1024), (-1.0, 1.0, 4096)]        # the largest fp32 below hi gives t == bins exactly
NO_CLAMP_CASES = [(0.0, 1.0, 256), (0.1, 0.7, 1000), (0.0, 1.0, 4096)]
F32 = np.float32


def scale_of(lo, hi, bins):
    """The launcher's scale: fp32(bins) / (hi - lo), the subtraction and the division rounded once each."""
    return F32(F32(bins) / F32(F32(hi) - F32(lo)))


def slots(x, lo, hi, bins):
    """x (any shape, taken as fp32) -> int64 slots in [0, bins + 3)."""
    x = np.asarray(x, dtype=F32)
    lo, hi, scale = F32(lo), F32(hi), scale_of(lo, hi, bins)
    with np.errstate(all="ignore"):
        d = np.subtract(x, lo, dtype=F32)
        t = np.multiply(d, scale, dtype=F32)
        inside = (x >= lo) & (x < hi)
        j = np.floor(np.where(inside, t, F32(0))).astype(np.int64)
    s = np.where(inside, 1 + np.minimum(bins - 1, j), 0)
    s = np.where(x >= hi, bins + 1, s)
    return np.where(np.isnan(x), bins + 2, s).astype(np.int64)


def value_key(v):
    """The value part of the library's selection key (csrc/eval_common.h: topk_key) of one fp32, as a Python int."""
    u = struct.unpack("<I", struct.pack("<f", float(v)))[0]
    if v != v:
        return 0xFFFFFFFF
    if u == 0x80000000:
        u = 0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def slot_literal(x, lo, hi, bins):
    """The header's four lines for ONE value, comparisons on the key's bits."""
    x = F32(x)
    S = bins + 3
    if x != x:
        return S - 1
    if value_key(x) < value_key(F32(lo)):
        return 0
    if value_key(x) >= value_key(F32(hi)):
        return S - 2
    t = F32(F32(x - F32(lo)) * scale_of(lo, hi, bins))
    return 1 + min(bins - 1, int(np.floor(t)))


def _nan(sign):
    return np.array([0xFFC00000 if sign else 0x7FC00000], dtype=np.uint32).view(F32)[0]


def edge_table(lo, hi, bins, fp16=False, interior=64):
    """The values at which the slot function can go wrong, as fp32 (fp16=True: every one representable in fp16): lo, hi and their
    neighbours on either side, +-inf, NaN of both signs, +-0, a denormal of either sign, the interior edges lo + j / scale with their two
    neighbours (the first and the last `interior` of them where bins is larger), and the exact edges an fp16 can hold."""
    lo32, hi32, scale = F32(lo), F32(hi), scale_of(lo, hi, bins)
    dt = np.float16 if fp16 else F32
    out = []

    def around(v):
        v = dt(v)
        return [np.nextafter(v, dt(-np.inf)), v, np.nextafter(v, dt(np.inf))]
    with np.errstate(all="ignore"):
        out += around(lo32) + around(hi32)
        out += [dt(np.inf), dt(-np.inf), _nan(0), _nan(1), dt(0.0), dt(-0.0)]
        tiny = np.nextafter(dt(0), dt(1))                                # the smallest denormal of the input format
        out += [tiny, -tiny, dt(2) * tiny, dt(-3) * tiny]
        js = sorted(set(list(range(min(bins, interior) + 1)) + list(range(max(0, bins - interior), bins + 1))))
        for j in js:
            out += around(F32(lo32 + F32(F32(j) / scale)))
            out += around(lo + j * (hi - lo) / bins)                      # the nominal edge, from fp64
    v = np.array([F32(e) for e in out], dtype=F32)
    if fp16:
        assert np.array_equal(v.astype(np.float16).astype(F32), v, equal_nan=True)
    return v


def scores(B, C, lo, hi, bins, fp16=False, seed=0, kind="uniform"):
    """[B, C] scores (torch, fp16 or fp32) with the edge table spread over rows and columns by a seeded permutation; the rest is uniform
    over a range a tenth wider than [lo, hi) on either side (`uniform`) or a softmax row (`softmax`: nearly all negatives in one slot)."""
    rng = np.random.default_rng(seed)
    w = hi - lo
    if kind == "softmax":
        z = rng.standard_normal((B, C)) * 3
        x = np.exp(z - z.max(axis=1, keepdims=True))
        x = (x / x.sum(axis=1, keepdims=True)).astype(F32)
    else:
        x = rng.uniform(lo - 0.1 * w, hi + 0.1 * w, size=(B, C)).astype(F32)
    edges = edge_table(lo, hi, bins, fp16)
    where = rng.permutation(B * C)[:len(edges)]
    x.reshape(-1)[where] = edges[rng.permutation(len(edges))[:len(where)]]
    t = torch.from_numpy(x)
    return t.half() if fp16 else t


def labels(B, C, kind="random", seed=0):
    """int64 [B]: `random`; `hot` (every row the same label: the hot cell); `bad` (random, with -1, C, 2^40 and the int64 extremes among
    them: rows offered to no class)."""
    rng = np.random.default_rng(seed + 17)
    y = rng.integers(0, C, size=B).astype(np.int64)
    if kind == "hot":
        y[:] = C // 2
    elif kind == "bad":
        bad = [-1, C, 2 ** 40, -2 ** 63, 2 ** 63 - 1, C + 2 ** 32, -2 ** 32]          # (the last two: equal to a class in their low 32 bits)
        pos = rng.permutation(B)[:max(1, min(B // 2, len(bad)))]
        y[pos] = np.array(bad[:len(pos)], dtype=np.int64)
    return torch.from_numpy(y)


def expected(out, y, lo, hi, bins, state=None):
    """The state after one call, by brute force over (b, c): int64 [C, 2, bins + 3] (added to `state` if given)."""
    B, C = out.shape
    S = bins + 3
    s = slots(out.float().numpy(), lo, hi, bins)
    want = np.zeros((C, 2, S), dtype=np.int64) if state is None else torch.as_tensor(state).long().numpy().copy()
    yy = y.numpy()
    for b in range(B):
        if not 0 <= int(yy[b]) < C:
            continue
        for c in range(C):
            want[c, 1 if int(yy[b]) == c else 0, s[b, c]] += 1
    return torch.from_numpy(want)


DEFECTS = ["fma", "no_min", "gt_at_hi", "le_at_lo", "nan_to_zero", "neg_zero_under", "planes_swapped", "overwrite", "drop_row_chunk",
           "drop_class_tile", "bad_label_negative"]


def _defect_slots(x, lo, hi, bins, defect):
    x = np.asarray(x, dtype=F32)
    lo32, hi32, scale = F32(lo), F32(hi), scale_of(lo, hi, bins)
    with np.errstate(all="ignore"):
        if defect == "fma":                                               # t = fma(x, scale, -(lo * scale)): one rounding where there are two
            t = (x.astype(np.float64) * np.float64(scale) - np.float64(F32(lo32 * scale))).astype(F32)
        else:
            t = np.multiply(np.subtract(x, lo32, dtype=F32), scale, dtype=F32)
        below = x <= lo32 if defect == "le_at_lo" else x < lo32
        if defect == "neg_zero_under" and lo32 == 0:
            below = below | ((x == 0) & np.signbit(x))
        above = (x > hi32 if defect == "gt_at_hi" else x >= hi32) & ~below
        inside = ~below & ~above & ~np.isnan(x)
        j = np.floor(np.where(inside, t, F32(0))).astype(np.int64)
    s = np.where(inside, 1 + (j if defect == "no_min" else np.minimum(bins - 1, j)), 0)
    s = np.where(above, bins + 1, s)
    return np.where(np.isnan(x), 0 if defect == "nan_to_zero" else bins + 2, s).astype(np.int64)


def model(out, y, lo, hi, bins, state, defect=None):
    """The kernel's walk on the host: class tiles of TILE, row chunks of CHUNK, each (class, chunk) added to `state` (int64 [C, 2, S], in
    place) -- with one of DEFECTS planted, or none."""
    B, C = out.shape
    S = bins + 3
    s = _defect_slots(out.float().numpy(), lo, hi, bins, defect)
    yy = y.numpy()
    st = state.numpy()
    if defect == "overwrite":
        st[:] = 0
    rows = B // CHUNK * CHUNK if defect == "drop_row_chunk" else B
    classes = C // TILE * TILE if defect == "drop_class_tile" else C
    for c0 in range(0, classes, TILE):
        for r0 in range(0, rows, CHUNK):
            for c in range(c0, min(c0 + TILE, classes)):
                for b in range(r0, min(r0 + CHUNK, rows)):
                    ok = 0 <= int(yy[b]) < C
                    if not ok and defect != "bad_label_negative":
                        continue
                    own = int(ok and int(yy[b]) == c)
                    if defect == "planes_swapped":
                        own = 1 - own
                    st[c, own, int(s[b, c])] += 1                         # (no_min: t == bins lands in the overflow slot, below hi)
    return state


def mismatch(got, want):
    """None where the two states are equal, else the count and the first cell that differs."""
    got, want = torch.as_tensor(got).long(), torch.as_tensor(want).long()
    if got.shape != want.shape:
        return f"shape {list(got.shape)} != {list(want.shape)}"
    bad = (got != want).nonzero()
    if len(bad) == 0:
        return None
    c, p, s = (int(v) for v in bad[0])
    return (f"{len(bad)} of {got.numel()} cells differ, the first at class {c}, plane {p}, slot {s} of {got.shape[2]}: "
            f"got {int(got[c, p, s])}, expected {int(want[c, p, s])}")


def random_state(C, bins, seed=0, high=50):
    rng = np.random.default_rng(seed + 99)
    return torch.from_numpy(rng.integers(0, high, size=(C, 2, bins + 3)).astype(np.int64))
