"""Search by class (include/ovmr_hip_retrieve.h) in plain torch, no library: the expectation, a brute force for tiny cases, the comparator,
the planted score matrices the CPU and the GPU tests share, and a model of the chunked update / merge with one planted defect at a time.

A pool is a score matrix s [N, C] (fp16 or fp32); image n is row n, offered with index base + n.  The order is the library's total order:
larger value first, equal values (-0 == +0) to the LOWER image index, every NaN above +inf.  There is no arithmetic: every comparison
is exact."""
import math

import torch

TILE, CHUNK = 16, 64          # RT_TILE, RT_ROWS of ovmr_amd/csrc/retrieve.hip: classes per workgroup, rows per chunk of retrieve_update_kernel
                              # (tests/test_retrieve_cpu.py holds the two pairs to each other)
TILE_NARROW, NARROW_MAX_C = 4, 2048     # RT_TILE_NARROW, RT_NARROW_MAX_C: up to that many classes a workgroup owns 4 classes, one per wave


def below(x, f):
    """x is below f in the value order (NaN above everything, NaNs equal among themselves): such an element is NOT eligible under floor f."""
    return (torch.isnan(f) & ~torch.isnan(x)) | (x < f)


def expected(s, m, floor=None, base=0, tail_index=-1):
    """(values fp32 [C, m], indices int64 [C, m]): torch.sort(stable, descending) along the image axis of the transposed score matrix
    (the method of nearest_cases.expected); with floor fp32 [N] the elements below their row's floor are removed first; tails are padded
    with (tail_index, -inf)."""
    t = s.float().t().contiguous()
    C, N = t.shape
    vals = torch.full((C, m), -math.inf)
    idx = torch.full((C, m), tail_index, dtype=torch.int64)
    for c in range(C):
        keep = torch.arange(N) if floor is None else (~below(t[c], floor.float())).nonzero().reshape(-1)
        v, i = torch.sort(t[c, keep], descending=True, stable=True)
        n = min(m, int(keep.numel()))
        vals[c, :n] = v[:n]
        idx[c, :n] = keep[i[:n]] + base
    return vals, idx


def _rank(x, index):
    """Sort key of one element: smaller = better."""
    return (0 if x != x else 1, 0.0 if x != x else -x, index)


def brute_force(s, m, floor=None, base=0):
    """The same order element by element on Python tuples (tiny cases only)."""
    N, C = s.shape
    vals, idx = [], []
    for c in range(C):
        rows = []
        for n in range(N):
            x = float(s[n, c])
            if floor is not None:
                f = float(floor[n])
                if (f != f and x == x) or x < f:
                    continue
            rows.append(_rank(x, base + n) + (x,))
        rows.sort(key=lambda t: t[:3])
        rows = rows[:m]
        vals.append([t[3] for t in rows] + [-math.inf] * (m - len(rows)))
        idx.append([t[2] for t in rows] + [-1] * (m - len(rows)))
    return torch.tensor(vals, dtype=torch.float32).reshape(C, m), torch.tensor(idx, dtype=torch.int64).reshape(C, m)


def mismatch(got, want):
    """None if (values, indices) equal the expectation -- indices bit for bit, values as numbers with NaN == NaN (the key does not tell
    -0 from +0) -- else the first differing (class, rank)."""
    (gv, gi), (wv, wi) = got, want
    gv, gi = gv.detach().cpu(), gi.detach().cpu()
    if gv.shape != wv.shape or gi.shape != wi.shape:
        return f"shapes {tuple(gv.shape)} / {tuple(gi.shape)} != {tuple(wv.shape)} / {tuple(wi.shape)}"
    if gv.dtype != torch.float32 or gi.dtype != torch.int64:
        return f"dtypes {gv.dtype} / {gi.dtype}"
    bad = (gi != wi) | ~((gv == wv) | (torch.isnan(gv) & torch.isnan(wv)))
    if not bool(bad.any()):
        return None
    c, j = (int(x) for x in bad.nonzero()[0])
    return (f"{int(bad.sum())} entries differ, first at class {c}, rank {j}: expected image {int(wi[c, j])} ({float(wv[c, j])}), "
            f"got image {int(gi[c, j])} ({float(gv[c, j])})")


# ---- planted pools ------------------------------------------------------------------------------------------------------------------

CUTS = {300: [(300,), (64, 64, 64, 64, 44), (1, 299), (65, 235)], 65: [(65,), (64, 1), (1, 64)], 64: [(64,), (63, 1)],
        63: [(63,), (31, 32)], 5: [(5,), (2, 3)], 1: [(1,)]}


def planted_pool(N, C, dtype=torch.float16, seed=0):
    """s [N, C]: scores on a grid of 1/8 in [-4, 4] (many ties), and where the pool is large enough
         column 0: images 3, 90 and 280 share the best value (m = 2: images 3 and 90 are in -- the tie decides membership across batches);
         column 1: all zero, -0 among +0 (every class answers images 0 .. m-1);      column 2: a NaN at image 7 (it ranks first);
         column 3: +inf at image 70, -inf at image 2;      column 4: rising along the stream;      column 5: falling;
         the last column: rising (a partial class tile does real work)."""
    g = torch.Generator().manual_seed(seed)
    s = (torch.randint(-32, 33, (N, C), generator=g).float() / 8)
    n = torch.arange(N).float()
    if C > 0:
        for r in (3, 90, 280):
            if r < N:
                s[r, 0] = 5.0
    if C > 1:
        s[:, 1] = 0.0
        s[1::3, 1] = -0.0
    if C > 2 and N > 7:
        s[7, 2] = float("nan")
    if C > 3 and N > 70:
        s[70, 3], s[2, 3] = float("inf"), -float("inf")
    if C > 4:
        s[:, 4] = n / 8 - 10
    if C > 5:
        s[:, 5] = 10 - n / 8
    if C > 6:
        s[:, C - 1] = n / 16
    return s.to(dtype)


def floor_table(s):
    """fp32 [N] for the pool s (fp16 grid): a cycle of -inf, the value of the row's element in column c = n % C (eligible), one fp16 step
    above it (that element is not eligible), +inf and NaN."""
    N, C = s.shape
    f = torch.empty(N)
    for n in range(N):
        x = s[n, n % C].float()
        x = torch.tensor(0.0) if bool(torch.isnan(x)) or bool(torch.isinf(x)) else x
        kind = n % 5
        step = torch.nextafter(x.half(), torch.tensor(math.inf, dtype=torch.float16)).float()
        f[n] = (-math.inf, float(x), float(step), math.inf, math.nan)[kind]
    return f


# ---- a model of the kernels, with one defect at a time ----------------------------------------------------------------------------------

DEFECTS = ("ties_later", "local_base", "ld_C", "drop_row_chunk", "drop_class_tile", "no_carry", "floor_gt", "tail_zero",
           "merge_drop_equal", "index31")


def _offer(lst, m, item, later=False):
    """lst: sorted [(rank key, index, value)] of one class; keeps the m best."""
    lst.append(item)
    lst.sort(key=(lambda t: (t[0][0], t[0][1], -t[0][2])) if later else (lambda t: t[0]))
    del lst[m:]


def _update(lists, m, storage, ld, B, C, base, floor, defect):
    """One ovmr_retrieve_update: storage is the flat buffer the batch lives in (rows ld apart), walked in row chunks and class tiles."""
    if defect == "no_carry":
        for l in lists:
            l.clear()
    stride = C if defect == "ld_C" else ld
    rows = B // CHUNK * CHUNK if defect == "drop_row_chunk" and B > CHUNK else B
    cols = C // TILE * TILE if defect == "drop_class_tile" and C > TILE else C
    for c in range(cols):
        for b in range(rows):
            x = float(storage[b * stride + c])
            if floor is not None:
                f = float(floor[b])
                if (f != f and x == x) or x < f or (defect == "floor_gt" and (x == f or (x != x and f != f))):
                    continue
            index = b if defect == "local_base" else base + b
            if defect == "index31":
                index &= 0x7FFFFFFF
            _offer(lists[c], m, (_rank(x, index), index, x), later=defect == "ties_later")


def simulate(s, m, cuts=None, floor=None, base=0, gap=0, defect=None, split=None, reverse=False):
    """The kernels' result on pool s [N, C], fed in batches of `cuts` rows (reversed batch order with the right bases if `reverse`), each
    batch stored with rows C + gap apart (the gap holds NaNs); split = n: rows [0, n) and [n, N) are two streams whose states are merged.
    defect: one of DEFECTS, or None for the honest model."""
    N, C = s.shape
    cuts = (N,) if cuts is None else cuts
    assert sum(cuts) == N
    ld = C + gap

    def stream(lo, hi):
        lists = [[] for _ in range(C)]
        spans, a = [], 0
        for n in cuts:
            spans.append((a, a + n))
            a += n
        for a, b in (reversed(spans) if reverse else spans):
            a, b = max(a, lo), min(b, hi)
            if a >= b:
                continue
            storage = torch.full(((b - a) * ld + C,), math.nan)
            storage[:(b - a) * ld].view(b - a, ld)[:, :C] = s[a:b].float()
            _update(lists, m, storage.tolist(), ld, b - a, C, base + a, None if floor is None else floor[a:b], defect)
        return lists

    if split is None:
        lists = stream(0, N)
    else:
        lists, other = stream(0, split), stream(split, N)
        for mine, theirs in zip(lists, other):
            for item in theirs:
                if defect == "merge_drop_equal" and any(t[0][:2] == item[0][:2] for t in mine):
                    continue
                _offer(mine, m, item, later=defect == "ties_later")
    tail = 0 if defect == "tail_zero" else -1
    vals = torch.tensor([[t[2] for t in l] + [-math.inf] * (m - len(l)) for l in lists], dtype=torch.float32).reshape(C, m)
    idx = torch.tensor([[t[1] for t in l] + [tail] * (m - len(l)) for l in lists], dtype=torch.int64).reshape(C, m)
    return vals, idx
