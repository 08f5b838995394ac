"""Cases, expectations and comparators for the neighbour search with exclusions (include/ovmr_hip_audit.h: ovmr_neighbours_rows, its tiled
and its short path) and for CustomCLIP.audit_bank.  Plain torch, no library: shared by test_hip_neighbours.py and test_hip_bank_audit.py
(GPU) and by test_audit_cpu.py, which proves that the comparators reject the defects they are there for.

Exact operands are those of nearest_cases.exact_case (head_exact.assert_exact): every partial sum is exact in fp32 in ANY order, so the
score is ONE fp16 number for the matrix pipe's order and for the short kernel's alike, and the expectation is a stable descending sort
over the candidate rows of each query: lo <= r < hi', not xlo <= r < xhi, both clamped to [0, R] as the header says, hi' = min(hi,
lo + max_range) where max_range > 0.  Indices bit for bit, values as numbers (nearest_cases.mismatch).
General operands are compared by margin (nearest_cases.margin) on the candidate set reduced by the exclusion: nothing is left out, so
the comparator needs no cap.
"""
import math

import torch

import nearest_cases as N
from head_exact import assert_exact

MAX_RANGE = 4096


def clamp_pair(lo, hi, R):
    """The header's clamping: 0 <= lo <= hi <= R."""
    lo = min(max(int(lo), 0), R)
    return lo, min(max(int(hi), lo), R)


def candidates(b, R, ranges=None, exclude=None, max_range=0):
    """The candidate rows of query b, increasing (int64 tensor)."""
    lo, hi = (0, R) if ranges is None else clamp_pair(ranges[b, 0], ranges[b, 1], R)
    if max_range > 0:
        hi = min(hi, lo + max_range)
    xlo, xhi = (0, 0) if exclude is None else clamp_pair(exclude[b, 0], exclude[b, 1], R)
    rows = torch.arange(lo, hi, dtype=torch.int64)
    return rows[~((rows >= xlo) & (rows < xhi))]


def expected(s16, k, ranges=None, exclude=None, max_range=0, tail_index=-1):
    """(values fp32 [B, k], indices int32 [B, k]): per query the stable descending sort of its candidates' scores, tail (tail_index, -inf)."""
    B, R = s16.shape
    s = s16.float()
    vals = torch.full((B, k), -math.inf)
    idx = torch.full((B, k), tail_index, dtype=torch.int32)
    for b in range(B):
        rows = candidates(b, R, ranges, exclude, max_range)
        if not rows.numel():
            continue
        v, i = torch.sort(s[b, rows], descending=True, stable=True)
        n = min(k, rows.numel())
        vals[b, :n] = v[:n]
        idx[b, :n] = rows[i[:n]].to(torch.int32)
    return vals, idx


def _key(x, r, ties_high=False):
    nan = x != x
    return (0 if nan else 1, 0.0 if nan else -x, -r if ties_high else r)


def brute_force(s16, k, ranges=None, exclude=None, max_range=0):
    """The same order spelled out element by element (tiny cases only)."""
    B, R = s16.shape
    vals, idx = [], []
    for b in range(B):
        rows = sorted(candidates(b, R, ranges, exclude, max_range).tolist(), key=lambda r: _key(float(s16[b, r]), r))[:k]
        vals.append([float(s16[b, r]) for r in rows] + [-math.inf] * (k - len(rows)))
        idx.append(rows + [-1] * (k - len(rows)))
    return torch.tensor(vals, dtype=torch.float32).reshape(B, k), torch.tensor(idx, dtype=torch.int32).reshape(B, k)


mismatch = N.mismatch


def margin_mismatch(got, Q, X, k, ranges=None, exclude=None, max_range=0):
    """nearest_cases.general_mismatch on the candidate set reduced by the exclusion: every returned row is a candidate, none repeated,
    scores (fp64) at least the n-th best candidate's - m, every value within m / 2 of its row's score, values do not increase and equal
    values come in increasing row order, the tail past the n candidates is (-1, -inf)."""
    gv, gi = got[0].detach().cpu().double(), got[1].detach().cpu().long()
    s = Q.double() @ X.double().t()
    m = N.margin(Q.shape[1], float(s.abs().max()))
    B, R = s.shape
    for b in range(B):
        cand = candidates(b, R, ranges, exclude, max_range)
        n = min(k, cand.numel())
        if bool((gi[b, n:] != -1).any()) or bool((gv[b, n:] != -math.inf).any()):
            return f"query {b}: tail past {n} candidates is not (-1, -inf)"
        if n == 0:
            continue
        rows = gi[b, :n]
        if not set(rows.tolist()) <= set(cand.tolist()) or rows.unique().numel() != n:
            return f"query {b}: rows {rows.tolist()} are not {n} distinct candidates"
        kth = torch.sort(s[b, cand], descending=True).values[n - 1]
        if bool((s[b, rows] < kth - m).any()):
            return f"query {b}: a returned row scores {float(s[b, rows].min())}, the n-th best candidate {float(kth)} (margin {m})"
        if bool(((gv[b, :n] - s[b, rows]).abs() > m / 2).any()):
            return f"query {b}: a value is {float((gv[b, :n] - s[b, rows]).abs().max())} from its row's score (m / 2 = {m / 2})"
        d = gv[b, 1:n] - gv[b, :n - 1]
        if bool((d > 0).any()) or bool(((d == 0) & (rows[1:] < rows[:-1])).any()):
            return f"query {b}: values increase, or equal values are not in increasing row order"
    return None


# ---- a model of both paths on a score matrix, with ONE planted defect ---------------------------------------------------------------------

DEFECTS = ("self_included", "excl_inclusive", "excl_position", "cut_64", "cut_8", "ties_high", "unrounded", "tail_zero", "no_truncation")


def simulate(s16, k, ranges=None, exclude=None, max_range=0, defect=None, s32=None):
    """The search as the library computes it -- candidates, keys, the k best -- optionally with one defect:
      "self_included": the exclusion is ignored;                 "excl_inclusive": the exclusion's end row is excluded too;
      "excl_position": the exclusion is compared with r - lo;    "cut_64" / "cut_8": the rows of a range's last, partial 64- / 8-row pass are lost;
      "ties_high": equal scores go to the higher row;            "unrounded": ordered by the fp32 scores s32, values from s16;
      "tail_zero": an unfilled rank holds index 0;               "no_truncation": max_range does not cut the range."""
    B, R = s16.shape
    vals = torch.full((B, k), -math.inf)
    idx = torch.full((B, k), 0 if defect == "tail_zero" else -1, dtype=torch.int32)
    for b in range(B):
        lo, hi = (0, R) if ranges is None else clamp_pair(ranges[b, 0], ranges[b, 1], R)
        if max_range > 0 and defect != "no_truncation":
            hi = min(hi, lo + max_range)
        xlo, xhi = (0, 0) if exclude is None else clamp_pair(exclude[b, 0], exclude[b, 1], R)
        if defect == "self_included":
            xlo = xhi = 0
        if defect == "excl_inclusive" and exclude is not None:
            xhi = min(R, xhi + 1)
        if defect in ("cut_64", "cut_8"):
            step = 64 if defect == "cut_64" else 8
            hi = lo + (hi - lo) // step * step
        rows = [r for r in range(lo, hi) if not xlo <= (r - lo if defect == "excl_position" else r) < xhi]
        order = (s32 if defect == "unrounded" else s16)[b]
        rows.sort(key=lambda r: _key(float(order[r]), r, defect == "ties_high"))
        for j, r in enumerate(rows[:k]):
            vals[b, j] = float(s16[b, r])
            idx[b, j] = r
    return vals, idx


# ---- the short path's cases ---------------------------------------------------------------------------------------------------------------

def short_lengths(k):
    """The range lengths the short path is held to: around k, around a pass of 8 rows and a trip of 64, and two trips and a row."""
    return sorted({0, 1, max(0, k - 1), k, 7, 8, 9, 63, 64, 65, 129})


def short_tables(B, R, k, max_range, seed):
    """ranges and exclude int32 [B, 2] for B queries on a bank of R >= 200 rows.  Query b's range has length short_lengths(k)[b % ..] (never
    above max_range, except the kinds below), starts at row 0 for b % 7 == 0, ends at R for b % 7 == 1, elsewhere at a seeded place.
    Kinds by b % 13 where B allows: 11 -> exactly max_range rows, 12 -> max_range + 3 rows (truncated: the expectation says so).
    Exclusions cycle through: none (empty), the first row, a middle row, the last row, the whole range, the range's upper half and beyond,
    rows outside the range, and unclamped values (negative lo, hi > R, hi < lo)."""
    g = torch.Generator().manual_seed(seed)
    lens = short_lengths(k)
    ranges, excl = [], []
    for b in range(B):
        n = min(lens[b % len(lens)], max_range, R)
        if b % 13 == 11:
            n = min(max_range, R)
        elif b % 13 == 12:
            n = min(max_range + 3, R)
        lo = 0 if b % 7 == 0 else R - n if b % 7 == 1 else int(torch.randint(0, R - n + 1, (1,), generator=g))
        hi = lo + n
        kind = b % 9
        x = {0: (0, 0), 1: (lo, lo + 1), 2: (lo + n // 2, lo + n // 2 + 1), 3: (hi - 1, hi), 4: (lo, hi), 5: (lo + n // 2, hi + 5),
             6: (hi, hi + 9), 7: (-5, lo + 2), 8: (lo + 1, R + 100)}[kind]
        if b % 18 == 17:
            x = (lo + 3, lo)                                        # hi < lo: clamps to an empty exclusion
        if b % 26 == 25:
            lo, hi = hi + 2, lo                                     # an unclamped range, hi < lo: empty
        ranges.append((lo, hi))
        excl.append(x)
    return torch.tensor(ranges, dtype=torch.int32).reshape(B, 2), torch.tensor(excl, dtype=torch.int32).reshape(B, 2)


# (B, R, D, k, max_range): every B in {1, 3, 4, 5, 257}, D in {64, 128, 512, 768, 1024}, k in {1, 5, 32}; max_range picks the 16-, 32- and
# 64-row trips of the kernel at every D parity (D / 64 odd takes the 64-row trip whatever max_range says)
SHORT_SHAPES = [
    (1, 300, 64, 1, 200), (3, 300, 128, 5, 200), (4, 300, 512, 32, 200), (5, 300, 768, 5, 200), (257, 400, 1024, 5, 200),
    (257, 400, 64, 32, 130), (5, 300, 128, 5, 16), (4, 300, 512, 5, 16), (5, 300, 512, 5, 30), (3, 300, 768, 1, 12), (5, 300, 1024, 32, 4096),
    (257, 700, 512, 5, 64),
]

# (B, R, D, k) of the tiled path with exclusion
TILED_SHAPES = [(5, 257, 64, 5), (66, 1000, 128, 5), (130, 1000, 512, 32), (33, 70001, 64, 5)]


def tiled_tables(B, R, k, slices=2):
    """exclude int32 [B, 2] for the tiled path (ranges: nearest_cases.range_table or None): across a tile boundary, across the boundary of
    `slices` slices, a whole tile, everything, a class-sized block, nothing."""
    T = N.n_tiles(R)
    cut = min(R - 1, ((T + slices - 1) // slices) * N.TILE)
    kinds = [(N.TILE - 9, N.TILE + 7), (cut - 5, cut + 11), (0, min(R, N.TILE)), (0, R), (16 * 3, 16 * 4), (0, 0), (R - 1, R), (-7, 3), (R - 20, R + 50)]
    rows = [kinds[b % len(kinds)] for b in range(B)]
    return torch.tensor(rows, dtype=torch.int32).reshape(B, 2)


def class_tables(B, R, per_class=16):
    """ranges NULL with a class-sized exclusion per query: query b leaves out the class of row (37 b) % R."""
    c = (torch.arange(B) * 37 % R) // per_class
    return torch.stack([c * per_class, torch.minimum((c + 1) * per_class, torch.tensor(R))], 1).to(torch.int32)


def planted_short_case(k=5, D=128, B=6, R=300):
    """The planted rows of the short path, all inside the range [100, 170) of every query, on exact operands: rows 110, 131 and 150 are one
    vector, the best for every query (the tie goes to the lower row; at k = 2 it decides the cut), query 3 is all zero (every score +0: the
    answer is the range's first rows)."""
    Q, X, _ = N.exact_case(B, R, D, k, 78)
    v = torch.zeros(D, dtype=torch.float16)
    v[:16] = 0.25
    for r in (110, 131, 150):
        X[r] = v
    Q[:, :16] = 0.375
    Q[3] = 0.0
    assert_exact(Q, X, "planted short")
    ranges = torch.tensor([[100, 170]] * B, dtype=torch.int32)
    return Q, X, N.scores16(Q, X), ranges


# ---- audit_bank ---------------------------------------------------------------------------------------------------------------------------

def value_gt(a, b):
    """a > b in the library's order on values: NaN largest (all NaNs equal), -0 == +0."""
    an, bn = torch.isnan(a), torch.isnan(b)
    return (an & ~bn) | (~an & ~bn & (a > b))


def expected_audit(s16, starts, k, classes=None, dup_threshold=0.995, defect=None):
    """What CustomCLIP.audit_bank returns, from the fp16 score matrix s16 [R, R] of the bank against itself and the classes' row starts
    [C + 1] (host).  defect (for the CPU proof): "suspect_ge" -- equality counts as suspect; "dup_high_row" -- of two equal best
    neighbours the higher row is reported."""
    R = s16.shape[0]
    starts = [int(x) for x in starts]
    C = len(starts) - 1
    label_of = torch.zeros(R, dtype=torch.int64)
    for c in range(C):
        label_of[starts[c]:starts[c + 1]] = c
    which = range(C) if classes is None else sorted({int(c) for c in classes})
    rows = torch.tensor([r for c in which for r in range(starts[c], starts[c + 1])], dtype=torch.int64)
    labels = label_of[rows]
    n = rows.numel()
    q = s16[rows]
    rng = torch.tensor([[starts[int(c)], starts[int(c) + 1]] for c in labels], dtype=torch.int32).reshape(n, 2)
    me = torch.stack([rows, rows + 1], 1).to(torch.int32)
    in_sim, in_row = expected(q, k, rng, me)
    out_sim, out_row = expected(q, k, None, rng)
    in_row, out_row = in_row.long(), out_row.long()
    out_label = torch.where(out_row >= 0, label_of[out_row.clamp(min=0)], out_row)
    have = (in_row[:, 0] >= 0) & (out_row[:, 0] >= 0)
    a, b = out_sim[:, 0], in_sim[:, 0]
    suspect = have & (value_gt(a, b) if defect != "suspect_ge" else ~value_gt(b, a))
    # the better of the two first neighbours in the total order: larger value, then lower row; a missing neighbour loses
    out_wins = (out_row[:, 0] >= 0) & ((in_row[:, 0] < 0) | value_gt(a, b) | (~value_gt(b, a) & ((out_row[:, 0] < in_row[:, 0]) != (defect == "dup_high_row"))))
    best_row = torch.where(out_wins, out_row[:, 0], in_row[:, 0])
    best_sim = torch.where(out_wins, a, b)
    duplicate_of = torch.where((best_row >= 0) & (best_sim >= dup_threshold), best_row, torch.full_like(best_row, -1))
    return {"rows": rows, "labels": labels, "in_sim": in_sim, "in_row": in_row, "out_sim": out_sim, "out_row": out_row, "out_label": out_label,
            "suspect": suspect, "duplicate_of": duplicate_of,
            "class_suspects": torch.bincount(labels[suspect], minlength=C), "class_duplicates": torch.bincount(labels[duplicate_of >= 0], minlength=C)}


AUDIT_FIELDS = ("rows", "labels", "in_sim", "in_row", "out_sim", "out_row", "out_label", "suspect", "duplicate_of", "class_suspects", "class_duplicates")


def audit_mismatch(got, want):
    """None if every field of an audit equals the expectation (dtype, shape, values; NaN == NaN), else the first field that differs."""
    for f in AUDIT_FIELDS:
        if f not in got:
            return f"field {f} is missing"
        g, w = got[f].detach().cpu(), want[f]
        if g.dtype != w.dtype or g.shape != w.shape:
            return f"{f}: {g.dtype} {tuple(g.shape)} != {w.dtype} {tuple(w.shape)}"
        bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w))) if g.is_floating_point() else g != w
        if bool(bad.any()):
            i = tuple(int(x) for x in bad.nonzero()[0])
            return f"{f}: {int(bad.sum())} entries differ, first at {i}: expected {w[i].item()}, got {g[i].item()}"
    return None


# the planted rows of audit_bank_case as (class, offset in the class), for three class layouts: the CPU proof's, and the uniform (2 images
# per class) and ragged stores of the 8-class `tiny` model of the GPU tests
PLANTS = {
    (16, 1, 16, 5, 16, 16, 9, 16): dict(copy=((0, 1), (0, 3)), cross=((2, 2), (4, 0)), near=((7, 6), (5, 4)),
                                        equal_in=((3, 0), (3, 1), (6, 2)), equal_out=((7, 1), (7, 2), (4, 5))),
    (2, 2, 2, 2, 2, 2, 2, 2): dict(copy=((0, 0), (0, 1)), cross=((1, 1), (2, 0)), near=((4, 1), (3, 1)),
                                   equal_in=((5, 0), (5, 1), (6, 0)), equal_out=((7, 0), (7, 1), (6, 1))),
    (3, 1, 4, 2, 4, 1, 2, 4): dict(copy=((0, 0), (0, 2)), cross=((2, 3), (4, 0)), near=((7, 3), (2, 1)),
                                   equal_in=((3, 0), (3, 1), (6, 0)), equal_out=((7, 0), (7, 1), (4, 2))),
}
NEAR = 15.0 / 16.0


def audit_bank_case(D=128, lens=(16, 1, 16, 5, 16, 16, 9, 16)):
    """An exact-operand bank [sum(lens), D] with class structure, and its class starts.  Row = 1/4 on the 8 columns of its class (columns
    8 c .. 8 c + 7) and +-1/4 on 8 seeded columns of the upper half: a row scores itself 1, a class-mate 1/2 +- a little, a stranger at
    most 1/2.  Planted (PLANTS[lens], as (class, offset) pairs):
      copy: the second row is a copy of the first, inside one class;
      cross: the second row, in another class, is a copy of the first;
      near: the second row is the first (of another class) less one entry: its best match (NEAR = 15/16) lies in another class, no copy;
      equal_in: one vector three times, twice in one class and once in a LATER class: for the first two the best in-class and
        out-of-class scores are EQUAL (not suspect; the lower row, in class, is the duplicate);
      equal_out: the same with the third copy in an EARLIER class: equal again, and the lower row is the one out of class.
    The layouts with one-image classes hold a class that is never suspect.  Returns X fp16, starts (list) and the fp16 score matrix of the
    bank against itself."""
    lens = tuple(int(n) for n in lens)
    plants = PLANTS[lens]
    g = torch.Generator().manual_seed(41)
    R, C = sum(lens), len(lens)
    assert D >= 2 * 8 * C and D % 64 == 0
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    X = torch.zeros((R, D))
    for c in range(C):
        for r in range(starts[c], starts[c + 1]):
            X[r, 8 * c:8 * c + 8] = 0.25
            cols = D // 2 + torch.randperm(D // 2, generator=g)[:8]
            X[r, cols] = (torch.randint(0, 2, (8,), generator=g) * 2 - 1) * 0.25

    def row(co):
        assert co[1] < lens[co[0]]
        return starts[co[0]] + co[1]

    def recast(dst, src):
        """row dst = the seeded part of row src under the pattern of dst's class"""
        c = dst[0]
        X[row(dst)] = 0.0
        X[row(dst), 8 * c:8 * c + 8] = 0.25
        X[row(dst), D // 2:] = X[row(src), D // 2:]

    X[row(plants["copy"][1])] = X[row(plants["copy"][0])]
    X[row(plants["cross"][1])] = X[row(plants["cross"][0])]
    src, dst = plants["near"]
    X[row(dst)] = X[row(src)]
    X[row(dst), D // 2 + int((X[row(dst), D // 2:] != 0).nonzero()[0])] = 0.0
    for key in ("equal_in", "equal_out"):
        a, b, c = plants[key]
        X[row(b)] = X[row(a)]
        X[row(c)] = X[row(a)]
    X = X.half()
    assert_exact(X, X, "audit bank")
    return X, starts, N.scores16(X, X)


def plant_rows(lens):
    """{name: bank rows} of PLANTS[lens]."""
    lens = tuple(int(n) for n in lens)
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    return {k: tuple(starts[c] + o for c, o in v) for k, v in PLANTS[lens].items()}
