"""Cases, expectations and the comparator for the nearest-exemplar search (ovmr_amd/csrc/nearest.hip, include/ovmr_hip_nearest.h).
Plain torch, no library: shared by test_hip_nearest.py (GPU) and test_nearest_cpu.py (which proves that the comparator rejects the defects
it is there for).

Exact operands (the method of head_exact.py).  Queries and bank rows are sparse with dyadic entries, every product is a multiple of 2^-p and
sum_k |product| < 2^(24 - p) (assert_exact): every partial sum is exact in fp32 in any K order, so the score h(acc) is ONE fp16 number
and the expectation is torch.sort(stable=True, descending=True) of the CPU's fp16 score matrix -- larger first, equal scores in increasing
row order, NaN above +inf, -0 == +0: the library's total order -- bit for bit in the indices.  Values are compared as numbers, NaN equal
to NaN: the key the kernel orders by does not tell -0 from +0 (include/ovmr_hip_nearest.h reports +0 for either).

General operands.  L2-normalised clustered features; the K order is free, so the comparison is by margin (general_mismatch).
"""
import math

import torch

from head_exact import _sparse, assert_exact

TILE = 256                                   # bank rows per tile of the kernel
KMAX = 32

# (B, R, D, k): every B in {1, 63, 64, 65, 130}, R in {1, k, 255, 256, 257, 1000, 70001}, D in {64, 128, 512, 768, 1024}, k in {1, 5, 31, 32};
# 32-query tiles (B <= 32, or D = 1024 where 64 queries do not fit LDS) and 64-query tiles, with and without spare query rows.
SHAPES = [
    (1, 1, 64, 1), (1, 5, 128, 5), (63, 255, 64, 5), (64, 256, 128, 31), (65, 257, 512, 32), (130, 1000, 768, 5), (65, 1000, 1024, 32),
    (64, 32, 1024, 32), (63, 31, 768, 31), (1, 257, 1024, 1), (130, 1000, 128, 32), (65, 256, 64, 1), (130, 70001, 64, 32), (64, 70001, 128, 5),
]


def n_tiles(R):
    return (R + TILE - 1) // TILE


def slices_for(R):
    """The forced slice counts of a case: 1, 2, 3 and one per tile (and one more than that: the last slice stays empty)."""
    return sorted({1, 2, 3, n_tiles(R), n_tiles(R) + 1})


def scores16(Q, X):
    """The fp16 score matrix: the fp64 product (exact for exact operands, NaN / inf propagate), ONE rounding to fp16.  Row blocks keep the
    fp64 copies small."""
    Xd = X.double().t().contiguous()
    return torch.cat([(Q[i:i + 16].double() @ Xd).half() for i in range(0, Q.shape[0], 16)]) if Q.shape[0] else torch.zeros((0, X.shape[0]), dtype=torch.float16)


def expected(s16, k, ranges=None, tail_index=-1):
    """(values fp32 [B, k], indices int32 [B, k]) of the library's order on the score matrix s16 [B, R]: torch.sort(stable, descending);
    with ranges [B, 2], row b sorts its rows lo <= r < hi only and pads its tail with (tail_index, -inf)."""
    B, R = s16.shape
    s = s16.float()
    if ranges is None:
        v, i = torch.sort(s, dim=1, descending=True, stable=True)
        return v[:, :k].contiguous(), i[:, :k].to(torch.int32).contiguous()
    vals = torch.full((B, k), -math.inf)
    idx = torch.full((B, k), tail_index, dtype=torch.int32)
    for b in range(B):
        lo, hi = int(ranges[b, 0]), int(ranges[b, 1])
        v, i = torch.sort(s[b, lo:hi], descending=True, stable=True)
        n = min(k, hi - lo)
        vals[b, :n] = v[:n]
        idx[b, :n] = (i[:n] + lo).to(torch.int32)
    return vals, idx


def brute_force(s16, k, ranges=None):
    """The same order spelled out element by element (tiny cases only): a Python sort on (NaN first, value descending with -0 == +0, row)."""
    B, R = s16.shape
    vals, idx = [], []
    for b in range(B):
        lo, hi = (0, R) if ranges is None else (int(ranges[b, 0]), int(ranges[b, 1]))
        rows = []
        for r in range(lo, hi):
            x = float(s16[b, r])
            rows.append((0 if x != x else 1, 0.0 if x != x else -x, r, x))       # -(-0.0) == 0.0: the zeros tie
        rows.sort(key=lambda t: t[:3])
        rows = rows[:k]
        vals.append([t[3] for t in rows] + [-math.inf] * (k - len(rows)))
        idx.append([t[2] for t in rows] + [-1] * (k - len(rows)))
    return torch.tensor(vals, dtype=torch.float32).reshape(B, k), torch.tensor(idx, dtype=torch.int32).reshape(B, k)


def mismatch(got, want):
    """None if (values, indices) equal the expectation -- indices bit for bit, values as numbers with NaN == NaN -- else the first
    differing (query, rank)."""
    (gv, gi), (wv, wi) = got, want
    gv, gi = gv.detach().cpu(), gi.detach().cpu()
    if gv.shape != wv.shape or gi.shape != wi.shape:
        return f"shapes {tuple(gv.shape)} / {tuple(gi.shape)} != {tuple(wv.shape)} / {tuple(wi.shape)}"
    if gv.dtype != torch.float32 or gi.dtype != torch.int32:
        return f"dtypes {gv.dtype} / {gi.dtype}"
    bad = (gi != wi) | ~((gv == wv) | (torch.isnan(gv) & torch.isnan(wv)))
    if not bool(bad.any()):
        return None
    b, j = (int(x) for x in bad.nonzero()[0])
    return (f"{int(bad.sum())} entries differ, first at query {b}, rank {j}: expected row {int(wi[b, j])} ({float(wv[b, j])}), "
            f"got row {int(gi[b, j])} ({float(gv[b, j])})")


# ---- exact cases ----------------------------------------------------------------------------------------------------------------

def dup_pairs(R):
    """(lo, hi): bank row hi is a copy of row lo -- inside one 32-row MFMA block, across two tiles (of one slice at slices = 1, of two at
    one slice per tile), in the first and the last tile."""
    pairs = []
    if R >= 8:
        pairs.append((1, 2))
    if R >= 320:
        pairs.append((6, 300))
    if R >= 3 * TILE:
        pairs.append((9, (n_tiles(R) - 1) * TILE + 3 if (n_tiles(R) - 1) * TILE + 3 < R else R - 1))
    return pairs


def exact_case(B, R, D, k, seed, nan_row=None, inf_row=None):
    """fp16 Q [B, D] +-(1..3)/8 and X [R, D] +-(1..4)/16, exact (asserted).  Planted as far as there is room: duplicate bank rows
    (dup_pairs), queries 1, 5, 9, .. aligned with the lower row of a pair (the pair takes the first two ranks, lower row first), queries
    b % 8 == 3 all zero (every score +0: the answer is rows 0 .. k-1).  nan_row: that bank row gets a NaN (it ranks first for everyone);
    inf_row: that bank row holds 65504 in the reserved last column alone and queries b % 5 == 2 hold +-65504 there (+-inf scores).
    Returns Q, X and the fp16 score matrix."""
    g = torch.Generator().manual_seed(seed)
    wide = D > 256
    X = _sparse(g, R, D, 12 if wide else 8, 16, 4)
    Q = _sparse(g, B, D, 24 if wide else 16, 8, 3)
    pairs = dup_pairs(R)
    for lo, hi in pairs:
        X[hi] = X[lo]
    for b in range(B):
        if b % 4 == 1 and pairs:
            lo = pairs[(b // 4) % len(pairs)][0]
            Q[b] = torch.sign(X[lo]) * 0.375
        elif b % 8 == 3:
            Q[b] = 0.0
    Q, X = Q.half(), X.half()
    assert_exact(Q, X, f"B={B} R={R} D={D}")
    if inf_row is not None and inf_row < R:
        X[inf_row] = 0.0
        X[inf_row, D - 1] = 65504.0
        for b in range(2, B, 5):
            Q[b, D - 1] = 65504.0 if b % 2 else -65504.0
    if nan_row is not None and nan_row < R:
        X[nan_row, 0] = math.nan
    return Q, X, scores16(Q, X)


def tie_cut_case(k=2, R=600, D=128, B=5):
    """Rows 3, 290 and 580 are one vector, the best for every query: at k = 2 the tie decides MEMBERSHIP (3 and 290 are in, 580 is out)."""
    Q, X, _ = exact_case(B, R, D, k, 77)
    v = torch.zeros(D, dtype=torch.float16)
    v[:16] = 0.25
    for r in (3, 290, 580):
        X[r] = v
    Q[:, :16] = 0.375
    assert_exact(Q, X, "tie cut")
    return Q, X, scores16(Q, X)


def zero_bank_case(B=5, R=1000, D=64):
    g = torch.Generator().manual_seed(5)
    return _sparse(g, B, D, 16, 8, 3).half(), torch.zeros((R, D), dtype=torch.float16), torch.zeros((B, R), dtype=torch.float16)


def signed_zero_case(B=3, R=700, D=64):
    """Scores of -2^-26 and +2^-26 round to -0 and +0 among +0s: all equal, the rows come in increasing order; row R - 1 scores 2^-13."""
    Q = torch.zeros((B, D), dtype=torch.float16)
    Q[:, 0] = 2.0 ** -13
    X = torch.zeros((R, D), dtype=torch.float16)
    X[5, 0] = -2.0 ** -13
    X[2, 0] = 2.0 ** -13
    X[300, 0] = -2.0 ** -13
    X[R - 1, 0] = 1.0
    s = scores16(Q, X)
    assert bool(torch.signbit(s[0, 5])) and float(s[0, 5]) == 0.0 and not bool(torch.signbit(s[0, 2])) and float(s[0, R - 1]) > 0
    return Q, X, s


def range_table(B, R, k, slices=2):
    """int32 [B, 2]: cycling through an empty range, one row, fewer than k rows, a tile boundary, a slice boundary (of `slices` slices), the
    whole bank; from query 64 on (a query tile of their own) every range lies in the first 100 rows: the workgroups of all later slices
    have nothing to do."""
    T = n_tiles(R)
    cut = min(R - 1, ((T + slices - 1) // slices) * TILE)
    kinds = [(17, 17), (R - 1, R), (40, 40 + max(1, k - 2)), (TILE - 6, TILE + 6), (cut - 12, cut + 18), (0, R), (R, R), (3, 3 + k)]
    rows = []
    for b in range(B):
        lo, hi = kinds[b % len(kinds)]
        if b >= 64:
            lo, hi = min(lo, 60), min(hi, 100)
        rows.append((max(0, min(lo, R)), max(0, min(hi, R))))
    rows = [(lo, max(lo, hi)) for lo, hi in rows]
    return torch.tensor(rows, dtype=torch.int32).reshape(B, 2)


# ---- the bank of just over 2^31 bytes, stated analytically ---------------------------------------------------------------------------

BIG_D = 128
BIG_R = 2 ** 31 // (2 * BIG_D) + 300          # 8 388 908 rows of 256 bytes: 2^31 + 76 800 bytes


def big_bank_plan(k, B=3):
    """Q [B, 128] and the planted rows {row: (x0, x1)} of an otherwise zero bank [BIG_R, 128]: the score of a planted row is
    q0 x0 + q1 x1, every other row scores +0.  Rows 0 .. k hold small positive values, decreasing (k + 1 of them: the last is cut), the last tile
    holds the best row, a copy of row 0 (it loses the tie) and a negative row (below all the zeros)."""
    Q = torch.zeros((B, BIG_D), dtype=torch.float16)
    Q[:, 0] = 0.25
    Q[:, 1] = torch.arange(B).half() * 0.25
    planted = {r: ((k + 1 - r) / 64.0, 0.0) for r in range(k + 1)}
    planted[BIG_R - 1] = (2.0, 1.0)
    planted[BIG_R - 200] = planted[0]
    planted[BIG_R - 77] = (-1.0, 0.0)
    planted[2 ** 31 // (2 * BIG_D)] = (1.0, -0.5)                # the first row past 2^31 bytes
    return Q, planted


def big_bank_expected(Q, planted, k, alias=None):
    """The expectation from the planted rows alone: their scores, and +0 for the lowest unplanted rows that can still make the list.
    alias: a model of a 32-bit byte offset -- rows from `alias` on read the contents of row r - alias."""
    rows = sorted(planted)
    zeros = [r for r in range(k + len(rows) + 1) if r not in planted][:k]
    content = dict(planted)
    if alias:
        for r in rows:
            if r >= alias:
                content[r] = planted.get(r - alias, (0.0, 0.0))
        zeros = [r for r in zeros if r < alias]
    cand = rows + zeros
    Xs = torch.tensor([content.get(r, (0.0, 0.0)) for r in cand], dtype=torch.float64)
    s = (Q[:, :2].double() @ Xs.t()).half().float()              # [B, n] scores of the candidates
    order = sorted(range(len(cand)), key=lambda i: cand[i])
    s, cand = s[:, order], [cand[i] for i in order]              # increasing row order: the stable sort breaks ties by row
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    idx = torch.tensor(cand, dtype=torch.int64)[i[:, :k]].to(torch.int32)
    return v[:, :k].contiguous(), idx.contiguous()


def big_bank_fill(X, planted):
    """Writes the planted rows into a zero bank tensor [BIG_R, 128] (any device)."""
    for r, (x0, x1) in planted.items():
        X[r, 0] = x0
        X[r, 1] = x1
    return X


# ---- general operands ---------------------------------------------------------------------------------------------------------------

def general_case(D, seed, classes=50, per_class=20, B=100):
    """L2-normalised fp16 features with trained-like clustering: classes x per_class bank rows around class centres, queries near centres."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn((classes, D), generator=g), dim=1)
    X = centres.repeat_interleave(per_class, 0) + 0.5 * torch.randn((classes * per_class, D), generator=g) / math.sqrt(D)
    Q = centres[torch.randint(0, classes, (B,), generator=g)] + 0.5 * torch.randn((B, D), generator=g) / math.sqrt(D)
    return torch.nn.functional.normalize(Q, dim=1).half(), torch.nn.functional.normalize(X, dim=1).half()


def margin(D, smax=1.0):
    """m = 2 (2^-12 + D 2^-24): half an fp16 step at |s| <= 1 plus the fp32 accumulation bound, on each side of the cut.  Where the
    fp64 scores themselves reach beyond 1 (an fp16-normalised feature against itself: 1 + a few 2^-11), the fp16 step is 2^-10 up to 2
    and the bound scales with it: m = 2 (2^-11 + 2 D 2^-24)."""
    assert smax < 2.0
    return 2.0 * (2.0 ** -12 + D * 2.0 ** -24) * (1.0 if smax <= 1.0 else 2.0)


def general_mismatch(got, Q, X, k, ranges=None):
    """None, or what is wrong: every returned row must score (fp64) at least the k-th best fp64 score - m, every value must lie within m / 2
    of its row's fp64 score, values must not increase and equal values come in increasing row order."""
    gv, gi = got[0].detach().cpu().double(), got[1].detach().cpu().long()
    s = Q.double() @ X.double().t()
    m = margin(Q.shape[1], float(s.abs().max()))             # (the reference's own scores say which fp16 binade the bound is for)
    B, R = s.shape
    for b in range(B):
        lo, hi = (0, R) if ranges is None else (int(ranges[b, 0]), int(ranges[b, 1]))
        n = min(k, hi - lo)
        if bool((gi[b, n:] != -1).any()) or bool((gv[b, n:] != -math.inf).any()):
            return f"query {b}: tail past {n} eligible rows is not (-1, -inf)"
        if n == 0:
            continue
        rows = gi[b, :n]
        if bool(((rows < lo) | (rows >= hi)).any()) or rows.unique().numel() != n:
            return f"query {b}: rows {rows.tolist()} outside [{lo}, {hi}) or repeated"
        kth = torch.sort(s[b, lo:hi], descending=True).values[n - 1]
        if bool((s[b, rows] < kth - m).any()):
            return f"query {b}: a returned row scores {float(s[b, rows].min())}, the k-th best is {float(kth)} (margin {m})"
        if bool(((gv[b, :n] - s[b, rows]).abs() > m / 2).any()):
            return f"query {b}: a value is {float((gv[b, :n] - s[b, rows]).abs().max())} from its row's score (m / 2 = {m / 2})"
        d = gv[b, 1:n] - gv[b, :n - 1]
        if bool((d > 0).any()) or bool(((d == 0) & (rows[1:] < rows[:-1])).any()):
            return f"query {b}: values increase, or equal values are not in increasing row order"
    return None


# ---- a model of the two launches on a score matrix, with the defects the comparator must reject ------------------------------------------

def _key(x, r, ties_high=False):
    nan = x != x
    return (0 if nan else 1, 0.0 if nan else -x, -r if ties_high else r)


def simulate(s16, k, ranges=None, slices=1, defect=None, s32=None, t_bad=0):
    """The search the way nearest.hip computes it -- per slice of whole tiles the k best keys, then the k best of all slices -- on the score
    matrix, optionally with ONE defect:
      "ties_high": equal scores go to the higher row;          "unrounded": ordered by the fp32 scores s32, values from s16;
      "drop_tile": tile t_bad's rows never become candidates;  "dedup_merge": the slice merge keeps one of several equal scores;
      "range_inclusive": a range's end row is eligible;        "tail_zero": an unfilled rank holds index 0."""
    B, R = s16.shape
    T = n_tiles(R)
    per = (T + slices - 1) // slices
    vals = torch.full((B, k), -math.inf)
    idx = torch.full((B, k), 0 if defect == "tail_zero" else -1, dtype=torch.int32)
    for b in range(B):
        lo, hi = (0, R) if ranges is None else (int(ranges[b, 0]), int(ranges[b, 1]))
        if defect == "range_inclusive" and ranges is not None:
            hi = min(R, hi + 1)
        merged = []
        for s in range(slices):
            a, e = max(lo, s * per * TILE), min(hi, (s + 1) * per * TILE)
            rows = [r for r in range(a, e) if not (defect == "drop_tile" and r // TILE == t_bad)]
            order = (s32 if defect == "unrounded" else s16)[b]
            rows.sort(key=lambda r: _key(float(order[r]), r, defect == "ties_high"))
            merged += rows[:k]
        order = (s32 if defect == "unrounded" else s16)[b]
        merged.sort(key=lambda r: _key(float(order[r]), r, defect == "ties_high"))
        if defect == "dedup_merge":
            seen, kept = set(), []
            for r in merged:
                x = float(s16[b, r])
                if x not in seen:
                    kept.append(r)
                    seen.add(x)
            merged = kept
        merged = merged[:k]
        for j, r in enumerate(merged):
            vals[b, j] = float(s16[b, r])
            idx[b, j] = r
    return vals, idx
