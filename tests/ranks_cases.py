"""Exact ranking figures: the reference and the tables behind test_ranks_cpu.py, test_hip_ranks.py and test_hip_ranks_model.py.  Plain
numpy and torch, importable without a GPU.

The reference is written from the text of include/ovmr_hip_ranks.h and shares nothing with the product's host statement
(ovmr_amd/evaluator.py: rank_keys, rank_edges, rank_cells, which sort and search): `cells` counts by brute force, every score against every
edge of its class, on the selection key's bits; `cell_literal` is a second statement, value by value.  `expected` builds the state by
brute force over (b, c); `edges_of` builds a pass's edge table value by value.

`model` is a CPU model of the kernel's walk (class tiles of TILE, row chunks of CHUNK, the halving search from the top bit of the class's
edge count) that can carry ONE planted defect of DEFECTS: test_ranks_cpu.py holds the comparator to rejecting each on a named case.
"""
import struct

import numpy as np
import torch

TILE, CHUNK, MAX_ROW_BLOCKS, STAGE = 16, 64, 256, 256      # eval_ranks.hip: RK_TILE, RK_ROWS, RK_MAX_ROW_BLOCKS, RK_STAGE (held by test_ranks_cpu.py)
F32 = np.float32
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)


def value_key(v):
    """The value part of the library's selection key (csrc/eval_common.h: topk_key) of one fp32, as a Python int."""
    v = F32(v)
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    if v != v:
        return 0xFFFFFFFF
    if u == 0x80000000:
        u = 0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def keys(x):
    """value_key over an array: int64 of the same shape."""
    x = np.asarray(x, dtype=F32)
    return np.array([value_key(v) for v in x.reshape(-1)], dtype=np.int64).reshape(x.shape)


def cell_literal(x, class_edges):
    """The header's rule for ONE score against the edges of its class (strictly descending)."""
    kx = value_key(x)
    k = sum(1 for e in class_edges if value_key(e) > kx)
    return 2 * k + 1 if k < len(class_edges) and value_key(class_edges[k]) == kx else 2 * k


def clamp(estart, c, E, max_edges=None):
    """(first edge, edge count) of class c as the kernel reads them: 0 <= lo <= hi <= E whatever estart holds, at most max_edges."""
    lo = min(max(int(estart[c]), 0), E)
    hi = min(max(int(estart[c + 1]), lo), E)
    n = hi - lo
    return lo, n if max_edges is None else min(n, int(max_edges))


def cells(out, edges, estart, max_edges=None):
    """out [B, C] -> int64 [B, C], the cell of every score within its class, every score against every edge."""
    kx = keys(torch.as_tensor(out).float().numpy())
    ek = keys(np.asarray(edges, dtype=F32))
    B, C = kx.shape
    got = np.zeros((B, C), dtype=np.int64)
    for c in range(C):
        lo, n = clamp(estart, c, len(ek), max_edges)
        e = ek[lo:lo + n]
        above = (e[None, :] > kx[:, c][:, None]).sum(axis=1)
        tied = (e[None, :] == kx[:, c][:, None]).any(axis=1)
        got[:, c] = 2 * above + tied
    return got


def expected(out, y, edges, estart, max_edges=None, state=None):
    """The state after one call, by brute force over (b, c): int64 [2, 2E + C] (added to `state` if given)."""
    B, C = out.shape
    E = len(edges)
    cell = cells(out, edges, estart, max_edges)
    want = np.zeros((2, 2 * E + C), dtype=np.int64) if state is None else torch.as_tensor(state).long().numpy().copy()
    yy = torch.as_tensor(y).numpy()
    for b in range(B):
        if not 0 <= int(yy[b]) < C:
            continue
        for c in range(C):
            want[1 if int(yy[b]) == c else 0, 2 * clamp(estart, c, E)[0] + c + cell[b, c]] += 1
    return torch.from_numpy(want)


def edges_of(out, y, C):
    """The edge table of a pass, value by value: per class the distinct scores of its own rows, canonical (one NaN, +0), descending in
    key order -> (edges fp32 [E], estart int32 [C + 1]) as numpy."""
    x = torch.as_tensor(out).float().numpy()
    yy = torch.as_tensor(y).numpy()
    edges, estart = [], [0]
    for c in range(C):
        by_key = {}
        for b in np.nonzero(yy == c)[0]:
            v = x[b, c]
            by_key[value_key(v)] = F32(np.nan) if v != v else (F32(0.0) if v == 0 else v)
        edges += [by_key[k] for k in sorted(by_key, reverse=True)]
        estart.append(len(edges))
    return np.array(edges, dtype=F32), np.array(estart, dtype=np.int32)


def specials(fp16=False):
    """The values the order can go wrong at: NaN of both signs and other payloads, +-inf, +-0, denormals of either sign, the extremes."""
    dt = np.float16 if fp16 else F32
    tiny = np.nextafter(dt(0), dt(1))
    fin = np.finfo(dt)
    v = [dt(np.inf), dt(-np.inf), dt(0.0), dt(-0.0), tiny, -tiny, dt(3) * tiny, dt(-2) * tiny, fin.max, fin.min, fin.tiny, -fin.tiny,
         dt(1), np.nextafter(dt(1), dt(0)), np.nextafter(dt(1), dt(2)), dt(-1)]
    out = np.array([F32(e) for e in v], dtype=F32)
    nans = np.array(NAN_BITS[:2] if fp16 else NAN_BITS, dtype=np.uint32).view(F32)
    return np.concatenate([out, nans])


def make_edges(counts, seed=0, special=False, fp16=False):
    """An edge table with counts[c] edges for class c: distinct values (multiples of 2^-10 in [-2, 2), exact in fp16; with `special` the
    table of specials() mixed in, one NaN at most and one zero), strictly descending in key order."""
    rng = np.random.default_rng(seed + 5)
    edges, estart = [], [0]
    for n in counts:
        pool = (rng.choice(4096, size=min(n, 4096), replace=False).astype(F32) - 2048) / 1024 if n else np.zeros(0, dtype=F32)
        if special and n:
            sp = specials(fp16)
            take = sp[rng.permutation(len(sp))[:min(n, len(sp))]]
            pool = np.concatenate([take, pool])
        by_key = {}
        for v in pool:
            by_key.setdefault(value_key(v), F32(np.nan) if v != v else (F32(0.0) if v == 0 else v))
        ks = sorted(by_key, reverse=True)[:n]
        assert len(ks) == n, (n, len(ks))
        edges += [by_key[k] for k in ks]
        estart.append(len(edges))
    return np.array(edges, dtype=F32), np.array(estart, dtype=np.int32)


def scores(B, C, edges, estart, kind="mixed", fp16=False, seed=0):
    """[B, C] scores (torch, fp16 or fp32): `mixed` -- a third of each column drawn from the class's own edges (ties), the rest continuous
    between and beyond them; `special` -- mixed, with specials() spread over rows and columns; `softmax` -- softmax rows (nearly every
    negative below every edge); `equal` -- one value everywhere."""
    rng = np.random.default_rng(seed)
    if kind == "equal":
        x = np.full((B, C), 0.25, dtype=F32)
    elif kind == "softmax":
        z = rng.standard_normal((B, C)) * 3
        x = np.exp(z - z.max(axis=1, keepdims=True))
        x = (x / x.sum(axis=1, keepdims=True)).astype(F32)
    else:
        x = rng.uniform(-2.5, 2.5, size=(B, C)).astype(F32)
        for c in range(C):
            lo, n = clamp(estart, c, len(edges))
            if n:
                rows = rng.permutation(B)[:max(1, B // 3)]
                x[rows, c] = edges[lo + rng.integers(0, n, size=len(rows))]
        if kind == "special":
            sp = specials(fp16)
            where = rng.permutation(B * C)[:min(B * C // 2, 4 * len(sp))]
            x.reshape(-1)[where] = sp[rng.integers(0, len(sp), size=len(where))]
    t = torch.from_numpy(x)
    return t.half() if fp16 else t


def labels(B, C, kind="random", seed=0):
    """int64 [B]: `random`; `hot` (every row the same label); `bad` (random, with -1, C, 2^40 and the int64 extremes among them)."""
    rng = np.random.default_rng(seed + 17)
    y = rng.integers(0, C, size=B).astype(np.int64)
    if kind == "hot":
        y[:] = C // 2
    elif kind == "bad":
        bad = [-1, C, 2 ** 40, -2 ** 63, 2 ** 63 - 1, C + 2 ** 32, -2 ** 32]          # (the last two: equal to a class in their low 32 bits)
        pos = rng.permutation(B)[:max(1, min(B // 2, len(bad)))]
        y[pos] = np.array(bad[:len(pos)], dtype=np.int64)
    return torch.from_numpy(y)


DEFECTS = ["tie_in_gap", "neg_zero_differs", "nan_lowest", "base_without_c", "planes_swapped", "last_cell_dropped", "neighbour_edges",
           "estart_unclamped"]


def _defect_key(v, defect):
    v = F32(v)
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    if v != v:
        return 0 if defect == "nan_lowest" else 0xFFFFFFFF
    if u == 0x80000000 and defect != "neg_zero_differs":
        u = 0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def model(out, y, edges, estart, max_edges, state, defect=None):
    """The kernel's walk on the host: class tiles of TILE, row chunks of CHUNK, per score the halving search from the top bit of the
    class's edge count, each (class, chunk) added to `state` (int64 [2, 2E + C], in place) -- with one of DEFECTS planted, or none.
    -> (state, adds that fell outside the state: 0 for the honest model whatever estart holds)."""
    B, C = out.shape
    E = len(edges)
    x = torch.as_tensor(out).float().numpy()
    yy = torch.as_tensor(y).numpy()
    st = state.numpy().reshape(-1)
    plane = 2 * E + C
    ek = [_defect_key(e, defect) for e in edges]
    outside = 0
    for c0 in range(0, C, TILE):
        for r0 in range(0, B, CHUNK):
            for c in range(c0, min(c0 + TILE, C)):
                if defect == "estart_unclamped":
                    lo, n = int(estart[c]), min(int(estart[c + 1]) - int(estart[c]), max_edges)
                else:
                    lo, n = clamp(estart, c, E, max_edges)
                src = clamp(estart, min(c + 1, C - 1), E, max_edges)[0] if defect == "neighbour_edges" else lo
                for b in range(r0, min(r0 + CHUNK, B)):
                    if not 0 <= int(yy[b]) < C:
                        continue
                    kx = _defect_key(x[b, c], defect)
                    pos, step = 0, (1 << (n.bit_length() - 1)) if n > 0 else 0
                    edge = lambda i: ek[src + i] if 0 <= src + i < E else 0           # noqa: E731
                    while step:
                        if pos + step <= n and edge(pos + step - 1) > kx:
                            pos += step
                        step >>= 1
                    tie = pos < n and edge(pos) == kx and defect != "tie_in_gap"
                    cell = 2 * pos + int(tie)
                    if defect == "last_cell_dropped" and cell == 2 * n:
                        continue
                    own = int(int(yy[b]) == c)
                    if defect == "planes_swapped":
                        own = 1 - own
                    at = own * plane + 2 * lo + (0 if defect == "base_without_c" else c) + cell
                    if 0 <= at < len(st):
                        st[at] += 1
                    else:
                        outside += 1
    return state, outside


def mismatch(got, want):
    """None where the two states are equal, else the count and the first cell that differs."""
    got, want = torch.as_tensor(got).long(), torch.as_tensor(want).long()
    if got.shape != want.shape:
        return f"shape {list(got.shape)} != {list(want.shape)}"
    bad = (got != want).nonzero()
    if len(bad) == 0:
        return None
    p, i = (int(v) for v in bad[0])
    return f"{len(bad)} of {got.numel()} cells differ, the first at plane {p}, cell {i} of {got.shape[1]}: got {int(got[p, i])}, expected {int(want[p, i])}"


def random_state(C, E, seed=0, high=50):
    rng = np.random.default_rng(seed + 99)
    return torch.from_numpy(rng.integers(0, high, size=(2, 2 * E + C)).astype(np.int64))
