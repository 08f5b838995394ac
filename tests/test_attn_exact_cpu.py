"""CPU companion of test_hip_attn_exact.py: for every case and shape of attn_exact.CASES the builder keeps what the exact comparison
rests on -- the codes are far apart, no expected value sits near an fp16 rounding tie, the integer-mean expectation IS what the fp64
statement of attention (test_hip_kernels._ref_attention) gives once rounded to fp16 (for fp32: is that value exactly), every key is
addressed and every full query tile sees every placement class (the reading of "every group in every query tile" that
attn_exact.py states) -- and the comparison notices one key dropped, counted twice or read with a neighbour's V row.
Pure numpy / torch: no library, no GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import attn_exact as A
from test_hip_kernels import _ref_attention


def _ids(c):
    return c.id


def _qkv_of(built, L, bh, f32=False):
    """(q, k, v) [L, 64] int64 of (sequence, head) bh."""
    b, h = divmod(bh, A.H)
    x = built.qkv.double().view(A.B, L, 3, A.H, 64)[b, :, :, h].numpy()
    assert (x == np.round(x)).all()
    return tuple(x[:, i].astype(np.int64) for i in range(3))


@pytest.mark.parametrize("c", A.CASES, ids=_ids)
def test_case_keeps_the_exactness_conditions(c):
    built = A.build(c.kind, c.L, c.f32)           # asserts the tie margin of every expected value and the fp32 representability
    L = c.L
    assert built.qkv.shape == (A.B * L, 3 * A.H * 64) and built.want.shape == (A.B * L, A.H * 64)
    assert built.qkv.dtype == built.want.dtype == (torch.float32 if c.f32 else torch.float16)
    uniform = c.kind in ("uniform", "ucausal")
    seen_v = set()
    for bh, head in enumerate(built.heads):
        q, k, v = _qkv_of(built, L, bh)
        # 1. the code-distance condition, on the codes and on the scores they give
        assert A.min_distance(head["codes"]) >= A.MIN_DISTANCE or len(head["codes"]) == 1
        raw = q @ k.T
        if uniform:
            assert not q.any() and (np.abs(k) == 4).all()
        else:
            groups, addr = head["groups"], head["addr"]
            of_key = np.empty(L, np.int64)
            for gi, g in enumerate(groups):
                of_key[g] = gi
            match = of_key[None, :] == addr[:, None]
            assert (raw[match] == 1024).all() and int(raw[~match].max(initial=0)) <= 1024 - 32 * A.MIN_DISTANCE
            # 4. every key in exactly one group of an allowed size, every group addressed
            assert sorted(x for g in groups for x in g) == list(range(L))
            assert {len(g) for g in groups} <= ({1, 2, 4} if c.f32 else {1, 2, 3, 4})
            assert set(addr.tolist()) == set(range(len(groups))), "a group that no query addresses"
            assert (np.abs(v) >= 1).all() and (np.abs(v) <= 15).all() and len(np.unique(v, axis=0)) == L
            if c.kind == "onehot":
                assert sorted(addr.tolist()) == list(range(L)) and (L == 1 or (addr != np.arange(L)).any())
                assert torch.equal(built.want.view(A.B, L, A.H, 64)[bh // A.H, :, bh % A.H].double(), torch.from_numpy(v[addr]).double())
            else:
                if L >= 4:
                    assert {len(g) for g in groups} >= ({1, 2, 4} if c.f32 or L < 12 else {1, 2, 3, 4}) - ({4} if L < 8 else set())
                for b16 in range(16, L, 16):                                  # both sides of every 16- / 32- / 64-key boundary share a code with another key
                    assert len(groups[of_key[b16 - 1]]) >= 2 and len(groups[of_key[b16]]) >= 2
                assert L < 2 or (of_key[0] == of_key[L - 1])
                every = set().union(*(A.key_classes(x, L) for x in range(L))) | {f"size{len(g)}" for g in groups}
                if c.kind == "groups":
                    cls = [A.group_classes(g, L) for g in groups]
                    for t0 in range(0, L - 15, 16):
                        got = set().union(*(cls[i] for i in addr[t0:t0 + 16]))
                        assert got == every, f"query tile {t0 // 16} misses {every - got}"
                else:                                                         # causal: query i addresses the group of key i
                    assert (addr == of_key).all()
                    later = np.asarray([max(groups[of_key[i]]) > i for i in range(L)])
                    edges = {0} | {x for b16 in range(16, L, 16) for x in (b16 - 1, b16)}
                    assert L < 2 or all(later[i] or len(groups[of_key[i]]) >= 2 for i in edges)
                    assert L < 2 or later[0], "row 0 has no member to mask"
                    assert L < 5 or len(groups[of_key[L - 1]]) >= 2
            if c.kind != "onehot":                                              # no partial sum of a group's column cancels: one sign per (group, column)
                for g in groups:
                    assert (np.abs(np.sign(v[g]).sum(0)) == len(g)).all()
        seen_v.add(v.tobytes())
    assert len(seen_v) == A.B * A.H or (uniform and L == 1), "two (sequence, head) pairs with the same V"
    # 3. the integer-mean expectation is the fp64 statement of attention, rounded to fp16 (fp32: is it exactly)
    ref = _ref_attention(built.qkv.float(), A.B, L, A.H, c.causal)
    msg = A.mismatch(ref if c.f32 else ref.half(), built.want, L)
    assert msg is None, msg
    if not c.f32:                                                             # ... and bit for bit once +-0 is one value
        assert torch.equal(A.bits(ref.half() + 0.0), A.bits(built.want + 0.0))


def test_case_table():
    """The lengths, variants and masks of the table, and the shape constants."""
    assert (A.B * A.H) % 8 != 0
    f16 = [c for c in A.CASES if not c.f32]
    for L in (1, 5, 16, 17, 32, 33, 63, 64, 65, 77, 127, 128, 129, 144, 145):
        assert {c.kind for c in f16 if c.L == L} == {"onehot", "groups", "uniform", "causal", "ucausal"}
        assert all(c.variants == (0, 1, 3) for c in f16 if c.L == L)
    for L in (192, 193, 197, 208, 209, 256, 257, 272, 273, 320, 321, 336, 337, 577):
        assert {c.kind for c in f16 if c.L == L and c.variants == (0, 1, 3, 5)} == {"onehot", "groups", "uniform"}
        assert {c.kind for c in f16 if c.L == L and c.causal} == ({"causal", "ucausal"} if L == 197 else set())
    assert all(c.variants == (0, 1) for c in f16 if c.L == 197 and c.causal)
    f32 = [c for c in A.CASES if c.f32]
    assert {(c.kind, c.L) for c in f32} == {(k, L) for L in (6, 18, 66, 127, 128) for k in ("onehot", "groups")} | {("uniform", L) for L in (16, 64, 128)}
    assert not any(c.causal for c in f32)
    assert A.Q_L == (197, 257, 577) and A.Q_LQ == (1, 16, 17, 33) and A.THREE_L == (197, 257, 577)


def test_round_half_is_round_to_nearest_even():
    """round_half against torch's fp16 conversion on values fp64 holds exactly, and on exact ties."""
    g = np.random.default_rng(0)
    for num, den in zip(g.integers(-4000, 4000, 3000).tolist(), (2 ** g.integers(0, 12, 3000)).tolist()):
        val, _ = A.round_half(Fraction(num, den))
        assert val == float(torch.tensor(num / den, dtype=torch.float64).half())
    for fr, want in ((Fraction(2049, 1), 2048.0), (Fraction(2051, 1), 2052.0), (Fraction(-2049, 2), -1024.0), (Fraction(1, 3), float(torch.tensor(1 / 3).half())),
                     (Fraction(1, 1 << 25), 0.0), (Fraction(3, 1 << 25), 2.0 ** -23)):
        val, tie = A.round_half(fr)
        assert val == want and (tie == 0) == (fr.denominator in (1, 2, 1 << 25))
    for n in range(1, 61):                                                    # a third is a sixth of a step from the tie
        assert A.round_half(Fraction(n, 3))[1] >= Fraction(1, 6 * 2048) or n % 3 == 0
    with pytest.raises(AssertionError):
        A.quotients_fp16(np.asarray([2049]), np.asarray([1]))
    for fr, margin in A.NEAR_TIES.items():                                    # the named exceptions are needed, and keep their own margin
        assert margin <= A.round_half(fr)[1] < A.TIE_MARGIN


@pytest.mark.parametrize("L,causal", [(5, 0), (5, 1), (33, 0), (33, 1), (197, 0), (197, 1), (273, 0), (577, 0)])
def test_uniform_case_sees_one_key_dropped_or_counted_twice(L, causal):
    """Uniform weights: one key dropped or counted twice anywhere changes the fp16 value of at least one column of every row that sees the
    key (L >= 2) -- the comparison the GPU test makes is equality, so that is all it takes."""
    built = A.build("ucausal" if causal else "uniform", L)
    _, _, v = _qkv_of(built, L, 0)
    want = built.want.view(A.B, L, A.H, 64)[0, :, 0].double().numpy()
    rows = sorted({0, 1, L // 2, L - 1} - ({0} if causal else set()))
    for qi in rows:
        n = qi + 1 if causal else L
        s = v[:n].sum(0)
        assert (torch.tensor(s / n).half().double().numpy() == want[qi]).all()
        for j in range(n):
            for s2, n2 in ((s - v[j], n - 1), (s + v[j], n + 1)):
                assert (torch.tensor(s2 / n2).half().double().numpy() != want[qi]).any(), f"L = {L}, row {qi}: key {j} goes unnoticed"


@pytest.mark.parametrize("kind,L", [("groups", 17), ("groups", 197), ("causal", 145), ("groups", 577)])
def test_group_case_sees_a_weight_or_a_row_mixup(kind, L):
    """Shared-code groups: in every row, a member counted twice or dropped (groups of two and more), a key outside the group
    counted in, or the V row of the neighbouring key read for a member changes the fp16 output row."""
    built = A.build(kind, L)
    causal = kind == "causal"
    for bh in (0, A.B * A.H - 1):
        head = built.heads[bh]
        _, _, v = _qkv_of(built, L, bh)
        want = built.want.view(A.B, L, A.H, 64)[bh // A.H, :, bh % A.H].double().numpy()

        def h16(s, n):
            return torch.tensor(s / n).half().double().numpy()

        for qi in range(L):
            mem = [x for x in head["groups"][head["addr"][qi]] if not causal or x <= qi]
            s, n = v[mem].sum(0), len(mem)
            assert (h16(s, n) == want[qi]).all()
            for j in mem:
                assert n == 1 or (h16(s + v[j], n + 1) != want[qi]).any()          # (a group of one key counted twice is the same mean)
                assert n == 1 or (h16(s - v[j], n - 1) != want[qi]).any()
                assert (h16(s - v[j] + v[(j + 1) % L], n) != want[qi]).any()
            other = (mem[-1] + 1) % L
            if other not in mem:
                assert (h16(s + v[other], n + 1) != want[qi]).any()


@pytest.mark.parametrize("L", A.THREE_L)
def test_three_level_rows(L):
    """attn_exact.three_level: per query raw scores 1024, 992 and 960 on its three near keys and at most 1024 - 32 * 6 elsewhere (a far key is
    at distance >= 8 from the query's code, another code's near key at >= 6); all rows of a 32-row query tile have their three near keys in
    the same key blocks in the same order; the seven orders all occur for every (sequence, head) with seven tiles and over the heads for the
    first tile, whose block triple holds the tail block; V in [1, 2)."""
    three = A.three_level(L)
    assert three.qkv.dtype == torch.float16
    x = three.qkv.double().view(A.B, L, 3, A.H, 64)
    tail_levels = set()
    for bh, tiles in enumerate(three.tiles):
        b, h = divmod(bh, A.H)
        q, k, v = (x[b, :, i, h].numpy() for i in range(3))
        assert v.min() >= 1.0 and v.max() < 2.0
        raw = q @ k.T
        assert len(tiles) == (L + 31) // 32 and {o for o, _, _ in tiles} == set(range(7))
        for t, (order, blocks, keys) in enumerate(tiles):
            rows = range(t * 32, min(L, t * 32 + 32))
            assert (len(set(blocks)) == 3 and order < 6 and list(blocks) == sorted(blocks)) or (len(set(blocks)) == 1 and order == 6)
            for c, mine in enumerate(keys):
                if order < 6:
                    assert [mine[d] // 64 for d in range(3)] == [blocks[A.ORDERS[order][d]] for d in range(3)]
                else:
                    assert {m // 64 for m in mine} == {blocks[0]}
                tail_levels |= {(d, order) for d in range(3) if mine[d] // 64 == (L - 1) // 64}
            for i in rows:
                mine = keys[(i - t * 32) % len(keys)]
                assert [raw[i, m] for m in mine] == [1024, 992, 960]
                rest = np.delete(raw[i], mine)
                assert rest.max() <= 1024 - 32 * 6
    assert len({d for d, _ in tail_levels}) == 3, "the tail block never holds one of the three levels"
